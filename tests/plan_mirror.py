"""The one Python mirror of the sampling path's launch plan (csrc/mst_plan.h) and of the defaults it is called with.

plan_trunk / rows_ntb / plan_slices / slice_of and plan_embed_in / embed_next_ksn / plan_embed_out restate the header function by
function; tests/test_launch_plan_cpu.py compares them with the header itself, field by field, on the CPU.  The names below them
(embed_in_kernel, embed_out_kernel, plain_path, trunk_path, slices, loop_slices, slices_of) are what the GPU test modules put into
their case ids and path tables."""

# csrc/mst_engine.hip defaults
SMALL_M = 1900                          # small_m (MST_SMALL_M): launches of at most this many token rows take the small path
SMALL_LN_M = 512                        # small_ln_m (MST_SMALL_LN_M): ... with the LayerNorms inside the 16-row GEMMs up to this many rows
NTB1_M, NTB2_FROM = 800, 1300           # g_rows_ntb1_m / g_rows_ntb2_from (MST_SMALL_NTB1_M / MST_SMALL_NTB2_FROM, read at load)

# PlanKnobs, in the struct's order, at the engine's defaults (8 layers: the model's)
KNOBS = dict(small_m=SMALL_M, small_ln=1, small_ln_m=SMALL_LN_M, small_fast=1, precise=0, fuse_qkv_attn=1, fuse_tail=1, tail_ntb=0,
             ln128_min_m=1 << 30, trunk_groups=0, num_layers=8, nsplit=0, dbg_stop=0)
PATHS = ("small-ring", "small-rows", "small-rows-ln", "resident", "large")          # TrunkPath
QKV_ATTN = ("unfused", "streamed", "ring")                                           # QkvAttn
PLAN_FIELDS = ("path", "precise", "lnf", "qkv_attn", "fuse_tail", "ln128", "tail_ntb", "nt16")      # TrunkPlan


def knobs(**over):
    assert set(over) <= set(KNOBS), over
    return {**KNOBS, **{k: int(v) for k, v in over.items()}}


def plan_trunk(k, rows, T, slices=1, instrumented=False):
    """mst::plan_trunk: TrunkPlan as a dict (path and qkv_attn as indices into PATHS / QKV_ATTN)."""
    S = T + 1
    M = rows * S
    small = bool(k["precise"]) or (k["small_m"] > 0 and M <= k["small_m"])
    precise = bool(k["precise"]) or (small and T <= 16)
    fast = small and not precise and bool(k["small_fast"])
    lnf = fast and bool(k["small_ln"]) and not k["dbg_stop"] and M <= k["small_ln_m"]
    n16 = (S + 15) // 16
    resident = bool(k["trunk_groups"] and n16 == 13 and k["fuse_qkv_attn"] == 1 and k["fuse_tail"] and k["tail_ntb"] == 0
                    and not k["dbg_stop"] and not k["precise"] and k["num_layers"] <= 8 and not instrumented)
    if small:
        path = "small-rows-ln" if lnf else "small-rows" if fast else "small-ring"
    else:
        path = "resident" if resident else "large"
    qkv = "unfused" if not k["fuse_qkv_attn"] else "streamed" if k["fuse_qkv_attn"] == 1 and S <= 208 else "ring"
    ntb = k["tail_ntb"] or 4
    if not k["tail_ntb"] and slices == 1:
        if (M + 31) // 32 <= 256:
            ntb = 2
        elif (M + 47) // 48 <= 256:
            ntb = 3
    return dict(path=PATHS.index(path), precise=int(precise), lnf=int(lnf), qkv_attn=QKV_ATTN.index(qkv), fuse_tail=int(bool(k["fuse_tail"])),
                ln128=int(M >= k["ln128_min_m"]), tail_ntb=ntb, nt16=13 if n16 == 13 else (n16 + 1) // 2 * 2)


def rows_ntb(M, ntb1_m=NTB1_M, ntb2_from=NTB2_FROM):
    """mst::rows_ntb: 16-token blocks per tile of a rows GEMM over M rows."""
    return 1 if M <= ntb1_m else 2 if M > ntb2_from else 4


def plan_slices(k, batch, cfg, frames):
    """mst::plan_slices: clip slices of a loop over `batch` clips."""
    if k["dbg_stop"]:
        return 1
    rows = (2 if cfg else 1) * batch
    n = k["nsplit"]
    if n == 0:
        path = PATHS[plan_trunk(k, rows, frames)["path"]]
        if path == "resident":
            return 1
        tiles = (rows * (frames + 1) + 63) // 64
        waves = (tiles + 255) // 256
        n = 3 if path != "large" else min(waves, 3)
        if path == "large" and waves == 1 and tiles >= 192:
            n = 3
    while n > 1 and rows // n < 8:
        n -= 1
    return n


def slice_of(batch, n, i):
    """mst::slice_of: (first clip, clips) of slice i; clips <= 0: the slice is empty."""
    per = -(-batch // n)
    c0 = i * per
    return c0, per if c0 + per <= batch else batch - c0


# ------------------------------------------------------------------------------ the two projections (K3, K9)
EMBED_BT, EMBED_SMEM = 64, 160 * 1024                                    # EmbCfg::BT / EmbCfg::SMEM
EMBED_KERNELS = ("latency", "ring")                                      # EmbedKernel
EMBED_IN_FIELDS = ("kin_pad", "ks", "kernel")                            # EmbedInPlan
EMBED_OUT_FIELDS = ("kernel", "nbw", "nx", "staged", "ksn", "ring_bf", "ring_xs")      # EmbedOutPlan


def embed_kin_pad(feats):
    return max(96, -(-feats // 32) * 32)


def embed_out_nbw(feats):
    return -(-feats // 128)


def plan_embed_in(feats, precise=False, embed_fast=True):
    """mst::plan_embed_in: EmbedInPlan as a dict (kernel as an index into EMBED_KERNELS)."""
    kp = embed_kin_pad(feats)
    return dict(kin_pad=kp, ks=kp // 32, kernel=EMBED_KERNELS.index("latency" if embed_fast and not precise else "ring"))


def embed_next_ksn(feats, T, precise=False, embed_fast=True):
    """mst::embed_next_ksn: KSN of the fused next-step embedding, or 0."""
    ks, nbw = embed_kin_pad(feats) // 32, embed_out_nbw(feats)
    if not embed_fast or precise or T % 4:
        return 0
    if (ks, nbw) not in ((5, 2), (6, 2), (9, 3)):
        return 0
    return ks if feats * (EMBED_BT + 4) * 4 + 16 + 2 * EMBED_BT * (ks * 64 + 16) <= EMBED_SMEM else 0


def plan_embed_out(feats, T, cfg=False, precise=False, embed_fast=True, mode=0, hi_lo=True, custom_w=False):
    """mst::plan_embed_out: EmbedOutPlan as a dict."""
    nbw = embed_out_nbw(feats)
    p = dict.fromkeys(EMBED_OUT_FIELDS, 0)
    p["nx"] = 2 if cfg else 1
    if embed_fast and not precise and hi_lo and not custom_w and not (cfg and nbw == 4):
        p.update(kernel=EMBED_KERNELS.index("latency"), nbw=nbw, staged=int(mode != 0 and nbw <= 3 and T % 4 == 0),
                 ksn=embed_next_ksn(feats, T, precise, embed_fast) if mode != 0 and not cfg else 0)
        return p
    bf = 256 if feats <= 256 else 384 if feats <= 384 else 512
    p.update(kernel=EMBED_KERNELS.index("ring"), ring_bf=bf, ring_xs=2 if hi_lo and bf <= 384 else 1)
    return p


def embed_in_kernel(feats, precise=False):
    """The pose embedding a sampling launch runs, by name."""
    p = plan_embed_in(feats, precise)
    return f"k_embed_in<{p['ks']}>" if EMBED_KERNELS[p["kernel"]] == "latency" else f"ring-in<kpad {p['kin_pad']}>"


def embed_out_kernel(feats, T, cfg=False, precise=False, mode=0, fused_next=False):
    """The output projection of a sampling launch over the last (split) stream, by name; fused_next: the step also embeds the next."""
    p = plan_embed_out(feats, T, cfg, precise, True, mode)
    if EMBED_KERNELS[p["kernel"]] == "ring":
        return f"launch_out_nx<{mode}, {p['ring_bf']}, NX {p['nx']}, XS {p['ring_xs']}>"
    if fused_next:
        assert p["ksn"], (feats, T, mode)
        return f"k_embed_out<{p['nbw']}, {mode}, 1, {p['ksn']}>"
    return f"k_embed_out<{p['nbw']}, {mode}, {p['nx']}>"


# ------------------------------------------------------------------------------ what the GPU tests name their cases by
def slices_of(B, n):
    """The non-empty slices of B clips in n slices: [(first clip, clips)]."""
    return [s for s in (slice_of(B, n, i) for i in range(n)) if s[1] > 0]


def plain_path(rows, T, small_m=SMALL_M, precise=False):
    """The path of one single-style launch sequence over `rows` transformer rows of T frames, as the profile families tell them apart."""
    p = plan_trunk(knobs(small_m=small_m, precise=precise), rows, T)
    path = PATHS[p["path"]]
    if path in ("large", "resident"):
        return "fused-large-tile"
    if p["precise"]:
        return "small-tile-hi-lo"        # every activation as hi + lo: engine precise mode, or clips of <= 16 frames
    return "small-launch-ln-in-gemm" if path == "small-rows-ln" else "small-tile"


def trunk_path(rows, T, small_m=SMALL_M, tail_ntb=0, slices=1):
    """The style-aware kernels of one launch sequence (run_trunk_style): the small path's GEMM tile height and whether its LayerNorms
    are fused (lnf) or run by k_ln_rows_style (ln); or the fused path's attention instantiation and tail height (`slices`: the launch
    sequences that share the chip)."""
    p = plan_trunk(knobs(small_m=small_m, tail_ntb=tail_ntb), rows, T, slices)
    path = PATHS[p["path"]]
    assert path != "small-ring", "several styles: clips of 16 frames or fewer are refused"
    if path == "small-rows-ln":
        return "small-ntb1-lnf"
    if path == "small-rows":
        return f"small-ntb{rows_ntb(rows * (T + 1))}-ln"
    return f"fused-nt{p['nt16']}-tail{p['tail_ntb']}"


def slices(B, T, cfg, streams=0, small_m=SMALL_M, trunk=False, precise=False):
    """The slices a loop over B clips runs as: [(first clip, clips)]."""
    k = knobs(nsplit=streams, small_m=small_m, trunk_groups=trunk, precise=precise)
    return slices_of(B, plan_slices(k, B, cfg, T))


def loop_slices(rows, T, small_m=SMALL_M):
    """Slice count of a loop whose batch is `rows` transformer rows (no MST_STREAMS, no resident trunk)."""
    return plan_slices(knobs(small_m=small_m), rows, False, T)
