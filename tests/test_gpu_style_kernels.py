"""Every style-aware kernel of csrc/mst_style.h against the per-style fp32 oracle, at the shapes its launch rules tell apart.

test_gpu_style_bank.py checks isolation bitwise (a mixed batch against the same batch with one style), which both sides of a shared
mistake pass.  Here every style's clips of a mixed batch are compared with oracle.denoiser run with that style's own weights:

  1. fused path, every k_qkv_attention2_style<NT16> (NT16 = 2, 4, 6, 8, 10, 12, 13), clip counts off and on multiples of 8;
  2. k_layer_tail_seg<2/3/4> on 18-token clips, where one 48- or 64-row tile holds 3-4 segments updated in place;
  3. the default tail-height rule picking 48-row tiles (HumanML, 48 clips);
  4. the small path: k_rows_gemm_seg at NTB 1 (LayerNorm fused and not), 4 and 2, k_ln_rows_style;
  5. classifier-free guidance per style, also where the doubled batch changes the path;
  6. sampling loops split into 3 slices (one plan per slice), DDPM with inpainting and a guided DDIM loop;
  7. bitwise invariants: the XCD-affine order equals the plain one; growing 3 -> 8 slots leaves slots 0-2 unchanged.

Each case id names the path it forces, computed by the mirror of the engine's launch plan (trunk_path, loop_slices of tests/plan_mirror.py)."""
import zlib

import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
from conftest import rel_l2
import style_fixture as sf
from plan_mirror import loop_slices, slices_of, trunk_path
from style_fixture import cu

pytestmark = pytest.mark.gpu

TOL = 1e-3                              # tests/test_gpu_style_bank.py, per style subset
K = 3
F_XIA, T_XIA = 181, 76
F_HML, T_HML = 263, 196

def pattern(name, B, k=K):
    if name == "cycle":                  # no two neighbouring clips share a style: a tile holds as many segments as clips it touches
        return [i % k for i in range(B)]
    if name == "odd":                    # one clip of another style inside a run of one style
        st = [1] * B
        st[B // 2] = 2
        return st
    raise ValueError(name)


def max_segments_per_tile(styles, T, tile_rows):
    from mst_amd.engine import plan_style_segments
    seg = plan_style_segments(styles, T + 1, tile_rows)
    return int(np.unique(seg[:, 0], return_counts=True)[1].max())


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def inputs(F, T, B, name):
    r = _rng(f"sk/{name}/{F}/{T}/{B}")
    x = r.standard_normal((B, F, 1, T), dtype=np.float32)
    t = np.array([(37 * i + 5) % 1000 for i in range(B)], np.int64)
    txt = r.standard_normal((B, 512), dtype=np.float32)
    scale = np.linspace(1.5, 3.0, B, dtype=np.float32)     # per-clip guidance scales (CFG_SCALE_MAX = 3.0)
    return x, t, txt, scale


def engine(monkeypatch, F, T, max_rows, slots=K, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    return sf.make_engine(F, T, max_rows, slots)


def forward(eng, styles, x, t, txt, scale=None):
    cfg = scale is not None
    eng.set_text(cu(txt), cfg=cfg)
    eng.set_styles(styles)
    out = eng.forward(cu(x), cu(t), scale=cu(scale) if cfg else None, cfg=cfg)
    torch.cuda.synchronize()
    return out


_REF = {}


def oracle_errors(out, styles, F, x, t, txt, scale=None, key=None):
    """rel-L2 of every style's clips against that style's oracle; the oracle's result is kept under `key` when one is given."""
    torch.set_num_threads(16)
    out = out.cpu().numpy() if isinstance(out, torch.Tensor) else out
    errs = {}
    for s in sorted(set(styles)):
        rows = [i for i, v in enumerate(styles) if v == s]
        k = None if key is None else (key, s)
        if k is None or k not in _REF:
            ref = np.asarray(sf.oracle_forward(F, s, x[rows], t[rows], txt[rows], None if scale is None else scale[rows]))
            if k is not None:
                _REF[k] = ref
        errs[s] = rel_l2(out[rows], _REF[k] if k is not None else ref)
    return errs


def report(request, errs):
    worst = max(errs, key=errs.get)
    print(f"\n{request.node.name}: worst style {worst} rel-L2 {errs[worst]:.2e} "
          f"({', '.join(f'{s}: {e:.1e}' for s, e in sorted(errs.items()))})")
    assert max(errs.values()) < TOL, errs


# ------------------------------------------------------------------------------ 1. fused path, every attention instantiation
ATTN = [(17, 13, "cycle"), (17, 13, "odd"), (40, 20, "cycle"), (76, 16, "cycle"), (100, 11, "cycle"), (150, 8, "cycle"),
        (180, 9, "cycle"), (207, 10, "cycle"), (207, 10, "odd")]


@pytest.mark.parametrize("T,B,pat", ATTN, ids=[f"T{T}-B{B}-{p}-{trunk_path(B, T, small_m=0)}" for T, B, p in ATTN])
def test_fused_attention_every_tile_count(request, monkeypatch, T, B, pat):
    eng = engine(monkeypatch, F_HML, T, B, MST_SMALL_M=0)
    st = pattern(pat, B)
    x, t, txt, _ = inputs(F_HML, T, B, "attn")
    out = forward(eng, st, x, t, txt)
    report(request, oracle_errors(out, st, F_HML, x, t, txt))


# ------------------------------------------------------------------------------ 2. every tail height, 3-4 segments in one tile
TAIL = [(ntb, p) for ntb in (2, 3, 4) for p in ("cycle", "odd")]


@pytest.mark.parametrize("ntb,pat", TAIL, ids=[f"T17-B24-{p}-{trunk_path(24, 17, small_m=0, tail_ntb=n)}" for n, p in TAIL])
def test_tail_height_short_clips(request, monkeypatch, ntb, pat):
    T, B = 17, 24                                     # 24 x 18 = 432 rows: the small path unless MST_SMALL_M=0
    eng = engine(monkeypatch, F_HML, T, B, MST_SMALL_M=0, MST_TAIL_NTB=ntb)
    st = pattern(pat, B)
    if pat == "cycle":
        assert max_segments_per_tile(st, T, 16 * ntb) >= 3                             # several workgroups update one tile
    x, t, txt, _ = inputs(F_HML, T, B, "tail")
    mixed = forward(eng, st, x, t, txt)
    report(request, oracle_errors(mixed, st, F_HML, x, t, txt, key=("tail", pat)))
    for s in sorted(set(st)):
        rows = [i for i, v in enumerate(st) if v == s]
        assert torch.equal(mixed[rows], forward(eng, [s] * B, x, t, txt)[rows]), s


# ------------------------------------------------------------------------------ 3. the default rule at 48-row tail tiles
@pytest.mark.parametrize("case", [f"T{T_HML}-B48-cycle-{trunk_path(48, T_HML)}"])
def test_default_tail_rule_48_row_tiles(request, monkeypatch, case):
    B = 48                                            # 9456 rows: 296 tiles of 32 rows > 256, 197 of 48 rows
    assert trunk_path(B, T_HML) == "fused-nt13-tail3"
    eng = engine(monkeypatch, F_HML, T_HML, B)
    st = pattern("cycle", B)
    x, t, txt, _ = inputs(F_HML, T_HML, B, "hml48")
    report(request, oracle_errors(forward(eng, st, x, t, txt), st, F_HML, x, t, txt))


# ------------------------------------------------------------------------------ 4. small path, every GEMM tile height
SMALL = [(F_XIA, T_XIA, 4, "cycle"), (F_XIA, T_XIA, 8, "cycle"), (F_XIA, T_XIA, 12, "cycle"), (F_XIA, T_XIA, 20, "cycle"),
         (F_HML, 17, 56, "cycle"), (F_HML, 17, 56, "odd")]


@pytest.mark.parametrize("F,T,B,pat", SMALL, ids=[f"T{T}-B{B}-{p}-{trunk_path(B, T)}" for F, T, B, p in SMALL])
def test_small_path_every_gemm_height(request, monkeypatch, F, T, B, pat):
    assert trunk_path(B, T).startswith("small")
    eng = engine(monkeypatch, F, T, B)
    st = pattern(pat, B)
    if T == 17 and pat == "cycle":
        assert max_segments_per_tile(st, T, 64) >= 3                                   # 64-row tiles touching 4-5 clips
    x, t, txt, _ = inputs(F, T, B, "small")
    report(request, oracle_errors(forward(eng, st, x, t, txt), st, F, x, t, txt))


# ------------------------------------------------------------------------------ 5. classifier-free guidance per style
CFG = [(F_XIA, T_XIA, 6), (F_HML, T_HML, 10), (F_XIA, T_XIA, 16)]   # the last: 16 clips alone are small, doubled fused


@pytest.mark.parametrize("F,T,B", CFG, ids=[f"T{T}-B{B}-cfg-{trunk_path(2 * B, T)}-plain-{trunk_path(B, T)}" for F, T, B in CFG])
def test_guided_forward_per_style(request, monkeypatch, F, T, B):
    eng = engine(monkeypatch, F, T, 2 * B)
    st = pattern("cycle", B)
    x, t, txt, scale = inputs(F, T, B, "cfg")
    report(request, oracle_errors(forward(eng, st, x, t, txt, scale), st, F, x, t, txt, scale))


# ------------------------------------------------------------------------------ 6. loops split into slices
def inpaint_mask(B, F, T):
    """Not the root pattern: whole feature rows (3 per clip, one of them varying with the clip) and a strided set of frames of ten
    more features."""
    m = np.zeros((B, F, 1, T), np.float32)
    for b in range(B):
        m[b, [5, 6, 7 + b % 5]] = 1
        m[b, 20:30, :, ::3] = 1
    return m


LOOPS = [(F_XIA, T_XIA, 24, "ddpm", False), (F_HML, T_HML, 64, "ddpm", False), (F_XIA, T_XIA, 12, "ddim", True)]


def _loop_id(F, T, B, sampler, cfg):
    rows = 2 * B if cfg else B
    n = loop_slices(rows, T)
    paths = {trunk_path(2 * nb if cfg else nb, T, slices=n) for _, nb in slices_of(B, n)}
    return f"T{T}-B{B}-{sampler}{'-cfg' if cfg else ''}-{n}slices-{'+'.join(sorted(paths))}"


@pytest.mark.parametrize("F,T,B,sampler,cfg", LOOPS, ids=[_loop_id(*c) for c in LOOPS])
def test_sliced_loop_vs_oracle_loop(request, monkeypatch, F, T, B, sampler, cfg):
    """10 steps (indices 9..0) with recorded noise and inpainting; one clip per style in every slice against the oracle's loop."""
    from mst_amd.engine import SAMPLER_DDIM, SAMPLER_DDPM
    from oracle import diffusion, schedule
    n, eta = 10, 0.3 if sampler == "ddim" else 0.0
    nsl = loop_slices(2 * B if cfg else B, T)
    assert nsl == 3
    eng = engine(monkeypatch, F, T, 2 * B if cfg else B)
    assert eng.loop_slices(B, cfg, T) == nsl
    st = pattern("cycle", B)
    _, _, txt, scale = inputs(F, T, B, "loop")
    r = _rng(f"sk/loop/{F}/{B}")
    motion = r.standard_normal((B, F, 1, T), dtype=np.float32)
    nz = r.standard_normal((n + 1, B, F, 1, T), dtype=np.float32)
    mask = inpaint_mask(B, F, T)
    sch = sf.schedule()
    eng.set_text(cu(txt), cfg=cfg)
    eng.set_styles(st)
    x9 = sch.q_sample(cu(motion), cu(np.full(B, n - 1)), cu(nz[0]), cu(mask))
    out = eng.sample_loop(sch, x9, n - 1, 0, SAMPLER_DDIM if sampler == "ddim" else SAMPLER_DDPM, eta=eta, cfg=cfg,
                          scale=cu(scale) if cfg else None, mask=cu(mask), motion=cu(motion), noise=cu(nz[1:])).cpu().numpy()
    assert np.array_equal(out[mask == 1], motion[mask == 1])                  # masked entries bit for bit
    tab, tmap = schedule.make("cosine", 1000, "")
    torch.set_num_threads(16)
    errs = {}
    for s in range(K):
        sel = [next(c for c in range(c0, c0 + nb) if st[c] == s) for c0, nb in slices_of(B, nsl)]
        ref = diffusion.sample_loop(
            lambda xx, tt: sf.oracle_forward(F, s, xx, tt, txt[sel], scale[sel] if cfg else None), tab, tmap, (len(sel), F, 1, T),
            lambda k: torch.from_numpy(nz[k][sel]), sampler, True, mask[sel], motion[sel], init_image=motion[sel],
            skip_timesteps=1000 - n, eta=eta).numpy()
        for j, c in enumerate(sel):
            errs[(s, c)] = rel_l2(out[c], ref[j])
    report(request, errs)


# ------------------------------------------------------------------------------ 7. bitwise invariants
XCD_ID = f"fwd-T{T_HML}-B16-{trunk_path(16, T_HML)}-loop-T{T_XIA}-B24-{loop_slices(24, T_XIA)}slices-{trunk_path(8, T_XIA, slices=3)}"


@pytest.mark.parametrize("case", [XCD_ID])
def test_xcd_order_equals_plain_order(monkeypatch, case):
    """MST_STYLE_XCD=0 (clips and segments in plain order) against the default XCD-affine order: a fused forward and a sliced
    small-path loop."""
    from mst_amd.engine import SAMPLER_DDPM
    res = {}
    for xcd in ("1", "0"):
        monkeypatch.setenv("MST_STYLE_XCD", xcd)
        B = 16
        eng = sf.make_engine(F_HML, T_HML, B, K)
        x, t, txt, _ = inputs(F_HML, T_HML, B, "xcd")
        fwd = forward(eng, pattern("cycle", B), x, t, txt)
        B = 24
        eng = sf.make_engine(F_XIA, T_XIA, B, K)
        assert eng.loop_slices(B, False, T_XIA) == 3
        x, t, txt, _ = inputs(F_XIA, T_XIA, B, "xcd")
        eng.set_text(cu(txt))
        eng.set_styles(pattern("cycle", B))
        loop = eng.sample_loop(sf.schedule(), cu(x), 9, 0, SAMPLER_DDPM, seed=77)
        torch.cuda.synchronize()
        res[xcd] = (fwd, loop)
    assert torch.equal(res["1"][0], res["0"][0])
    assert torch.equal(res["1"][1], res["0"][1])


@pytest.mark.parametrize("case", [f"K8-slot7-T{T_XIA}-B16-{trunk_path(16, T_XIA, small_m=0)}"])
def test_grow_to_eight_slots(request, monkeypatch, case):
    """3 slots loaded and used, then 8: slots 0-2 give the same bits, and a batch over all 8 (slot 7 included) meets the oracle."""
    B, T = 16, T_XIA
    eng = engine(monkeypatch, F_XIA, T, B, MST_SMALL_M=0)
    x, t, txt, _ = inputs(F_XIA, T, B, "grow")
    st3 = pattern("cycle", B)
    before = forward(eng, st3, x, t, txt)
    eng.style_slots(8)
    assert torch.equal(forward(eng, st3, x, t, txt), before)                  # slots 1-2 are still loaded after the growth
    for s in range(K, 8):
        eng.load_layers_slot(s, sf.layer_list(sf.style_weights(F_XIA, s)))
    assert torch.equal(forward(eng, st3, x, t, txt), before)
    st8 = pattern("cycle", B, k=8)
    report(request, oracle_errors(forward(eng, st8, x, t, txt), st8, F_XIA, x, t, txt))
