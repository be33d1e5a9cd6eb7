"""The sampling path per token, per feature row and per clip, at every feature width's projection kernels and every tile plan of the trunk.

Every other parity test pools a whole tensor into one relative L2 against 1e-3, which dilutes an error confined to a tile edge (one
token of a (64, 263, 1, 196) tensor scaled by 1.01 moves the pooled figure from 4.0e-4 to 4.09e-4).  Here every case is compared with
the oracle through tests/token_profile.py: each token and each feature row against the oracle's own f16-operand rounding model on the
same inputs, each clip against the suite's bar.  The cases and what each launches come from tests/token_cases.py and
tests/plan_mirror.py; test_the_cases_reach_every_instantiation (CPU) holds the lists to the kernels the launchers switch over.

The factors (tests/token_profile.py: C_TOK, C_ROW): 1.5 x the worst kernel / model ratio (with the median floor) measured on an MI355X
over ALL cases below -- the half covers other seeds and weights -- and no more than 3 (tokens) and 6 (rows): above those a bar no longer
separates a 0.3 % local error from rounding.  Worst ratios per group (tokens | rows | worst clip error), 90 cases and 404
comparisons, 36 s in all:

    widths, forward          1.05 (97 x 70)       | 1.23 (289 x 70) | 4.6e-4
    widths, guided           1.01 (97 x 70)       | 1.38 (320 x 68) | 7.3e-4
    widths, DDPM loop        1.07 (129 x 70)      | 1.16 (192 x 68) | 4.4e-4
    widths, DDIM loop        1.08 (97 x 70)       | 1.12 (481 x 70) | 4.3e-4
    widths, guided DDPM loop 1.06 (97 x 70)       | 1.13 (353 x 70) | 6.6e-4
    widths, guided DDIM loop 1.08 (97 x 70)       | 1.09 (161 x 68) | 6.6e-4
    precise, forward         0.11                 | 0.25            | 4.8e-5
    precise, guided          0.16                 | 0.33            | 1.3e-4
    large tiles, forward     1.00 (ntb 2, 3 x 196) | 1.04            | 4.9e-4
    large tiles, guided      0.93                 | 1.01            | 7.9e-4 (3 x 15)
    small paths, forward     1.00                 | 1.14 (3 x 60)   | 5.0e-4
    small paths, guided      0.93                 | 1.07            | 7.0e-4
    batch 64, two clips      0.96 forward, 0.90 guided | 1.01, 0.96      (tests/test_gpu_parity.py, all four tile paths)

The kernels sit AT the model, token by token: the projections' split activations buy nothing visible against the f16 weights.
"""
import numpy as np
import pytest
import torch

import plan_mirror as pm
import token_cases as tc
import token_profile as tp

from token_profile import C_ROW, C_TOK


def dev():
    return torch.device("cuda:0")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def make(F, T, rows):
    import mst_amd  # noqa: F401
    from mst_amd.engine import DenoiserEngine
    eng = DenoiserEngine(F, T, rows, device=dev())
    w, pe = tc.weights(F)
    eng.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, pe=torch.from_numpy(pe))
    return eng


def report(what, kernels, got, ref, model, ntb=4, clip_bar=tp.CLIP_BAR):
    """Print the figures first, then assert them."""
    r = tp._bft(ref)
    tok = float(tp.token_ratios(got, ref, model).max()) if r.shape[1] >= tp.TOKEN_MIN_FEATS else float("nan")
    row = float(tp.row_ratios(got, ref, model).max()) if r.shape[0] * r.shape[2] >= tp.ROW_MIN_SAMPLES else float("nan")
    print(f"PROFILE {what}: {' + '.join(kernels)}: clip {tp.clip_errors(got, ref).max():.3e} (model {tp.clip_errors(model, ref).max():.3e}), "
          f"token ratio {tok:.2f}, row ratio {row:.2f}")
    tp.assert_profiles(got, ref, model, C_TOK, C_ROW, ntb, what, clip_bar)


def run_forwards(eng, F, T, B, kernels, what, ntb=4, clip_bars=(tp.CLIP_BAR, tp.CLIP_BAR)):
    i = tc.forward_inputs(F, T, B)
    eng.set_text(cu(i["txt"]))
    got = eng.forward(cu(i["x"]), cu(i["t"])).cpu().numpy()
    report(f"{what} forward", kernels["forward"][:2], got, *tc.oracle_forward(F, T, B, False), ntb, clip_bars[0])
    eng.set_text(cu(i["txt"]), cfg=True)
    got = eng.forward(cu(i["x"]), cu(i["t"]), scale=cu(i["scale"]), cfg=True).cpu().numpy()
    report(f"{what} guided", kernels["guided"][:2], got, *tc.oracle_forward(F, T, B, True), ntb, clip_bars[1])


@pytest.mark.gpu
@pytest.mark.parametrize("F,T", tc.width_cases(), ids=lambda v: str(v))
def test_every_width_per_token_row_and_clip(F, T):
    """One forward, one guided forward with per-clip scales and a 2-step DDPM and DDIM (eta = 0.3) loop with recorded noise, a mask
    that is not the root pattern and the x0-hat dump -- the second step runs behind the first step's frame-row or fused-embedding
    hand-off -- on two clips whose boundary lies inside the third, partial 64-frame tile.  Both loops run plain and under
    classifier-free guidance with the same per-clip scales (k_embed_out<NBW, 1 | 2, 2> up to 384 features, the ring beyond)."""
    from mst_amd.engine import Schedule, SAMPLER_DDPM, SAMPLER_DDIM
    from oracle import schedule
    B = tc.WIDTH_CLIPS
    kernels = tc.width_kernels(F, T)
    eng = make(F, T, 2 * B)
    ntb = pm.plan_trunk(pm.knobs(), B, T)["tail_ntb"]
    run_forwards(eng, F, T, B, kernels, f"width {F} x {T}", ntb)
    i = tc.loop_inputs(F, T, B)
    scale = cu(tc.forward_inputs(F, T, B)["scale"])
    tab, tmap = schedule.make("cosine", 1000, "ddim20")
    sch = Schedule(tab, tmap, dev())
    m = i["mask"].astype(bool)
    for guided in (False, True):
        eng.set_text(cu(i["txt"]), cfg=guided)
        ntb = pm.plan_trunk(pm.knobs(), 2 * B if guided else B, T)["tail_ntb"]
        for (name, mode, eta), sampler in zip(tc.LOOPS, (SAMPLER_DDPM, SAMPLER_DDIM)):
            x1 = sch.q_sample(cu(i["motion"]), cu(np.full(B, 1)), cu(i["nz"][0]), cu(i["mask"]))
            got, dump = eng.sample_loop(sch, x1, 1, 0, sampler, eta, cfg=guided, scale=scale if guided else None, mask=cu(i["mask"]),
                                        motion=cu(i["motion"]), noise=cu(i["nz"][1:]), dump_xstart=True)
            dump, got = dump.cpu().numpy(), got.cpu().numpy()
            call = name + " guided" if guided else name
            report(f"width {F} x {T} {call} loop", kernels[call], dump, *tc.oracle_loop(F, T, B, name, eta, guided), ntb)
            for step in range(2):
                assert np.array_equal(dump[step][m], i["motion"][m]), (call, step)        # masked entries bit-exact
            assert np.array_equal(got[m], i["motion"][m]), call


@pytest.mark.gpu
@pytest.mark.parametrize("F,T", tc.precise_cases(), ids=lambda v: str(v))
def test_precise_mode_ring_projections_per_token_row_and_clip(F, T):
    """Precise mode runs both projections on the slab ring with split weights: launch_out_nx<0, 256 | 384 | 512, ..>, XS = 2 up to
    384 rows.  Per clip against test_precise_mode_forward_cfg_and_loop's bars (1e-4 forward, 2e-4 guided); per token and per row
    against the same model as everywhere, which these kernels undercut by far -- a wrong tile edge still does not."""
    B = tc.WIDTH_CLIPS
    eng = make(F, T, 2 * B)
    eng.set_precise(True)
    run_forwards(eng, F, T, B, tc.width_kernels(F, T, precise=True), f"precise {F} x {T}", clip_bars=(1e-4, 2e-4))


@pytest.mark.gpu
@pytest.mark.parametrize("ntb,T", tc.trunk_cases(), ids=lambda v: str(v))
def test_large_tiles_at_every_tail_height_per_token_row_and_clip(ntb, T, monkeypatch):
    """Three clips on the large-tile path (MST_SMALL_M=0) with the fused tail's tile height forced to 32, 48 and 64 tokens."""
    monkeypatch.setenv("MST_SMALL_M", "0")
    monkeypatch.setenv("MST_TAIL_NTB", str(ntb))
    B, F = tc.TRUNK_CLIPS, tc.FEATS
    kernels = {c: (f"{path} ({detail})", pm.embed_out_kernel(F, T, c == "guided"))
               for c, (path, detail, _) in tc.trunk_kernels(B, T, small_m=0, tail_ntb=ntb).items()}
    run_forwards(make(F, T, 2 * B), F, T, B, kernels, f"large tiles, tail_ntb {ntb}, 3 x {T}", ntb)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", tc.SMALL_SHAPES, ids=lambda v: str(v))
def test_small_paths_per_token_row_and_clip(B, T):
    """The small paths at their defaults: rows-GEMM tile heights 1 (LayerNorm inside the GEMM), 4 and 2, and the split-operand ring."""
    F = tc.FEATS
    plans = tc.trunk_kernels(B, T)
    kernels = {c: (f"{path} ({detail})", pm.embed_out_kernel(F, T, c == "guided")) for c, (path, detail, _) in plans.items()}
    run_forwards(make(F, T, 2 * B), F, T, B, kernels, f"small path {B} x {T}", plans["guided"][2]["tail_ntb"])


def test_the_cases_reach_every_instantiation():
    """The case lists against what the launchers of mst_engine.hip switch over (through the mirror of csrc/mst_plan.h, which
    tests/test_launch_plan_cpu.py ties to the header)."""
    ins, outs, fused, rings = set(), set(), set(), set()
    for F, T in tc.width_cases():
        ins.add(pm.plan_embed_in(F)["ks"])
        # what test_every_width_per_token_row_and_clip runs: forward, guided forward, and both loops plain and guided
        for cfg, mode in ((0, 0), (1, 0), (0, 1), (0, 2), (1, 1), (1, 2)):
            p = pm.plan_embed_out(F, T, cfg, mode=mode)
            if pm.EMBED_KERNELS[p["kernel"]] == "latency":
                outs.add((p["nbw"], mode, p["nx"], p["staged"]))
                if p["ksn"]:
                    fused.add((p["nbw"], mode, p["ksn"]))
            else:
                rings.add((mode, p["ring_bf"], p["nx"], p["ring_xs"]))
    assert ins == set(range(3, 17))                                             # every k_embed_in<KS>
    # every k_embed_out<NBW, MODE, NX> launch_embed_out can select: NX 1 at every NBW, NX 2 (guidance) up to NBW 3; a forward
    # (mode 0) has one epilogue, a loop step (modes 1, 2) the staged one at T % 4 == 0 up to NBW 3 and finish otherwise
    assert outs == ({(nbw, 0, nx, 0) for nbw in (1, 2, 3, 4) for nx in (1, 2) if (nbw, nx) != (4, 2)}
                    | {(nbw, mode, nx, st) for nbw in (1, 2, 3, 4) for mode in (1, 2) for nx in (1, 2) for st in (0, 1)
                       if (nbw, st) != (4, 1) and (nbw, nx) != (4, 2)})
    # the three fused kernels k_embed_out<2, MODE, 1, 5>, <2, MODE, 1, 6>, <3, MODE, 1, 9>, for both samplers
    assert fused == {(2, m, 5) for m in (1, 2)} | {(2, m, 6) for m in (1, 2)} | {(3, m, 9) for m in (1, 2)}
    # the NBW == 4 guidance fallback, launch_out_nx<MODE, 512, ..> with NX 2: the forward and both samplers' steps
    assert rings == {(mode, 512, 2, 1) for mode in (0, 1, 2)}
    # NBW == 1 at a full 128 features
    assert (128, 68) in tc.width_cases() and pm.plan_embed_out(128, 68)["nbw"] == 1 and pm.plan_embed_out(129, 68)["nbw"] == 2
    # precise mode: the ring at every width, with and without guidance, and the ring pose embedding
    prec = {(p["ring_bf"], p["nx"], p["ring_xs"]) for F, T in tc.precise_cases() for cfg in (0, 1)
            for p in [pm.plan_embed_out(F, T, cfg, precise=True)] if pm.EMBED_KERNELS[p["kernel"]] == "ring"}
    assert prec == {(256, 1, 2), (256, 2, 2), (384, 1, 2), (384, 2, 2), (512, 1, 1), (512, 2, 1)}
    assert all(pm.EMBED_KERNELS[pm.plan_embed_in(F, precise=True)["kernel"]] == "ring" for F, _ in tc.precise_cases())
    # the trunk: every path except the resident one; the fused tail at 2, 3 and 4 blocks of 16 tokens; k_qkv_attention2<NT16> from
    # its lowest to its highest instantiation, and the ring kernel behind it (S = 224); the rows GEMMs at 1, 2 and 4 blocks a tile
    paths, tails, nt16, qkv, rows_ntb = set(), set(), set(), set(), set()
    for ntb, T in tc.trunk_cases():
        for path, _, p in tc.trunk_kernels(tc.TRUNK_CLIPS, T, small_m=0, tail_ntb=ntb).values():
            assert path == "large"
            paths.add(path), tails.add(p["tail_ntb"]), qkv.add(pm.QKV_ATTN[p["qkv_attn"]]), nt16.add(p["nt16"])
    for B, T in tc.SMALL_SHAPES:
        path, _, p = tc.trunk_kernels(B, T)["forward"]
        paths.add(path)
        if path.startswith("small-rows"):
            rows_ntb.add(1 if path == "small-rows-ln" else pm.rows_ntb(B * (T + 1)))
    assert paths == {"small-ring", "small-rows", "small-rows-ln", "large"}
    assert tails == {2, 3, 4} and rows_ntb == {1, 2, 4} and qkv == {"streamed", "ring"}
    assert nt16 == {2, 8, 12, 13, 14}                   # 16-token blocks of a clip: the lowest, the odd one (13) and the highest
