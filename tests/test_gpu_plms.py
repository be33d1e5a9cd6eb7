"""The PLMS sampler on the GPU (reference gaussian_diffusion.py:1084-1279): the multistep step at every site that applies the diffusion
update (MODE 4 of the fused kernels, k_plms_epilogue stand-alone), the two-evaluation step that opens a chain, and the loops.

  1. the stand-alone kernels against the float64 closed form (tests/plms_fixture.py): every index, cur_order 1..4, every MEAN, blend, clamp;
  2. fused single steps and the Euler step against the reference's own outputs (tests/golden/plms.npz), small- and large-tile paths;
  3. a five-step order-4 chain (the Euler step, then cur_order 2, 3, 4, 4) on every fused path -- rows as tests/test_gpu_reverse.py's
     TRAJ, each asserting from mirrors of the launch rules which path it takes --
       (a) every x_{k+1} and every ring slot recomputed in float64 from the engine's OWN x0-hat, inputs and history;
       (b) every x0-hat against the fp32 oracle forward at that step's input (the Euler step: both evaluations);
       (c) two runs, (d) one five-step call == five one-step calls with steps_done carried, (e) noise arguments change nothing: bit for bit;
  4. bitwise properties: slicing, neighbours, the mirror's loop entries, graph replay at every order;
  5. whole 20-step loops against the reference's, relative to this engine's own DDIM error against the reference's DDIM;
  6. refusals, each naming its reason;
  7. invert once, decode with PLMS under three styles as one batch.

The bars.  (a) is elementwise, 2e-5 (tests/test_gpu_parity.py's stand-alone-step constant) of `scale`, the summed magnitudes of the
products the value is built from (plms_fixture); tests/test_plms_cpu.py holds the reference's own goldens to the same bar, and they sit
at 1.8e-7.  (b) is the project's forward bar, 1e-3 relative L2.  The second evaluation of the Euler step is not dumped by the engine: it
is recovered from x_1, which is linear in it (plms_fixture.euler_gain), around the oracle's own second output."""
import ctypes as C

import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
import mst_amd.synthetic as syn
import plms_fixture as pf
from conftest import SEED, rel_l2
from oracle import denoiser
from plan_mirror import SMALL_M, plain_path, slices
from test_gpu_noise import FAMILIES, TRUNK_FAMILIES, draw_site, mask_of
from test_gpu_reverse import (EMB, PE, RSCA, SCA, TOL, VEC, _model, _step_inputs, _xstart64, cu, dev, embeds_next, make, sched, weights,
                              within)

pytestmark = pytest.mark.gpu
BAR_STEP = pf.BAR_STEP


def nan_ring(shp):
    """A ring nobody has written: a slot that is read before its step wrote it poisons x."""
    return torch.full((3,) + tuple(shp), float("nan"), device=dev())


def eps_scale(tab, pred, x, t):
    """(srac |x| + |pred|) / srm1ac: the magnitudes of the two products eps is built from."""
    srac, srm1, _ = pf._entries(tab, t, x)
    return (srac * np.abs(x) + np.abs(pred)) / srm1


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ------------------------------------------------------------------------------ 1. the stand-alone kernels
STEP_T = {"ddim20": [list(range(0, 7)), list(range(7, 14)), list(range(14, 20)) + [19]], "": [[0, 1, 500, 999, 999, 1, 0]]}


def _history(shp):
    return [syn.normal(SEED, f"ps/h{k}", shp) for k in (1, 2, 3)]          # newest first


@pytest.mark.parametrize("mean", [0, 1, 2], ids=["x_start", "epsilon", "previous_x"])
@pytest.mark.parametrize("resp", ["ddim20", ""], ids=["ddim20-every-index", "full-0-1-500-999"])
def test_standalone_step_equals_the_float64_closed_form(resp, mean):
    """Schedule.plms_step: a different index per clip (7 clips a call: every index of ddim20; 0, 1, 500, 999 of the full schedule),
    cur_order 1..4, blend on / off, clamp on / off.  x0-hat against the float64 front end, sample and eps against the closed form applied
    to the KERNEL's x0-hat; at index 0 the sample is x0-hat bit for bit; under a mask the masked x0-hat is the motion bit for bit."""
    sch, tab, _ = sched(resp)
    B, F, T = 7, 24, 10                                           # 240 elements a clip: one partly filled block (several blocks: below)
    v = _step_inputs(B, F, T)
    hist = _history((B, F, 1, T))
    worst = worst_e = 0.0
    for ts in STEP_T[resp]:
        t = np.asarray(ts)
        for blend in (False, True):
            for clamp in (False, True):
                mk, mot = (v["mask"], v["motion"]) if blend else (None, None)
                kw = dict(mask=None if mk is None else cu(mk), motion=None if mot is None else cu(mot), clip_denoised=clamp, mean_type=mean)
                p64 = _xstart64(tab, mean, v["mo"], v["x"], t, mk, mot, clamp)
                for c in (1, 2, 3, 4):
                    old = [cu(h) for h in hist[:c - 1]][::-1]      # oldest first, as old_eps holds them
                    s, p, e = (a.cpu().numpy() for a in sch.plms_step(cu(v["mo"]), cu(v["x"]), cu(t), history=old, order=c, **kw))
                    assert np.isfinite(s).all()
                    if mean == 0:
                        assert np.array_equal(p, p64.astype(np.float32))            # blend and clamp are exact in fp32
                    elif not clamp:
                        f = lambda name: pf._bc(pf._f32(np.asarray(tab[name])[t]), v["x"])
                        raw = np.abs(_xstart64(tab, 0, v["mo"], v["x"], t, mk, mot, False))
                        mag = (np.abs(f("sqrt_recip_alphas_cumprod") * v["x"]) + f("sqrt_recipm1_alphas_cumprod") * raw if mean == 1 else
                               (raw + np.abs(f("posterior_mean_coef2") * v["x"])) / f("posterior_mean_coef1"))
                        within(p, p64, mag, f"x0-hat mean {mean} t {ts}")
                    if clamp:
                        assert np.abs(p).max() <= 1.0
                    if blend and mean == 0 and not clamp:
                        m = v["mask"].astype(bool)
                        assert np.array_equal(p[m], v["motion"][m])
                    want, scale, eps = pf.closed_form(tab, p, v["x"], t, hist[:c - 1])
                    what = f"mean {mean} t {ts} blend {blend} clamp {clamp} cur_order {c}"
                    worst = max(worst, within(s, want, scale, "sample " + what))
                    worst_e = max(worst_e, within(e, eps, eps_scale(tab, p, v["x"], t), "eps " + what))
                    zero = t == 0
                    if zero.any():
                        assert np.array_equal(s[zero], p[zero]), "at index 0 the sample is x0-hat, bit for bit"
    print(f"\nstand-alone PLMS step '{resp}' mean {mean}: worst |kernel - closed form| / scale: sample {worst:.2e}, eps {worst_e:.2e} (bar {BAR_STEP:.0e})")


def test_standalone_step_more_than_one_block_per_clip_and_eps_into_the_oldest_slot():
    """per_clip = 263 * 196 = 51548 elements (202 blocks of 256 threads per clip), three clips at three indices, cur_order 4; then the
    same call with eps written over the oldest history entry, as the ring does at order 4: the same bits."""
    sch, tab, _ = sched("ddim20")
    B, F, T = 3, 263, 196
    v = _step_inputs(B, F, T)
    hist = _history((B, F, 1, T))
    t = np.array([0, 11, 19])
    old = [cu(h) for h in hist][::-1]
    kw = dict(mask=cu(v["mask"]), motion=cu(v["motion"]))
    s, p, e = sch.plms_step(cu(v["mo"]), cu(v["x"]), cu(t), history=old, order=4, **kw)
    want, scale, eps = pf.closed_form(tab, p.cpu().numpy(), v["x"], t, hist)
    r = within(s.cpu().numpy(), want, scale, "sample")
    within(e.cpu().numpy(), eps, eps_scale(tab, p.cpu().numpy(), v["x"], t), "eps")
    assert np.array_equal(p.cpu().numpy(), pf.blend(v["mo"], v["mask"], v["motion"]).astype(np.float32))
    oldest = old[0].clone()
    s2, p2, e2 = sch.plms_step(cu(v["mo"]), cu(v["x"]), cu(t), history=[oldest] + old[1:], order=4, eps_out=oldest, **kw)
    assert e2.data_ptr() == oldest.data_ptr()
    assert torch.equal(s, s2) and torch.equal(p, p2) and torch.equal(e, oldest)
    print(f"\nworst ratio {r:.2e}")


@pytest.mark.parametrize("mean", [0, 1, 2], ids=["x_start", "epsilon", "previous_x"])
def test_standalone_euler_halves_equal_the_closed_form(mean):
    """first_half: x_mid from pred ITSELF, eps out; plms_euler: tables at t - 1 for the second evaluation, at t behind it."""
    sch, tab, _ = sched("ddim20")
    B, F, T = 7, 24, 10
    v = _step_inputs(B, F, T)
    mo2 = syn.normal(SEED, "ps/mo2", (B, F, 1, T))
    worst = 0.0
    for ts in ([1, 2, 3, 9, 10, 18, 19], [19, 1, 7, 13, 16, 4, 5]):
        t = np.asarray(ts)
        for blend in (False, True):
            for clamp in (False, True):
                mk, mot = (v["mask"], v["motion"]) if blend else (None, None)
                kw = dict(mask=None if mk is None else cu(mk), motion=None if mot is None else cu(mot), clip_denoised=clamp, mean_type=mean)
                xm, p, e = (a.cpu().numpy() for a in sch.plms_step(cu(v["mo"]), cu(v["x"]), cu(t), first_half=True, **kw))
                want, scale, eps = pf.euler_first(tab, p, v["x"], t)
                worst = max(worst, within(xm, want, scale, f"x_mid t {ts}"))
                within(e, eps, eps_scale(tab, p, v["x"], t), f"eps t {ts}")
                s = sch.plms_euler(cu(mo2), cu(xm), cu(v["x"]), cu(e), cu(t), **kw).cpu().numpy()
                p2 = _xstart64(tab, mean, mo2, xm, t - 1, mk, mot, clamp)      # the second evaluation's x0-hat: tables at t - 1, from x_mid
                want, scale = pf.euler_second(tab, p2, xm, v["x"], e, t)
                if mean != 0:                                                   # (the conversion's own products are part of what is summed)
                    f = lambda name: pf._bc(pf._f32(np.asarray(tab[name])[t - 1]), v["x"])
                    raw = np.abs(_xstart64(tab, 0, mo2, xm, t - 1, mk, mot, False))
                    mag = (np.abs(f("sqrt_recip_alphas_cumprod") * xm) + f("sqrt_recipm1_alphas_cumprod") * raw if mean == 1 else
                           (raw + np.abs(f("posterior_mean_coef2") * xm)) / f("posterior_mean_coef1"))
                    scale = scale + np.abs(pf.euler_gain(tab, t, v["x"])) * mag
                worst = max(worst, within(s, want, scale, f"sample t {ts} blend {blend} clamp {clamp}"))
    print(f"\nstand-alone Euler halves mean {mean}: worst ratio {worst:.2e} (bar {BAR_STEP:.0e})")


# ------------------------------------------------------------------------------ 2. fused steps against the reference
@pytest.mark.parametrize("path", ["small", "large"])
@pytest.mark.parametrize("tag,resp", [("xia", ""), ("xia", "100"), ("xia", "ddim20"), ("hml", "ddim20")],
                         ids=["xia-full", "xia-100", "xia-ddim20", "hml-ddim20"])
def test_fused_single_steps_vs_the_reference(tag, resp, path):
    """One-step native calls late in a chain (steps_done 3, so cur_order = order) over the seeded history, at index 0, an interior index
    and the last index, with and without the pair: x0-hat within 1e-3 of the reference's; sample and the ring slot written from the
    engine's own x0-hat within 2e-5 of scale.  For ddim20 also the Euler step: x0-hat and the recovered second evaluation within 1e-3
    of the reference's two, the ring as the header says."""
    g = pf.golden()
    v = pf.golden_inputs(tag)
    F, T, st = v["F"], v["T"], pf.STRIDE[tag]
    eng = make(F, T, 2, env={"MST_SMALL_M": 0} if path == "large" else None)
    sch, tab, _ = sched(resp)
    eng.set_text(cu(v["txt"]))
    h = v["hist"]
    worst_p = worst_s = 0.0
    for t in pf.INDICES[resp]:
        for pair in (0, 1):
            kw = dict(mask=cu(v["mask"]), motion=cu(v["motion"])) if pair else {}
            for c in (1, 2, 3, 4):
                ring = cu(np.stack([h[2], h[1], h[0]]))            # chain step 3 reads e1 / e2 / e3 from slots 2 / 1 / 0 and writes slot 0
                s, d = eng.sample_loop_plms(sch, cu(v["x"]), t, t, order=c, steps_done=3, hist=ring, dump_xstart=True, **kw)
                s, p, ring = s.cpu().numpy(), d[0].cpu().numpy(), ring.cpu().numpy()
                ep = rel_l2(p[..., ::st], g[f"{tag}|{resp}|{t}|{pair}|pred_xstart"])
                assert ep <= TOL, (t, pair, c, ep)
                want, scale, eps = pf.closed_form(tab, p, v["x"], [t], h[:c - 1])
                worst_s = max(worst_s, within(s, want, scale, f"sample t {t} pair {pair} cur_order {c}"))
                within(ring[0], eps, eps_scale(tab, p, v["x"], [t]), "ring slot 0")
                assert np.array_equal(ring[1], h[1]) and np.array_equal(ring[2], h[0])
                es = rel_l2(s[..., ::st], g[f"{tag}|{resp}|{t}|{pair}|{c}|sample"])
                print(f"\n{tag} '{resp}' {path} t={t} pair={pair} cur_order={c}: x0-hat {ep:.2e} (bar {TOL:.0e}), sample vs the reference's {es:.2e}")
                worst_p = max(worst_p, ep)
                if t == 0:
                    assert np.array_equal(s, p)
                if pair:
                    assert np.array_equal(p[:, :3], v["motion"][:, :3])
    if resp == "ddim20":
        for t in pf.EULER_INDICES:
            for pair in (0, 1):
                kw = dict(mask=cu(v["mask"]), motion=cu(v["motion"])) if pair else {}
                ring = nan_ring(v["x"].shape)
                s, d = eng.sample_loop_plms(sch, cu(v["x"]), t, t, order=2, steps_done=0, hist=ring, dump_xstart=True, **kw)
                s, p, ring = s.cpu().numpy(), d[0].cpu().numpy(), ring.cpu().numpy()
                key = f"{tag}|euler|{t}|{pair}|"
                ep = rel_l2(p[..., ::st], g[key + "pred_xstart"])
                x_mid, _, eps = pf.euler_first(tab, p, v["x"], [t])
                within(ring[0], eps, eps_scale(tab, p, v["x"], [t]), "ring slot 0: eps of the first evaluation")
                assert np.array_equal(ring[1], v["x"]) and np.isnan(ring[2]).all()
                # the second evaluation, recovered from x_1 around the reference's own second output
                sub = lambda a: np.asarray(a)[..., ::st]
                ref2 = g[key + "out2"]
                if pair:
                    ref2 = pf.blend(ref2, sub(v["mask"]), sub(v["motion"])).astype(np.float32)
                want, scale = pf.euler_second(tab, ref2, sub(x_mid), sub(v["x"]), sub(eps), [t])
                p2 = ref2 + (sub(s) - want) / pf.euler_gain(tab, [t], ref2)
                e2 = rel_l2(p2, ref2)
                print(f"\n{tag} {path} euler t={t} pair={pair}: x0-hat {ep:.2e}, second evaluation {e2:.2e} (bar {TOL:.0e}), "
                      f"sample vs the reference's {rel_l2(sub(s), g[key + 'sample']):.2e}")
                assert ep <= TOL and e2 <= TOL, (t, pair, ep, e2)
                if pair:                                            # masked rows: the second x0-hat is the motion, so x_1 is closed there
                    within(sub(s)[:, :3], want[:, :3], scale[:, :3], "x_1 on the masked rows")
    print(f"\n{tag} '{resp}' {path}: worst x0-hat {worst_p:.2e} (bar {TOL:.0e}), worst update {worst_s:.2e} of scale (bar {BAR_STEP:.0e})")


# ------------------------------------------------------------------------------ 3. a five-step order-4 chain on every fused path
def row(id, F, T, B, resp="ddim20", t0=19, cfg=False, mask=None, env=None, expect=None, site=None, nsl=1, ksn=0, **variant):
    return pytest.param(dict(F=F, T=T, B=B, resp=resp, t0=t0, cfg=cfg, mask=mask, env=env or {}, expect=expect, site=site, nsl=nsl, ksn=ksn,
                             **variant), id=id)


# t0: the index the chain STARTS at (it runs down over five indices; t0 = 4 ends at index 0, where the sample is x0-hat).
CHAINS = [
    row("small-launch-T76-B2-root-mask-ksn6", 181, 76, 2, mask="root", expect="small-launch-ln-in-gemm", site=EMB, ksn=6),
    row("small-tile-T76-B9-ksn6-to-index-0", 181, 76, 9, t0=4, expect="small-tile", site=EMB, ksn=6),
    row("fused-large-T76-B2-ksn6-full-schedule", 181, 76, 2, resp="", t0=999, env={"MST_SMALL_M": 0}, expect="fused-large-tile", site=EMB, ksn=6),
    row("fused-large-T196-B2-hml-ksn9-root-mask", 263, 196, 2, mask="root", env={"MST_SMALL_M": 0}, expect="fused-large-tile", site=EMB, ksn=9),
    row("scalar-T75-B3-F190-resp100-to-index-0", 190, 75, 3, resp="100", t0=4, mask="third", expect="small-launch-ln-in-gemm", site=SCA),
    row("scalar-large-T75-B3-F190", 190, 75, 3, env={"MST_SMALL_M": 0}, expect="fused-large-tile", site=SCA),
    row("short-T5-B2-third-mask-hi-lo", 181, 5, 2, mask="third", t0=10, expect="small-tile-hi-lo", site=SCA),
    row("cfg2.5-small-T76-B2", 181, 76, 2, cfg=True, mask="root", expect="small-launch-ln-in-gemm", site=EMB),
    row("cfg2.5-large-T76-B2-to-index-0", 181, 76, 2, cfg=True, t0=4, env={"MST_SMALL_M": 0}, expect="fused-large-tile", site=EMB),
    row("slices-cfg2.5-T76-B12-3x4", 181, 76, 12, cfg=True, env={"MST_STREAMS": 3}, expect="small-tile", site=EMB, nsl=3),
    row("slices-T76-B24-3x8-ksn6-root-mask", 181, 76, 24, mask="root", env={"MST_STREAMS": 3}, expect="small-tile", site=EMB, nsl=3, ksn=6),
    row("styles-3slots-T76-B6", 181, 76, 6, mask="root", expect="style", site=EMB, ksn=6, styles=3),
    row("precise-T76-B2-ring-finish-vector", 181, 76, 2, mask="root", expect="small-tile-hi-lo", site=VEC, precise=True),
    row("precise-T61-B2-F150-ring-finish-scalar", 150, 61, 2, t0=4, expect="small-tile-hi-lo", site=RSCA, precise=True),
    row("trunk-resident-T196-B10-hml-ksn9", 263, 196, 10, mask="root", expect="fused-large-tile", site=EMB, ksn=9, trunk=True),
    row("graph-replay-T76-B2", 181, 76, 2, mask="root", env={"MST_GRAPH": 1, "MST_GRAPH_STEPS": 2}, expect="small-launch-ln-in-gemm",
        site=EMB, graph=True),
]


@pytest.mark.parametrize("c", CHAINS)
def test_five_step_order4_chain_on_every_fused_path(c):
    F, T, B, cfg, env, t0 = c["F"], c["T"], c["B"], c["cfg"], c["env"], c["t0"]
    styles, trunk, precise, graph = c.get("styles", 0), c.get("trunk", False), c.get("precise", False), c.get("graph", False)
    order, n = 4, 5
    mult = 2 if cfg else 1
    # -- which kernels this row runs, from the launch rules
    sl = slices(B, T, cfg, env.get("MST_STREAMS", 0), env.get("MST_SMALL_M", SMALL_M), trunk, precise)
    assert len(sl) == c["nsl"], sl
    if not styles:
        assert {plain_path(mult * nb, T, env.get("MST_SMALL_M", SMALL_M), precise) for _, nb in sl} == {c["expect"]}
    assert draw_site(F, T, cfg, precise) == c["site"]
    assert embeds_next(F, T, cfg, precise, graph) == c["ksn"]
    if styles:
        import style_fixture as sf
        eng = sf.make_engine(F, T, mult * B, styles)
        st = [(0, 1, 1, 2, 0, 2)[i % 6] for i in range(B)]
    else:
        eng = make(F, T, mult * B, env, precise)
        w = weights(F)
    if trunk:
        eng.set_trunk_groups(True)
    assert eng.loop_slices(B, cfg, T) == len(sl)
    sch, tab, tmap = sched(c["resp"])
    assert t0 - n + 1 >= 0 and t0 <= len(tmap) - 1
    shp = (B, F, 1, T)
    x0 = syn.normal(SEED, "pt/x", shp)
    txt = syn.normal(SEED, "pt/txt", (B, 512))
    scale = np.full(B, 2.5, np.float32) if cfg else None
    mask = motion = None
    if c["mask"]:
        mask, motion = mask_of(c["mask"], B, F, T), syn.normal(SEED, "pt/motion", shp)
    eng.set_text(cu(txt), cfg=cfg)
    if styles:
        eng.set_styles(st)
    kw = dict(cfg=cfg, scale=None if scale is None else cu(scale), mask=None if mask is None else cu(mask),
              motion=None if motion is None else cu(motion), dump_xstart=True)

    def chain(x, t_start, nsteps, done, ring, **extra):
        out = eng.sample_loop_plms(sch, x.clone(), t_start, t_start - nsteps + 1, order=order, steps_done=done, hist=ring, **kw, **extra)
        torch.cuda.synchronize()
        return out

    ring = nan_ring(shp)
    final, dump = chain(cu(x0), t0, n, 0, ring)
    assert torch.isfinite(final).all() and torch.isfinite(ring).all() and dump.shape[0] == n
    # -- (c) two runs; (e) a seed, a NaN-filled noise buffer, eta and mask_noise: all ignored.  Bit for bit.
    for extra in (dict(), dict(seed=2 + (5 << 32)), dict(noise=torch.full((n,) + shp, float("nan"), device=dev())), dict(eta=0.7, mask_noise=True)):
        r2 = nan_ring(shp)
        f2, d2 = chain(cu(x0), t0, n, 0, r2, **extra)
        assert torch.equal(final, f2) and torch.equal(dump, d2) and torch.equal(ring, r2), extra.keys()
    # -- (d) the five-step call == five one-step calls with steps_done carried (what the progressive generator runs)
    x, r1 = cu(x0), nan_ring(shp)
    xs, rings = [x0], []
    for k in range(n):
        x, d1 = chain(x, t0 - k, 1, k, r1)
        assert torch.equal(d1[0], dump[k]), f"x0-hat of step {k}: {int((d1[0] != dump[k]).sum())} elements differ"
        xs.append(x.cpu().numpy())
        rings.append(r1.cpu().numpy())
    assert torch.equal(x, final) and torch.equal(r1, ring)
    if trunk:
        eng.trunk_check()

    # the oracle forward on a few clips of the batch (clips are independent): the first and last of every slice
    sel = sorted({i for c0, nb in sl for i in (c0, c0 + nb - 1)} | {B // 2})

    def oracle(xin, t):
        tt = torch.from_numpy(tmap[np.asarray(t)[sel]])
        xi, tx = torch.from_numpy(np.ascontiguousarray(xin[sel])), torch.from_numpy(txt[sel])
        if styles:
            import style_fixture as sf
            ref = np.zeros((len(sel),) + shp[1:], np.float32)
            for s in range(styles):
                rows = [i for i, b in enumerate(sel) if st[b] == s]
                if rows:
                    ref[rows] = sf.oracle_forward(F, s, xi[rows], tt[rows], tx[rows]).numpy()
        elif cfg:
            ref = denoiser.cfg_forward(w, PE, xi, tt, tx, torch.from_numpy(scale[sel])).numpy()
        else:
            ref = denoiser.forward(w, PE, xi, tt, tx).numpy()
        if mask is not None:
            ref = pf.blend(ref, mask[sel], motion[sel]).astype(np.float32)
        return ref

    worst_a = worst_b = 0.0
    for k in range(n):
        t = np.full(B, t0 - k)
        p = dump[k].cpu().numpy()
        # (b) the forward
        e = rel_l2(p[sel], oracle(xs[k], t))
        worst_b = max(worst_b, e)
        assert e <= TOL, f"x0-hat of step {k} (index {t0 - k}): {e:.3e} vs the oracle forward"
        if mask is not None:
            m = mask.astype(bool)
            assert np.array_equal(p[m], motion[m]), "masked entries of x0-hat must be the motion, bit for bit"
        if k == 0:
            # the Euler step: ring slot 0 <- eps of the first evaluation, slot 1 <- the original x, slot 2 untouched
            x_mid, _, eps = pf.euler_first(tab, p, xs[0], t)
            worst_a = max(worst_a, within(rings[0][0], eps, eps_scale(tab, p, xs[0], t), "ring slot 0 after the Euler step"))
            assert np.array_equal(rings[0][1], xs[0]) and np.isnan(rings[0][2]).all()
            ref2 = oracle(x_mid.astype(np.float32), t - 1)
            want, sc = pf.euler_second(tab, ref2, x_mid[sel], xs[0][sel], eps[sel], t[sel])
            p2 = ref2 + (xs[1][sel] - want) / pf.euler_gain(tab, t[sel], ref2)
            e2 = rel_l2(p2, ref2)
            worst_b = max(worst_b, e2)
            assert e2 <= TOL, f"the Euler step's second evaluation (index {t0 - 1}): {e2:.3e} vs the oracle forward"
            if mask is not None:                                  # where the second x0-hat is known exactly, x_1 is closed
                ms = mask[sel].astype(bool)
                worst_a = max(worst_a, within(xs[1][sel][ms], want[ms], sc[ms], "x_1 on the masked entries"))
            continue
        cur = pf.cur_order(order, min(k, order - 1))
        assert cur == (2, 3, 4, 4)[k - 1]
        hist = [rings[k - 1][(k - 1 - i) % 3] for i in range(cur - 1)]          # newest first
        want, sc, eps = pf.closed_form(tab, p, xs[k], t, hist)
        worst_a = max(worst_a, within(xs[k + 1], want, sc, f"x after chain step {k} (index {t0 - k}, cur_order {cur})"))
        worst_a = max(worst_a, within(rings[k][k % 3], eps, eps_scale(tab, p, xs[k], t), f"ring slot {k % 3} after chain step {k}"))
        for s in range(3):
            if s != k % 3:
                assert same(rings[k][s], rings[k - 1][s]), f"chain step {k} touched ring slot {s}"
        if t0 - k == 0:
            assert np.array_equal(xs[k + 1], p), "at index 0 the sample is x0-hat, bit for bit"
    # -- a chain that is one slice of plain kernels: the families a profiled run launches, and that run equals this one
    checked = False
    if len(sl) == 1 and not (styles or trunk or graph):
        eng.profile(True, 1)
        try:
            rp = nan_ring(shp)
            pfin, pdump = chain(cu(x0), t0, n, 0, rp)
            fams = {k for k, v in eng.profile_read().items() if v[1]}
        finally:
            eng.profile(False)
        assert torch.equal(final, pfin) and torch.equal(dump, pdump) and torch.equal(ring, rp)
        assert FAMILIES[c["expect"]] | {"embed_out_step"} <= fams and not fams & (TRUNK_FAMILIES - FAMILIES[c["expect"]]), fams
        checked = True
    if trunk:
        eng.set_trunk_groups(False)
    print(f"\n{c['expect']} / {c['site']} / KSN {c['ksn']} / slices {sl}: update and ring {worst_a:.2e} of scale (bar {BAR_STEP:.0e}), "
          f"x0-hat vs oracle {worst_b:.2e} (bar {TOL:.0e})" + (" / families confirmed by a profiled run" if checked else ""))


# ------------------------------------------------------------------------------ 4. bitwise properties
def test_one_slice_equals_three_slices():
    """MST_STREAMS 1 against 3 on the large-tile path at a fixed tile height: element offsets into x AND the ring, the slice's first
    clip, per-slice warm-up and chaining."""
    F, T, B, n = 181, 76, 24, 5
    sch, _, _ = sched("ddim20")
    x0, txt = cu(syn.normal(SEED, "pb/x", (B, F, 1, T))), cu(syn.normal(SEED, "pb/txt", (B, 512)))
    mask, motion = cu(syn.root_horizontal_mask(B, F, T)), cu(syn.normal(SEED, "pb/motion", (B, F, 1, T)))
    outs = []
    for streams in (1, 3):
        eng = make(F, T, B, {"MST_STREAMS": streams, "MST_SMALL_M": 0, "MST_TAIL_NTB": 4})
        assert eng.loop_slices(B, False, T) == streams
        eng.set_text(txt)
        ring = nan_ring(x0.shape)
        x, d = eng.sample_loop_plms(sch, x0.clone(), 19, 19 - n + 1, order=4, hist=ring, mask=mask, motion=motion, dump_xstart=True)
        outs.append((x, d, ring))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("path", ["small", "large"])
def test_a_clip_does_not_depend_on_its_neighbours(path):
    F, T, B = 181, 76, 3
    eng = make(F, T, B, {"MST_SMALL_M": 0} if path == "large" else None)
    sch, _, _ = sched("ddim20")
    res = []
    for k in (0, 1):
        x = syn.normal(SEED, f"pn/x{k}", (B, F, 1, T))
        txt = syn.normal(SEED, f"pn/txt{k}", (B, 512))
        motion = syn.normal(SEED, f"pn/motion{k}", (B, F, 1, T))
        x[1], txt[1], motion[1] = syn.normal(SEED, "pn/x", (F, 1, T)), syn.normal(SEED, "pn/t", (512,)), syn.normal(SEED, "pn/m", (F, 1, T))
        eng.set_text(cu(txt))
        ring = nan_ring(x.shape)
        out = eng.sample_loop_plms(sch, cu(x), 19, 15, order=4, hist=ring, mask=cu(syn.root_horizontal_mask(B, F, T)), motion=cu(motion))
        res.append((out, ring))
    torch.cuda.synchronize()
    assert torch.equal(res[0][0][1], res[1][0][1]) and torch.equal(res[0][1][:, 1], res[1][1][:, 1])
    assert not torch.equal(res[0][0][0], res[1][0][0])


def test_every_order_through_a_graph_equals_the_host_enqueued_loop():
    """Seven steps from the last index of ddim20 at orders 1 .. 4: MST_GRAPH=1 with two-step graphs (the warm-up and the remainder from
    the host, then replays of ONE captured graph -- the same for every order and every position in a chain, so one engine runs them
    all) against MST_GRAPH=0.  Every order twice: the second call only replays."""
    F, T, B, n = 181, 76, 2, 7
    sch, _, _ = sched("ddim20")
    x0, txt = cu(syn.normal(SEED, "pg/x", (B, F, 1, T))), cu(syn.normal(SEED, "pg/txt", (B, 512)))
    engs = [make(F, T, B, {"MST_GRAPH": graph, "MST_GRAPH_STEPS": 2}) for graph in (0, 1)]
    for eng in engs:
        eng.set_text(txt)
    for order in (1, 2, 3, 4, 2):
        outs = []
        for eng in engs:
            for rep in range(2):
                ring = nan_ring(x0.shape) if order > 1 else None
                x, d = eng.sample_loop_plms(sch, x0.clone(), 19, 19 - n + 1, order=order, hist=ring, dump_xstart=True)
                torch.cuda.synchronize()
                outs.append((x, d) + ((ring,) if ring is not None else ()))
        assert torch.isfinite(outs[0][0]).all() and all(torch.isfinite(o[-1]).all() for o in outs)
        for o in outs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(outs[0], o)), order


def _plms_diffusion():
    from mst_amd.diffusion import gaussian_diffusion as gd
    from mst_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    return SpacedDiffusion(use_timesteps=space_timesteps(1000, "ddim20"), betas=gd.get_named_beta_schedule("cosine", 1000),
                           model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE)


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_loop_entries_of_the_mirror_agree_bit_for_bit(order):
    """plms_sample_loop (one native call) == its progressive generator (a native call per index, steps_done carried) ==
    plms_sample_loop_from(x_T, 20); nothing is drawn from torch's generator; the generator's old_eps are clones of the ring, newest
    last, at most order - 1 long; every yielded step is the float64 update of its own x0-hat and history."""
    c, shp, y = _model()
    d, m = c["ddim"], c["m"]
    x0 = cu(syn.normal(SEED, "pm/x", shp))
    torch.manual_seed(3)
    before = torch.get_rng_state()
    whole = d.plms_sample_loop(m, shp, noise=x0, clip_denoised=False, model_kwargs=y, order=order)
    assert torch.equal(torch.get_rng_state(), before), "the PLMS loop drew from torch's generator"
    prog = list(d.plms_sample_loop_progressive(m, shp, noise=x0, clip_denoised=False, model_kwargs=y, order=order))
    assert len(prog) == 20 and all(o["sample"] is not None and isinstance(o["old_eps"], list) for o in prog)
    assert torch.equal(prog[-1]["sample"], whole)
    assert torch.equal(d.plms_sample_loop_from(m, x0, 20, order=order, clip_denoised=False, model_kwargs=y), whole)
    dump = d.plms_sample_loop_from(m, x0, 20, order=order, clip_denoised=False, model_kwargs=y, dump_all_xstart=True)
    assert len(dump) == 20 and all(torch.equal(a, o["pred_xstart"]) for a, o in zip(dump, prog))
    assert torch.equal(x0, cu(syn.normal(SEED, "pm/x", shp))), "the caller's clip was modified"
    assert [len(o["old_eps"]) for o in prog] == [min(k + 1, order - 1) for k in range(20)]
    _, tab, _ = sched("ddim20")
    x, hist = x0.cpu().numpy(), []
    for k, o in enumerate(prog):
        t = np.full(shp[0], 19 - k)
        p = o["pred_xstart"].cpu().numpy()
        eps = pf.eps_of(tab, p, x, t)
        if order > 1:
            within(o["old_eps"][-1].cpu().numpy(), eps, eps_scale(tab, p, x, t), f"old_eps[-1] of step {k}")
            for a, b in zip(o["old_eps"][:-1][::-1], hist):       # the older entries are the earlier steps' eps, bit for bit
                assert np.array_equal(a.cpu().numpy(), b)
        if k > 0 or order == 1:
            cur = pf.cur_order(order, len(hist[:order - 1]))
            want, sc, _ = pf.closed_form(tab, p, x, t, hist[:cur - 1])
            within(o["sample"].cpu().numpy(), want, sc, f"generator step {k}")
        hist = ([o["old_eps"][-1].cpu().numpy()] + hist)[:3] if order > 1 else []
        x = o["sample"].cpu().numpy()


def test_a_plain_callable_goes_step_by_step_through_the_standalone_kernels():
    """The model behind a lambda: plms_sample per index (model calls + mst_plms_epilogue / mst_plms_euler), the live old_eps list; against
    the native loop: x0-hat within the forward bar at the first step, every update the float64 closed form of its own x0-hat."""
    c, shp, y = _model()
    d, m = _plms_diffusion(), c["m"]                                # (plain SpacedDiffusion: q_sample of the skipped start wants no mask)
    x0 = cu(syn.normal(SEED, "pm/x", shp))
    plain = lambda xx, tt, **kw: m(xx, tt, **kw)
    _, tab, _ = sched("ddim20")
    native = list(d.plms_sample_loop_progressive(m, shp, noise=x0, clip_denoised=False, model_kwargs=y, order=3, skip_timesteps=16))
    outs, lens = [], []
    for o in d.plms_sample_loop_progressive(plain, shp, noise=x0, clip_denoised=False, model_kwargs=y, order=3, device=dev(), skip_timesteps=16):
        outs.append(o)
        lens.append(len(o["old_eps"]))
    assert len(outs) == 4 and lens == [1, 2, 2, 2]
    assert all(o["old_eps"] is outs[0]["old_eps"] for o in outs), "the live list, as in the reference"
    # (skip_timesteps with no init_image: q_sample of zeros at index 3, then indices 3 .. 0)
    x = d.q_sample(torch.zeros_like(x0), torch.full((shp[0],), 3, device=dev()), x0).cpu().numpy()
    hist = []
    for k, o in enumerate(outs):
        t = np.full(shp[0], 3 - k)
        p = o["pred_xstart"].cpu().numpy()
        if k > 0:
            want, sc, _ = pf.closed_form(tab, p, x, t, hist[:min(2, k)])
            within(o["sample"].cpu().numpy(), want, sc, f"per-step call {k}")
        hist = [pf.eps_of(tab, p, x, t).astype(np.float32)] + hist
        x = o["sample"].cpu().numpy()
    assert rel_l2(outs[0]["pred_xstart"].cpu().numpy(), native[0]["pred_xstart"].cpu().numpy()) < TOL
    assert np.array_equal(outs[-1]["sample"].cpu().numpy(), outs[-1]["pred_xstart"].cpu().numpy())      # index 0


# ------------------------------------------------------------------------------ 5. whole loops against the reference
def test_whole_20_step_loops_vs_the_reference():
    """This engine's 20-step PLMS loops at orders 2, 3, 4 against the reference's own (tests/golden/plms.npz), from the same noise.
    The yardstick is existing behaviour: e_ddim, this engine's DDIM eta-0 loop against the reference's DDIM golden from that noise.
    A per-step x0-hat error reaches eps' multiplied by at most A_r = sum |a_i| (2, 44/12, 160/24), so the PLMS error at order r must
    be at most A_r * e_ddim.  Measured on an MI355X: see docs/LAB_NOTES.md, "PLMS"."""
    from test_gpu_boundary import PROMPTS, build
    m = build()["m"]
    d = _plms_diffusion()
    g = pf.golden()
    noise = cu(pf.golden_noise())
    T = noise.shape[-1]
    assert pf.PROMPT == PROMPTS[0]
    y = {"y": {"text": [pf.PROMPT], "mask": torch.ones(1, 1, 1, T, device=dev())}}
    torch.manual_seed(1)
    ddim = d.ddim_sample_loop(m, tuple(noise.shape), noise=noise, clip_denoised=False, model_kwargs=y, eta=0.0)
    e_ddim = rel_l2(ddim.cpu().numpy(), g["xia|loop20|ddim"])
    errs = {}
    for r in (2, 3, 4):
        out = d.plms_sample_loop(m, tuple(noise.shape), noise=noise, clip_denoised=False, model_kwargs=y, order=r)
        assert torch.isfinite(out).all()
        errs[r] = rel_l2(out.cpu().numpy(), g[f"xia|loop20|plms{r}"])
    print(f"\n20-step loops vs the reference: e_ddim {e_ddim:.3e}; " +
          ", ".join(f"PLMS order {r} {errs[r]:.3e} (bar A_{r} e_ddim = {pf.A[r] * e_ddim:.3e})" for r in errs))
    for r in errs:
        assert errs[r] <= pf.A[r] * e_ddim, (r, errs[r], pf.A[r] * e_ddim)


# ------------------------------------------------------------------------------ 6. refusals
def test_refusals_name_their_reason(monkeypatch):
    from mst_amd import _native as N
    from mst_amd.engine import SAMPLER_PLMS
    F, T, B = 181, 76, 2
    eng = make(F, T, B)
    sch, _, _ = sched("ddim20")
    eng.set_text(cu(syn.normal(SEED, "pr/txt", (B, 512))))
    x = cu(syn.normal(SEED, "pr/x", (B, F, 1, T)))
    keep = x.clone()
    ring = nan_ring(x.shape)
    for bad in (0, 5, -2):
        with pytest.raises(RuntimeError, match="order .* is invalid"):
            eng.sample_loop_plms(sch, x, 5, 3, order=bad, hist=ring)
    with pytest.raises(RuntimeError, match="steps_done -1 is negative"):
        eng.sample_loop_plms(sch, x, 5, 3, order=2, steps_done=-1, hist=ring)
    with pytest.raises(RuntimeError, match="hist_dev is NULL"):
        eng.sample_loop_plms(sch, x, 5, 3, order=2, hist=None)
    with pytest.raises(RuntimeError, match="cannot start at index 0"):
        eng.sample_loop_plms(sch, x, 0, 0, order=2, hist=ring)
    with pytest.raises(RuntimeError, match="bad index range"):
        eng.sample_loop_plms(sch, x, 3, 5, order=2, hist=ring)
    with pytest.raises(RuntimeError, match="bad index range"):
        eng.sample_loop_plms(sch, x, 20, 18, order=2, hist=ring)
    with pytest.raises(RuntimeError, match="bad sampler 3: MST_SAMPLER_PLMS .* call mst_sample_loop_plms"):      # the generic entry names the new one
        eng.sample_loop(sch, x, 5, 3, SAMPLER_PLMS)
    with pytest.raises(RuntimeError, match="bad sampler 3"):
        sch.step(x, x, cu(np.array([0, 1])), None, SAMPLER_PLMS)
    torch.cuda.synchronize()
    assert torch.equal(x, keep) and torch.isnan(ring).all(), "a refused call touched x or the ring"
    # what is NOT refused: order 1 without a ring, at index 0; a continued chain at index 0
    eng.sample_loop_plms(sch, x.clone(), 0, 0, order=1, hist=None)
    eng.sample_loop_plms(sch, x.clone(), 0, 0, order=2, steps_done=1, hist=torch.zeros_like(ring))
    t = cu(np.array([0, 1]))
    with pytest.raises(ValueError, match="order is invalid"):
        sch.plms_step(x, x, t, history=[x, x, x, x])
    with pytest.raises(RuntimeError, match="bad mean type"):
        sch.plms_step(x, x, t, mean_type=3)
    g, out = torch.ones_like(x), torch.empty_like(x)
    rc = N.lib().mst_step_backward(sch.handle, N.ptr(g), None, None, 0, N.ptr(t), B, x.numel() // B, SAMPLER_PLMS, C.c_float(0.0), None,
                                   N.ptr(out), N.stream_ptr(dev()))
    assert rc != 0
    msg = N.lib().mst_last_error().decode()
    assert "MST_SAMPLER_PLMS" in msg and "_with_grad" in msg, msg
    rc = N.lib().mst_plms_epilogue(sch.handle, N.ptr(x), N.ptr(x), None, None, N.ptr(t), B, x.numel() // B, 0, 0, 3, 0, N.ptr(x), None, None,
                                   N.ptr(out), None, None, N.stream_ptr(dev()))
    assert rc != 0 and "needs 2 history entries" in N.lib().mst_last_error().decode()
    torch.cuda.synchronize()
    # several styles: what style_check refuses for every loop, it refuses here
    import style_fixture as sf
    seng = sf.make_engine(F, T, 6, 3)
    seng.set_text(cu(syn.normal(SEED, "pr/txt6", (6, 512))))
    seng.set_styles([0, 1, 2, 0, 1, 2])
    x6, r6 = cu(syn.normal(SEED, "pr/x6", (6, F, 1, T))), nan_ring((6, F, 1, T))
    seng.set_precise(True)
    with pytest.raises(RuntimeError, match="precise"):
        seng.sample_loop_plms(sch, x6, 19, 17, order=2, hist=r6)
    seng.set_precise(False)
    seng.set_trunk_groups(True)
    with pytest.raises(RuntimeError, match="several styles: the resident trunk"):
        seng.sample_loop_plms(sch, x6, 19, 17, order=2, hist=r6)
    seng.set_trunk_groups(False)
    seng.profile(True, 1)
    try:
        with pytest.raises(RuntimeError, match="several styles: profiling"):
            seng.sample_loop_plms(sch, x6, 19, 17, order=2, hist=r6)
    finally:
        seng.profile(False)
    seng.set_styles([0, 1, 2])
    with pytest.raises(RuntimeError, match="named 3 clips, the call has 6"):
        seng.sample_loop_plms(sch, x6, 19, 17, order=2, hist=r6)
    torch.cuda.synchronize()
    assert torch.isnan(r6).all()
    # the mirror
    c, shp, y = _model()
    d, m = c["ddim"], c["m"]
    xm = cu(syn.normal(SEED, "pr/xm", shp))
    with pytest.raises(ValueError, match="order is invalid"):
        d.plms_sample_loop(m, shp, noise=xm, model_kwargs=y, order=5)
    with pytest.raises(ValueError, match="cannot start at index 0"):
        d.plms_sample_loop_from(m, xm, 1, order=2, model_kwargs=y)
    with pytest.raises(NotImplementedError, match="cond_fn"):
        d.plms_sample_loop(m, shp, noise=xm, model_kwargs=y, cond_fn=lambda *a, **k: None)
    with pytest.raises(NotImplementedError, match="randomize_class"):
        d.plms_sample_loop(m, shp, noise=xm, model_kwargs=y, randomize_class=True)


# ------------------------------------------------------------------------------ 7. the recipe
def test_invert_once_decode_with_plms_under_three_styles_as_one_batch():
    """ddim_reverse_sample_loop under slot 0, the latents repeated 3 times, decoded by plms_sample_loop_from as ONE 6-clip batch with
    y['style']: each style's clips equal, bit for bit, that style's own single-style decode of the same latents (the comparison and the
    bar of tests/test_gpu_reverse.py's DDIM recipe).  Also under ClassifierFreeSampleModel."""
    from mst_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from test_gpu_style_bank import K, SHAPES, _bank
    F, T = SHAPES["xia"]
    bank, _ = _bank("xia")
    assert K == 3
    d = _plms_diffusion()
    B = 2
    content = cu(syn.normal(SEED, "pc/content", (B, F, 1, T)))
    txt = cu(syn.normal(SEED, "pc/txt", (B, 512)))
    for model, extra in ((bank, {}), (ClassifierFreeSampleModel(bank), {"scale": cu(np.full(B, 2.5, np.float32))})):
        yi = {"y": {"text_embed": txt, "style": torch.zeros(B, dtype=torch.long), **extra}}
        latents = d.ddim_reverse_sample_loop(model, content, num_steps=8, clip_denoised=False, model_kwargs=yi)
        rep = lambda v: v.repeat(K, *([1] * (v.dim() - 1)))
        style = torch.arange(K).repeat_interleave(B)
        y6 = {"y": {"text_embed": rep(txt), "style": style, **{k: rep(v) for k, v in extra.items()}}}
        mixed = d.plms_sample_loop_from(model, rep(latents), 8, order=3, clip_denoised=False, model_kwargs=y6)
        assert mixed.shape[0] == K * B and torch.isfinite(mixed).all()
        for s in range(K):
            ys = {"y": {**y6["y"], "style": torch.full((K * B,), s)}}
            alone = d.plms_sample_loop_from(model, rep(latents), 8, order=3, clip_denoised=False, model_kwargs=ys)
            rows = (style == s).nonzero().flatten().tolist()
            assert torch.equal(mixed[rows], alone[rows]), s
        assert not torch.equal(mixed[0:B], mixed[B:2 * B])                                # the styles do differ
