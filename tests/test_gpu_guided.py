"""Guided sampling on the GPU (reference gaussian_diffusion.py:454-506, :577-580, :821-847): the guided update at every site that applies
the diffusion step (MODEs 5 / 6 of the fused kernels, k_step_epilogue_guided stand-alone), both kinds of guide, the loops, denoised_fn.

  1. the stand-alone kernel against the float64 closed forms (tests/guide_fixture.py): every index, both samplers, every MEAN, blend,
     clamp, both guide kinds, with and without the guide's mask, both a_t modes; x0-hat bit-equal to the unguided call;
  2. fused single steps against the reference's own outputs (tests/golden/guided.npz) on the small- and the large-tile path;
  3. bitwise properties of the target kind: k steps == k one-step calls, 3 slices == 1, neighbours, weight 0, graph replay, CFG, a
     two-style bank, the sites the Xia shapes do not reach (scalar epilogue, precise mode's ring GEMM); the gradient kind fed with
     TargetGuide.__call__'s tensor against the target kind;
  4. whole 20-step loops against the reference's guided goldens, natively (TargetGuide) and step by step (the guide behind a lambda);
  5. denoised_fn;  6. refusals, each naming its reason.

The bars.  Updates are elementwise, 2e-5 (tests/test_gpu_parity.py's stand-alone-step constant) of `scale`, the summed magnitudes of
the products the value is built from (guide_fixture); tests/test_guided_cpu.py holds the reference's own goldens to the same bar.
x0-hat against the reference is the project's forward bar, 1e-3 relative L2."""
import ctypes as C

import numpy as np
import pytest
import torch

import guide_fixture as gf
import mst_amd  # noqa: F401
import mst_amd.synthetic as syn
from conftest import SEED, rel_l2
from plan_mirror import SMALL_M, plain_path, slices
from test_gpu_noise import draw_site
from test_gpu_reverse import EMB, RSCA, SCA, TOL, VEC, _model, _step_inputs, cu, dev, embeds_next, make, sched, within

pytestmark = pytest.mark.gpu
BAR_STEP = gf.BAR_STEP
DDPM, DDIM = 0, 1


def G(x, **kw):
    from mst_amd.engine import guide_args
    return guide_args(x, **kw)


def guide_np(B, F, T, tag="gs"):
    """A seeded guide for B clips: target, a mask that is mixed inside rows, one weight per clip (clip 0: weight 0)."""
    shp = (B, F, 1, T)
    m = (syn.uniform(SEED, tag + "/m", shp, 0.0, 1.0) < 0.4).astype(np.float32)
    w = np.linspace(0.0, 2.0, B).astype(np.float32)
    return 3.0 * syn.normal(SEED, tag + "/y", shp), m, w


# ------------------------------------------------------------------------------ 1. the stand-alone kernel
STEP_T = {"ddim20": [list(range(0, 7)), list(range(7, 14)), list(range(14, 20)) + [19]], "": [[0, 1, 500, 999, 999, 1, 0]]}


def _standalone(sch, tab, sampler, eta, mean, v, t, gnp, var=None, B=7):
    """Every blend / clamp / guide combination at indices t; returns the worst ratio."""
    y, m, w = gnp
    x = v["x"]
    noise = syn.normal(SEED, "gs/noise", x.shape)
    worst = 0.0
    for blend in (False, True):
        for clamp in (False, True):
            mk, mot = (v["mask"], v["motion"]) if blend else (None, None)
            kw = dict(sampler=sampler, eta=eta, mask=None if mk is None else cu(mk), motion=None if mot is None else cu(mot),
                      mask_noise=blend, clip_denoised=clamp, mean_type=mean)
            s0, p0 = sch.step(cu(v["mo"]), cu(x), cu(t), cu(noise), **kw)
            nz = noise * (1 - mk) if blend else noise
            guides = [("gradient", None, None)] + [("target", mm, f) for mm in (None, m) for f in (0, 1)]
            for kind, mm, follow in guides:
                if kind == "gradient":
                    grad = syn.normal(SEED, "gs/grad", x.shape)
                    ga = G(cu(x), grad=cu(grad))
                else:
                    grad = gf.target_grad(tab, x, t, y, mm, w, follow)
                    ga = G(cu(x), target=cu(y), mask=None if mm is None else cu(mm), weight=cu(w), follow_schedule=follow)
                s, p = sch.step_guided(cu(v["mo"]), cu(x), cu(t), cu(noise), ga, **kw)
                assert torch.equal(p, p0), "x0-hat must not see the guide"
                s, p = s.cpu().numpy(), p.cpu().numpy()
                assert np.isfinite(s).all()
                extra = {}
                if sampler == DDPM:
                    extra["var"] = var
                    if mean == 2:
                        extra["raw_mean"] = gf.xstart64(tab, 2, v["mo"], x, t, mk, mot, False)[1]
                want, scale = gf.guided(tab, None if sampler == DDPM else eta, p, x, t, grad, nz, **extra)
                worst = max(worst, within(s, want, scale, f"t {list(t)} blend {blend} clamp {clamp} {kind} mask {mm is not None} follow {follow}"))
                zero = np.asarray(t) == 0
                if sampler == DDPM and var is None and zero.any():            # variance_0 = 0: bit-equal to the unguided step there
                    assert np.array_equal(s[zero], s0.cpu().numpy()[zero])
                assert not np.array_equal(s[~zero], s0.cpu().numpy()[~zero])
    return worst


@pytest.mark.parametrize("mean", [0, 1, 2], ids=["x_start", "epsilon", "previous_x"])
@pytest.mark.parametrize("sampler,eta", [(DDPM, 0.0), (DDIM, 0.5)], ids=["ddpm", "ddim.5"])
def test_standalone_guided_step_equals_the_float64_closed_form(sampler, eta, mean):
    """Schedule.step_guided: seven clips at seven indices a call (every index of ddim20; 0, 1, 500, 999 of the full schedule), B, F, T =
    7, 24, 10.  x0-hat bit-equal to the unguided call; the sample within 2e-5 of scale of the closed form applied to the kernel's own
    x0-hat; the guided sample differs from the unguided one wherever the guide can act."""
    B, F, T = 7, 24, 10
    v = _step_inputs(B, F, T)
    gnp = guide_np(B, F, T)
    worst = 0.0
    for resp in ("ddim20", ""):
        sch, tab, _ = sched(resp)
        for ts in STEP_T[resp]:
            worst = max(worst, _standalone(sch, tab, sampler, eta, mean, v, np.asarray(ts), gnp))
    print(f"\nstand-alone guided step sampler {sampler} mean {mean}: worst |kernel - closed form| / scale {worst:.2e} (bar {BAR_STEP:.0e})")


def test_standalone_guided_step_reads_the_variance_row_it_was_given():
    """FIXED_LARGE: the betas-based row (nonzero at index 0), not the posterior variance and not exp(log_variance)."""
    from mst_amd.engine import Schedule
    tab, tmap = gf.tables("ddim20")
    var = gf.variance_row(tab, large=True)
    sch = Schedule(tab, tmap, dev(), log_variance=np.log(var), variance=var)
    B, F, T = 7, 24, 10
    r = _standalone(sch, tab, DDPM, 0.0, 0, _step_inputs(B, F, T), np.array([0, 1, 5, 10, 15, 18, 19]), guide_np(B, F, T), var=var)
    print(f"\nFIXED_LARGE: worst ratio {r:.2e}")


def test_standalone_guided_step_more_than_one_block_per_clip():
    """per_clip = 263 * 196 = 51548 elements (202 blocks of 256 threads per clip), three clips at three indices, both samplers."""
    sch, tab, _ = sched("ddim20")
    B, F, T = 3, 263, 196
    v = _step_inputs(B, F, T)
    y, m, w = guide_np(B, F, T)
    w = np.array([0.5, 1.0, 2.0], np.float32)
    t = np.array([0, 11, 19])
    noise = syn.normal(SEED, "gs/noise", v["x"].shape)
    grad = gf.target_grad(tab, v["x"], t, y, m, w, 1)
    ga = G(cu(v["x"]), target=cu(y), mask=cu(m), weight=cu(w), follow_schedule=1)
    for sampler, eta in ((DDPM, 0.0), (DDIM, 0.5)):
        s, p = sch.step_guided(cu(v["mo"]), cu(v["x"]), cu(t), cu(noise), ga, sampler=sampler, eta=eta, mask=cu(v["mask"]), motion=cu(v["motion"]),
                               mask_noise=True)
        want, scale = gf.guided(tab, None if sampler == DDPM else eta, p.cpu().numpy(), v["x"], t, grad, noise * (1 - v["mask"]))
        print(f"\nsampler {sampler}: worst ratio {within(s.cpu().numpy(), want, scale, 'sample'):.2e}")


# ------------------------------------------------------------------------------ 2. fused single steps against the reference
@pytest.mark.parametrize("path", ["small", "large"])
@pytest.mark.parametrize("tag", ["xia", "hml"])
def test_fused_single_steps_vs_the_reference(tag, path):
    """One-step native calls (the target kind, both a_t modes; p_sample, ddim eta 0 and eta 0.5, recorded noise) at every golden case.
    Small-tile path: one clip.  Large-tile path: 26 copies of the clip (Xia: 2002 token rows > MST_SMALL_M = 1900).  x0-hat within 1e-3
    of the reference's; the sample recomputed in float64 from the engine's own x0-hat within 2e-5 of scale."""
    g = gf.golden()
    v = gf.golden_inputs(tag)
    F, T, st = v["F"], v["T"], gf.STRIDE[tag]
    B = 1 if path == "small" else 26
    assert plain_path(B, T) == ("fused-large-tile" if path == "large" else "small-launch-ln-in-gemm")
    eng = make(F, T, B)
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape[1:]))
    eng.set_text(cu(rep(v["txt"])))
    x = rep(v["x"])
    worst_p = worst_s = worst_ref = 0.0
    for tg, resp, t, variant in [c for c in gf.single_step_cases() if c[0] == tag]:
        sch, tab, _ = sched(resp)
        key = gf.key_of(tag, resp, t, variant)
        noise = gf.step_noise(tag, key)
        kw = dict(mask=cu(rep(v["mask"])), motion=cu(rep(v["motion"])), mask_noise=True) if variant else dict(mask_noise=False)
        nz = noise * (1 - v["mask"]) if variant else noise
        for sampler, eta in gf.SAMPLERS.items():
            for follow in (0, 1):
                ga = G(cu(x), target=cu(rep(v["y"])), mask=cu(rep(v["m"])), weight=gf.WEIGHT, follow_schedule=follow)
                s, d = eng.sample_loop(sch, cu(x), t, t, DDPM if eta is None else DDIM, eta or 0.0, noise=cu(rep(noise))[None], dump_xstart=True,
                                       guide=ga, **kw)
                s, p = s.cpu().numpy(), d[0].cpu().numpy()
                assert all(np.array_equal(s[0], s[b]) for b in range(1, B))
                ep = rel_l2(p[:1, ..., ::st], g[key + "|pred_xstart"])
                assert ep <= TOL, (key, sampler, ep)
                grad = gf.target_grad(tab, v["x"], [t], v["y"], v["m"], gf.WEIGHT, follow)
                want, scale = gf.guided(tab, sampler, p[:1], v["x"], [t], grad, nz)
                worst_s = max(worst_s, within(s[:1], want, scale, f"{key} {sampler} follow {follow}"))
                worst_ref = max(worst_ref, rel_l2(s[:1, ..., ::st], g[f"{key}|{sampler}|{follow}|sample"]))
                worst_p = max(worst_p, ep)
                if variant:
                    assert np.array_equal(p[:, :3], rep(v["motion"])[:, :3])
    print(f"\n{tag} {path}: worst x0-hat {worst_p:.2e} (bar {TOL:.0e}), worst update {worst_s:.2e} of scale (bar {BAR_STEP:.0e}), "
          f"worst sample vs the reference's {worst_ref:.2e}")


# ------------------------------------------------------------------------------ 3. properties of the target kind
def row(id, F, T, B, sampler=DDPM, eta=0.0, resp="ddim20", t0=19, cfg=False, mask=None, env=None, expect=None, site=None, nsl=1, ksn=0, **variant):
    return pytest.param(dict(F=F, T=T, B=B, sampler=sampler, eta=eta, resp=resp, t0=t0, cfg=cfg, mask=mask, env=env or {}, expect=expect,
                             site=site, nsl=nsl, ksn=ksn, **variant), id=id)


# t0: the index the loop STARTS at (it runs down over four indices; t0 = 3 ends at index 0).
LOOPS = [
    row("small-launch-T76-B2-ddpm-root-mask-ksn6", 181, 76, 2, mask="root", expect="small-launch-ln-in-gemm", site=EMB, ksn=6),
    row("small-tile-T76-B9-ddim.5-ksn6-to-index-0", 181, 76, 9, DDIM, 0.5, t0=3, expect="small-tile", site=EMB, ksn=6),
    row("fused-large-T196-B2-hml-ddpm-ksn9-root-mask-full-schedule", 263, 196, 2, resp="", t0=999, mask="root", env={"MST_SMALL_M": 0},
        expect="fused-large-tile", site=EMB, ksn=9),
    row("fused-large-T76-B2-ddim0-to-index-0", 181, 76, 2, DDIM, 0.0, t0=3, env={"MST_SMALL_M": 0}, expect="fused-large-tile", site=EMB, ksn=6),
    row("scalar-T75-B3-F190-ddpm-resp100", 190, 75, 3, resp="100", t0=50, mask="root", expect="small-launch-ln-in-gemm", site=SCA),
    row("scalar-large-T75-B3-F190-ddim.5", 190, 75, 3, DDIM, 0.5, env={"MST_SMALL_M": 0}, expect="fused-large-tile", site=SCA),
    row("cfg2.5-small-T76-B2-ddpm", 181, 76, 2, cfg=True, mask="root", expect="small-launch-ln-in-gemm", site=EMB),
    row("cfg2.5-large-T76-B2-ddim.5", 181, 76, 2, DDIM, 0.5, cfg=True, env={"MST_SMALL_M": 0}, expect="fused-large-tile", site=EMB),
    row("slices-T76-B24-3x8-ddpm-ksn6-root-mask", 181, 76, 24, mask="root", env={"MST_STREAMS": 3}, expect="small-tile", site=EMB, nsl=3, ksn=6),
    row("styles-2slots-T76-B6-ddim.5", 181, 76, 6, DDIM, 0.5, mask="root", expect="style", site=EMB, ksn=6, styles=2),
    row("precise-T76-B2-ddpm-ring-finish-vector", 181, 76, 2, mask="root", expect="small-tile-hi-lo", site=VEC, precise=True),
    row("precise-T61-B2-F150-ddim.5-ring-finish-scalar", 150, 61, 2, DDIM, 0.5, t0=3, expect="small-tile-hi-lo", site=RSCA, precise=True),
    row("graph-replay-T76-B2-ddpm", 181, 76, 2, mask="root", env={"MST_GRAPH": 1, "MST_GRAPH_STEPS": 2}, expect="small-launch-ln-in-gemm",
        site=EMB, graph=True),
    row("graph-replay-T76-B2-ddim.5", 181, 76, 2, DDIM, 0.5, env={"MST_GRAPH": 1, "MST_GRAPH_STEPS": 2}, expect="small-launch-ln-in-gemm",
        site=EMB, graph=True),
]


@pytest.mark.parametrize("c", LOOPS)
def test_four_step_target_guided_loop_on_every_fused_path(c):
    """A four-step loop with in-kernel Philox noise replaced by a buffer (so the float64 form can follow it), rows as
    tests/test_gpu_reverse.py's TRAJ, each asserting from mirrors of the launch rules which kernels it runs:
      (a) every x_{k+1} recomputed in float64 from the engine's OWN x0-hat, x_k, the guide and the noise: 2e-5 of scale;
      (b) one four-step call == four one-step calls, bit for bit (x and every x0-hat); two runs are the same bits;
      (c) x0-hat is bit-equal to the UNGUIDED loop's at the first step (same x), and the samples differ;
      (d) weight 0, one step: the same x0-hat bit for bit and a sample within 2e-5 of scale of the unguided step's.  Not bit for bit: the
          DDIM form re-derives pred' = srac x - srm1ac eps from eps = (srac x - pred) / srm1ac even when the guide adds nothing, which does
          not round back to pred; and the ancestral mean c1 pred + c2 x is contracted to ONE fma by the compiler, which is free to fuse
          either product and chooses per instantiation (measured: 12 of these 14 rows are bit-equal, the element-wise epilogue and the
          ring GEMM's vector epilogue are not), so equality of bits is not a property of the formulation."""
    F, T, B, cfg, env, t0, sampler, eta = c["F"], c["T"], c["B"], c["cfg"], c["env"], c["t0"], c["sampler"], c["eta"]
    styles, precise, graph = c.get("styles", 0), c.get("precise", False), c.get("graph", False)
    n, mult = 4, 2 if cfg else 1
    sl = slices(B, T, cfg, env.get("MST_STREAMS", 0), env.get("MST_SMALL_M", SMALL_M), False, precise)
    assert len(sl) == c["nsl"], sl
    if not styles:
        assert {plain_path(mult * nb, T, env.get("MST_SMALL_M", SMALL_M), precise) for _, nb in sl} == {c["expect"]}
    assert draw_site(F, T, cfg, precise) == c["site"]
    assert embeds_next(F, T, cfg, precise, graph) == c["ksn"]
    if styles:
        import style_fixture as sf
        eng = sf.make_engine(F, T, mult * B, styles)
    else:
        eng = make(F, T, mult * B, env, precise)
    assert eng.loop_slices(B, cfg, T) == len(sl)
    sch, tab, _ = sched(c["resp"])
    shp = (B, F, 1, T)
    x0, txt = syn.normal(SEED, "gl/x", shp), syn.normal(SEED, "gl/txt", (B, 512))
    noise = syn.normal(SEED, "gl/noise", (n,) + shp)
    y, m, w = guide_np(B, F, T, "gl")
    w = w + 0.5
    mask = motion = None
    if c["mask"]:
        mask, motion = syn.root_horizontal_mask(B, F, T), syn.normal(SEED, "gl/motion", shp)
    eng.set_text(cu(txt), cfg=cfg)
    if styles:
        eng.set_styles([(0, 1, 1, 0, 1, 0)[i % 6] for i in range(B)])
    kw = dict(cfg=cfg, scale=cu(np.full(B, 2.5, np.float32)) if cfg else None, mask=None if mask is None else cu(mask),
              motion=None if motion is None else cu(motion), mask_noise=mask is not None, dump_xstart=True)

    def loop(x, t_start, nsteps, nz, weight=w, guided=True):
        ga = G(x, target=cu(y), mask=cu(m), weight=cu(weight), follow_schedule=1) if guided else None
        out = eng.sample_loop(sch, x.clone(), t_start, t_start - nsteps + 1, sampler, eta, noise=nz, guide=ga, **kw)
        torch.cuda.synchronize()
        return out

    final, dump = loop(cu(x0), t0, n, cu(noise))
    assert torch.isfinite(final).all() and dump.shape[0] == n
    f2, d2 = loop(cu(x0), t0, n, cu(noise))
    assert torch.equal(final, f2) and torch.equal(dump, d2)
    # (b) + (a)
    x, xs = cu(x0), [x0]
    for k in range(n):
        x, d1 = loop(x, t0 - k, 1, cu(noise[k:k + 1]))
        assert torch.equal(d1[0], dump[k]), f"x0-hat of step {k}: {int((d1[0] != dump[k]).sum())} elements differ"
        xs.append(x.cpu().numpy())
    assert torch.equal(x, final)
    worst = 0.0
    for k in range(n):
        t = np.full(B, t0 - k)
        nz = noise[k] * (1 - mask) if mask is not None else noise[k]
        grad = gf.target_grad(tab, xs[k], t, y, m, w, 1)
        want, scale = gf.guided(tab, None if sampler == DDPM else eta, dump[k].cpu().numpy(), xs[k], t, grad, nz)
        worst = max(worst, within(xs[k + 1], want, scale, f"step {k}"))
    # (c) + (d)
    p_final, p_dump = loop(cu(x0), t0, n, cu(noise), guided=False)
    assert torch.equal(p_dump[0], dump[0]) and not torch.equal(p_final, final)
    u, ud = loop(cu(x0), t0, 1, cu(noise[:1]), guided=False)
    z, zd = loop(cu(x0), t0, 1, cu(noise[:1]), weight=np.zeros(B, np.float32))
    assert torch.equal(zd, ud)
    nz = noise[0] * (1 - mask) if mask is not None else noise[0]
    _, scale = gf.guided(tab, None if sampler == DDPM else eta, zd[0].cpu().numpy(), x0, np.full(B, t0), np.zeros(shp), nz)
    within(z.cpu().numpy(), u.cpu().numpy().astype(np.float64), scale, "weight 0 against the unguided step")
    print(f"\n{c['expect']} / {c['site']} / KSN {c['ksn']} / slices {sl}: update {worst:.2e} of scale (bar {BAR_STEP:.0e})")


def test_one_slice_equals_three_slices():
    F, T, B, n = 181, 76, 24, 3
    sch, _, _ = sched("ddim20")
    x0, txt = cu(syn.normal(SEED, "gb/x", (B, F, 1, T))), cu(syn.normal(SEED, "gb/txt", (B, 512)))
    y, m, w = guide_np(B, F, T, "gb")
    for sampler in (DDPM, DDIM):
        outs = []
        for streams in (1, 3):
            eng = make(F, T, B, {"MST_STREAMS": streams, "MST_SMALL_M": 0, "MST_TAIL_NTB": 4})
            assert eng.loop_slices(B, False, T) == streams
            eng.set_text(txt)
            ga = G(x0, target=cu(y), mask=cu(m), weight=cu(w), follow_schedule=1)
            outs.append(eng.sample_loop(sch, x0.clone(), 19, 19 - n + 1, sampler, 0.5, seed=7, dump_xstart=True, guide=ga))
        torch.cuda.synchronize()
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("path", ["small", "large"])
def test_a_clip_does_not_depend_on_its_neighbours_targets_and_weights(path):
    F, T, B = 181, 76, 3
    eng = make(F, T, B, {"MST_SMALL_M": 0} if path == "large" else None)
    sch, _, _ = sched("ddim20")
    x, txt = syn.normal(SEED, "gn/x", (B, F, 1, T)), syn.normal(SEED, "gn/txt", (B, 512))
    eng.set_text(cu(txt))
    for sampler in (DDPM, DDIM):
        res = []
        for k in (0, 1):
            y, m, w = guide_np(B, F, T, f"gn{k}")
            y1, m1, _ = guide_np(B, F, T, "gn")
            y[1], m[1], w[1] = y1[1], m1[1], 1.25
            ga = G(cu(x), target=cu(y), mask=cu(m), weight=cu(w))
            res.append(eng.sample_loop(sch, cu(x), 19, 17, sampler, 0.0, seed=3, guide=ga))
        torch.cuda.synchronize()
        assert torch.equal(res[0][1], res[1][1]) and not torch.equal(res[0][2], res[1][2])


@pytest.mark.parametrize("sampler,eta", [(DDPM, 0.0), (DDIM, 0.5)], ids=["ddpm", "ddim.5"])
def test_gradient_kind_fed_with_the_target_guides_tensor_equals_the_target_kind(sampler, eta):
    """One fused step: MST_GUIDE_GRADIENT with TargetGuide.__call__'s torch tensor against MST_GUIDE_TARGET computed in the kernel --
    the same x0-hat bit for bit, samples within 2e-5 of scale (the two gradients differ by fp32 rounding alone)."""
    from mst_amd.diffusion.guidance import TargetGuide
    F, T, B, t = 181, 76, 3, 12
    eng = make(F, T, B)
    sch, tab, tmap = sched("ddim20")
    full, _ = gf.tables("")
    x, txt, noise = syn.normal(SEED, "gk/x", (B, F, 1, T)), syn.normal(SEED, "gk/txt", (B, 512)), syn.normal(SEED, "gk/n", (1, B, F, 1, T))
    y, m, w = guide_np(B, F, T, "gk")
    eng.set_text(cu(txt))
    guide = TargetGuide(y, mask=m, weight=w, alphas_cumprod=full["alphas_cumprod"])
    grad = guide(cu(x), torch.full((B,), int(tmap[t]), device=dev()))
    a, da = eng.sample_loop(sch, cu(x), t, t, sampler, eta, noise=cu(noise), dump_xstart=True, guide=G(cu(x), grad=grad))
    b, db = eng.sample_loop(sch, cu(x), t, t, sampler, eta, noise=cu(noise), dump_xstart=True,
                            guide=G(cu(x), target=cu(y), mask=cu(m), weight=cu(w), follow_schedule=1))
    assert torch.equal(da, db)
    _, scale = gf.guided(tab, None if sampler == DDPM else eta, da[0].cpu().numpy(), x, np.full(B, t), grad.cpu().numpy(), noise[0])
    print(f"\ngradient kind vs target kind: {within(a.cpu().numpy(), b.cpu().numpy().astype(np.float64), scale, 'sample'):.2e} of scale")


# ------------------------------------------------------------------------------ 4. whole loops against the reference
def _plain_diffusion(resp="ddim20", mean="START_X"):
    from mst_amd.diffusion import gaussian_diffusion as gd
    from mst_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    return SpacedDiffusion(use_timesteps=space_timesteps(1000, resp), betas=gd.get_named_beta_schedule("cosine", 1000),
                           model_mean_type=gd.ModelMeanType[mean], model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE)


def _golden_guide():
    from mst_amd.diffusion.guidance import TargetGuide
    y, m = gf.guide_inputs("xia")
    return TargetGuide(y, mask=m, weight=gf.WEIGHT, alphas_cumprod=gf.tables("")[0]["alphas_cumprod"])


@pytest.mark.parametrize("smp", ["ddim", "ddpm"])
def test_whole_20_step_guided_loops_vs_the_reference(smp, monkeypatch):
    """20 steps under "ddim20" from the golden's noise: natively with a TargetGuide (one native call: counted), and with the same guide
    behind a lambda (a gradient per step, one step per engine call).  Bar: 1.5 x this engine's own unguided error against the
    reference's unguided loop from the same noise, computed here -- the guide term is fp32 elementwise and adds no 16-bit operand; the
    factor allows for the moved trajectory -- and in any case below the project's 1e-3 loop bar."""
    from mst_amd.engine import DenoiserEngine
    from test_gpu_boundary import PROMPTS, build, recorded_noise
    m = build()["m"]
    d = _plain_diffusion()
    g = gf.golden()
    noise = cu(gf.loop_noise())
    T = noise.shape[-1]
    assert gf.PROMPT == PROMPTS[0]
    y = {"y": {"text": [gf.PROMPT], "mask": torch.ones(1, 1, 1, T, device=dev())}}
    guide = _golden_guide()
    calls = []
    orig = DenoiserEngine.sample_loop
    monkeypatch.setattr(DenoiserEngine, "sample_loop", lambda self, *a, **k: (calls.append(k.get("guide")), orig(self, *a, **k))[1])

    def run(cond_fn):
        calls.clear()
        with recorded_noise(f"guided/xia/{smp}"):
            if smp == "ddim":
                return d.ddim_sample_loop(m, tuple(noise.shape), noise=noise, clip_denoised=False, cond_fn=cond_fn, model_kwargs=y, eta=0.0)
            return d.p_sample_loop(m, tuple(noise.shape), noise=noise, clip_denoised=False, cond_fn=cond_fn, model_kwargs=y)

    e_plain = rel_l2(run(None).cpu().numpy(), g[f"xia|loop20|{smp}|plain"])
    native = run(guide)
    assert len(calls) == 1 and calls[0] is not None, "a TargetGuide loop is one native call"
    e_native = rel_l2(native.cpu().numpy(), g[f"xia|loop20|{smp}|guided"])
    stepwise = run(lambda x, t, **kw: guide(x, t, **kw))
    assert len(calls) == 20 and all(c is not None for c in calls)
    e_step = rel_l2(stepwise.cpu().numpy(), g[f"xia|loop20|{smp}|guided"])
    moved = rel_l2(native.cpu().numpy(), g[f"xia|loop20|{smp}|plain"])
    print(f"\n20-step {smp} loops vs the reference: unguided {e_plain:.3e}; guided native {e_native:.3e}, step by step {e_step:.3e} "
          f"(bar 1.5 x unguided = {1.5 * e_plain:.3e}, and 1e-3); guided vs the reference's UNGUIDED loop {moved:.3f}")
    assert moved >= 0.9 * gf.MOVED
    for e in (e_native, e_step):
        assert e <= 1.5 * e_plain and e < 1e-3, (e, e_plain)


def test_loop_entries_of_the_mirror_with_a_guide():
    """ddim_sample_loop, its progressive generator and ddim_sample_loop_from with a TargetGuide agree bit for bit; the progressive
    p_sample loop yields the unguided x0-hat and every sample is the float64 guided update of it; InpaintingGaussianDiffusion + CFG
    wrapper runs; a mismatched alphas_cumprod table is refused at entry."""
    from mst_amd.diffusion.guidance import TargetGuide
    c, shp, y = _model()
    d, m = c["ddim"], c["m"]
    B, F, _, T = shp
    yt, mk, w = guide_np(B, F, T, "gm")
    full = gf.tables("")[0]["alphas_cumprod"]
    guide = TargetGuide(yt, mask=mk, weight=w + 0.5, alphas_cumprod=full)
    x0 = cu(syn.normal(SEED, "gm/x", shp))
    pair = {"y": {**y["y"], "inpainting_mask": cu(syn.root_horizontal_mask(B, F, T)), "inpainted_motion": cu(syn.normal(SEED, "gm/motion", shp))}}
    whole = d.ddim_sample_loop(m, shp, noise=x0, clip_denoised=False, cond_fn=guide, model_kwargs=pair, eta=0.0)
    prog = list(d.ddim_sample_loop_progressive(m, shp, noise=x0, clip_denoised=False, cond_fn=guide, model_kwargs=pair, eta=0.0))
    assert len(prog) == 20 and torch.equal(prog[-1]["sample"], whole)
    assert torch.equal(d.ddim_sample_loop_from(m, x0, 20, clip_denoised=False, cond_fn=guide, model_kwargs=pair), whole)
    plain = d.ddim_sample_loop(m, shp, noise=x0, clip_denoised=False, model_kwargs=pair, eta=0.0)
    assert not torch.equal(plain, whole)
    _, tab, _ = sched("ddim20")
    x = x0.cpu().numpy()
    for k, o in enumerate(prog[:4]):
        t = np.full(B, 19 - k)
        grad = gf.target_grad(tab, x, t, yt, mk, w + 0.5, 1)
        want, sc = gf.guided(tab, 0.0, o["pred_xstart"].cpu().numpy(), x, t, grad, None)
        within(o["sample"].cpu().numpy(), want, sc, f"generator step {k}")
        x = o["sample"].cpu().numpy()
    with pytest.raises(ValueError, match="ORIGINAL process"):
        d.ddim_sample_loop(m, shp, noise=x0, clip_denoised=False, cond_fn=TargetGuide(yt, alphas_cumprod=d.alphas_cumprod), model_kwargs=pair)


# ------------------------------------------------------------------------------ 5. denoised_fn
@pytest.mark.parametrize("ddim", [0, 1], ids=["p_sample", "ddim_sample"])
def test_denoised_fn(ddim):
    """An identity denoised_fn reproduces the fused step within 2e-5 of scale; clamp-to-+-0.5 against the float64 form applied to the
    clamped x0-hat; combined with a guide; through a loop (one step per call)."""
    c, shp, y = _model()
    d, m = c["ddim"], c["m"]
    B, F, _, T = shp
    _, tab, _ = sched("ddim20")
    x = cu(syn.normal(SEED, "gd/x", shp))
    mask, motion = cu(syn.root_horizontal_mask(B, F, T)), cu(syn.normal(SEED, "gd/motion", shp))
    kw = {"y": {**y["y"], "inpainting_mask": mask, "inpainted_motion": motion}}
    t = torch.tensor([11, 4], device=dev())[:B]
    eta = 0.5 if ddim else None
    step = (lambda **k: d.ddim_sample(m, x, t, clip_denoised=False, model_kwargs=kw, eta=0.5, **k)) if ddim else \
        (lambda **k: d.p_sample(m, x, t, clip_denoised=False, model_kwargs=kw, **k))

    def seeded(**k):
        torch.manual_seed(5)
        noise = torch.randn_like(x) * (1 - mask)
        torch.manual_seed(5)
        return step(**k), noise.cpu().numpy()

    plain, nz = seeded()
    ident, _ = seeded(denoised_fn=lambda v: v)
    xn, tn = x.cpu().numpy(), t.cpu().numpy()
    _, scale = gf.guided(tab, eta, plain["pred_xstart"].cpu().numpy(), xn, tn, np.zeros(shp), nz)
    within(ident["sample"].cpu().numpy(), plain["sample"].cpu().numpy().astype(np.float64), scale, "identity denoised_fn")
    assert torch.equal(ident["pred_xstart"], plain["pred_xstart"])
    clamp = lambda v: v.clamp(-0.5, 0.5)
    cl, _ = seeded(denoised_fn=clamp)
    p = cl["pred_xstart"].cpu().numpy()
    assert np.array_equal(p, np.clip(plain["pred_xstart"].cpu().numpy(), -0.5, 0.5)) and np.abs(p).max() == 0.5
    want, scale = gf.guided(tab, eta, p, xn, tn, np.zeros(shp), nz)
    within(cl["sample"].cpu().numpy(), want, scale, "clamp denoised_fn")
    yt, mk, w = guide_np(B, F, T, "gd")
    cond = lambda xx, tt, **k: cu(w + 0.5).view(-1, 1, 1, 1) * cu(mk) * (cu(yt) - xx)
    both, _ = seeded(denoised_fn=clamp, cond_fn=cond)
    assert torch.equal(both["pred_xstart"], cl["pred_xstart"])
    want, scale = gf.guided(tab, eta, p, xn, tn, gf.target_grad(tab, xn, tn, yt, mk, w + 0.5, 0), nz)
    within(both["sample"].cpu().numpy(), want, scale, "clamp denoised_fn + guide")
    loop = d.ddim_sample_loop if ddim else d.p_sample_loop
    out = loop(m, shp, noise=x, clip_denoised=False, denoised_fn=clamp, model_kwargs=kw, skip_timesteps=17)
    assert torch.isfinite(out).all() and float(out.abs().max()) <= 0.5             # index 0: the sample is the clamped x0-hat
    out2 = loop(m, shp, noise=x, clip_denoised=False, denoised_fn=clamp, cond_fn=cond, model_kwargs=kw, skip_timesteps=17)
    assert torch.isfinite(out2).all() and out2.shape == out.shape             # (the guided DDIM step moves pred' at index 0 too: no bound there)


# ------------------------------------------------------------------------------ 6. refusals
def test_refusals_name_their_reason():
    from mst_amd import _native as N
    from mst_amd.engine import SAMPLER_DDIM_REVERSE, SAMPLER_PLMS, Schedule
    F, T, B = 181, 76, 2
    eng = make(F, T, B)
    sch, tab, tmap = sched("ddim20")
    x = cu(syn.normal(SEED, "gr/x", (B, F, 1, T)))
    eng.set_text(cu(syn.normal(SEED, "gr/txt", (B, 512))))
    target = G(x, target=x, weight=1.0)
    with pytest.raises(RuntimeError, match="MST_GUIDE_GRADIENT carries the gradient of ONE step"):
        eng.sample_loop(sch, x.clone(), 5, 3, DDIM, seed=1, guide=G(x, grad=x))
    with pytest.raises(RuntimeError, match="MST_SAMPLER_DDIM_REVERSE takes no guide"):
        eng.sample_loop(sch, x.clone(), 3, 5, SAMPLER_DDIM_REVERSE, guide=target)
    with pytest.raises(RuntimeError, match="MST_SAMPLER_PLMS takes no guide"):
        eng.sample_loop(sch, x.clone(), 5, 3, SAMPLER_PLMS, guide=target)
    with pytest.raises(RuntimeError, match="needs target_dev"):
        eng.sample_loop(sch, x.clone(), 5, 3, DDIM, seed=1, guide=G(x, weight=1.0))
    with pytest.raises(RuntimeError, match="needs weight_dev"):
        eng.sample_loop(sch, x.clone(), 5, 3, DDIM, seed=1, guide=G(x, target=x))
    bad = G(x, target=x, weight=1.0)
    bad[0].kind = 7
    with pytest.raises(RuntimeError, match="bad guide kind 7"):
        eng.sample_loop(sch, x.clone(), 5, 3, DDIM, seed=1, guide=bad)
    empty = N.MstGuideArgs()
    empty.kind = 1
    with pytest.raises(RuntimeError, match="MST_GUIDE_GRADIENT needs grad_dev"):
        eng.sample_loop(sch, x.clone(), 5, 5, DDIM, seed=1, guide=(empty, []))
    # a schedule without the variance row (the C entry alone): the guided ancestral step is refused, the guided DDIM step runs
    table = np.ascontiguousarray(np.stack([np.asarray(tab[k] if k != "_log_variance" else tab["posterior_log_variance_clipped"], np.float64)
                                           .astype(np.float32) for k in mst_amd.engine.TABLE_ORDER]))
    tm = np.ascontiguousarray(np.asarray(tmap, np.int32))
    h = C.c_void_p()
    N.check(N.lib().mst_schedule_create(20, table.ctypes.data_as(C.c_void_p), tm.ctypes.data_as(C.c_void_p), 0, C.byref(h)))
    bare = Schedule.__new__(Schedule)
    bare.handle, bare.num_steps, bare.device = h, 20, dev()
    with pytest.raises(RuntimeError, match="needs the schedule's variance row: call mst_schedule_set_variance"):
        eng.sample_loop(bare, x.clone(), 5, 3, DDPM, seed=1, guide=target)
    t = torch.full((B,), 5, device=dev())
    with pytest.raises(RuntimeError, match="mst_step_epilogue_guided: a guided MST_SAMPLER_DDPM step needs the schedule's variance row"):
        bare.step_guided(x, x, t, x, target, sampler=DDPM)
    a = eng.sample_loop(bare, x.clone(), 5, 3, DDIM, seed=1, guide=target)
    b = eng.sample_loop(sch, x.clone(), 5, 3, DDIM, seed=1, guide=target)
    assert torch.equal(a, b)
    with pytest.raises(RuntimeError, match="mst_step_epilogue_guided: MST_SAMPLER_DDIM_REVERSE takes no guide"):
        sch.step_guided(x, x, t, x, target, sampler=SAMPLER_DDIM_REVERSE)
    # unguided entries are what they were: mst_sample_loop knows no guide
    c, shp, y = _model()
    with pytest.raises(NotImplementedError, match="guided PLMS is out of scope"):
        c["ddim"].plms_sample_loop(c["m"], shp, noise=cu(syn.normal(SEED, "gr/n", shp)), model_kwargs=y, cond_fn=lambda *a, **k: None)
