"""DDIM inversion on the GPU: SAMPLER_DDIM_REVERSE (reference gaussian_diffusion.py:910-946, x_t -> x_{t+1}) at every site that applies
the update, and the ascending loop around it.

  1. the stand-alone step kernel against the float64 closed form (tests/reverse_fixture.py), every index, every MEAN, blend, clamp;
  2. fused single steps against the reference's own outputs (tests/golden/reverse.npz);
  3. short ascending loops on every fused path -- the row id names the trunk path, the slice plan and the kernel site that applies the
     update, and the first assertions prove them from mirrors of the engine's launch rules (tests/test_gpu_noise.py's) --
       (a) every x_{j+1} recomputed in float64 from the engine's OWN x0-hat_j and x_j: the update arithmetic, exactly;
       (b) every x0-hat_j against the fp32 oracle forward at the engine's x_j: the forward, at the project's 1e-3;
     plus what must hold bit for bit: a k-step loop == k one-step loops, two runs, two seeds, a NaN-filled noise buffer;
  4. bitwise properties of the loop entries of the diffusion mirror, slicing, neighbours;
  5. refusals, each naming its reason;
  6. the round trip invert -> decode against the reference's;
  7. the recipe: invert once, decode under several styles as one mixed batch.

Why the bars look the way they do.  The update is a difference of large terms: an error e in x0-hat reaches the sample as g(t) e with
g(0) = 13.16 for ddim20 (reverse_fixture.g; tests/test_reverse_cpu.py pins the table).  So (a) measures the update against the engine's
own x0-hat elementwise, relative to the magnitudes of the products that are summed (reverse_fixture.closed_form's `scale`), at the
constant the existing stand-alone DDIM-step test uses (tests/test_gpu_parity.py::test_elementwise_kernels_vs_oracle: 2e-5), and (b)
holds the forward alone to 1e-3.  Against the reference's sample the bar is max(1, g(t)) * 1e-3; free-running over 20 steps g(0) * 1e-3."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
import mst_amd.synthetic as syn
import reverse_fixture as rf
from conftest import SEED, rel_l2
from oracle import denoiser

pytestmark = pytest.mark.gpu
BAR_STEP = 2e-5          # tests/test_gpu_parity.py: the stand-alone DDIM step's constant
TOL = 1e-3               # the project's bar for a forward
PE = syn.positional_table(5000, 512)


def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def REV():
    from mst_amd.engine import SAMPLER_DDIM_REVERSE
    return SAMPLER_DDIM_REVERSE


_W, _SCH = {}, {}


def weights(F):
    if F not in _W:
        _W[F] = syn.denoiser_state(SEED, F, layer_prefix="seqTransEncoder.layers.")      # the golden's weights (tests/test_gpu_parity.py)
    return _W[F]


def sched(resp):
    from mst_amd.engine import Schedule
    if resp not in _SCH:
        tab, tmap = rf.tables(resp)
        _SCH[resp] = (Schedule(tab, tmap, dev()), tab, np.asarray(tmap))
    return _SCH[resp]


def make(F, T, rows, env=None, precise=False):
    """An engine created under `env` (the MST_* switches are read at creation)."""
    from mst_amd.engine import DenoiserEngine
    env = {k: str(v) for k, v in (env or {}).items()}
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        eng = DenoiserEngine(F, T, rows, device=dev())
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    eng.load_state_dict({k: torch.from_numpy(v) for k, v in weights(F).items()}, layer_prefix="seqTransEncoder.layers.", pe=torch.from_numpy(PE))
    if precise:
        eng.set_precise(True)
    return eng


def within(got, want, scale, what):
    """|got - want| <= BAR_STEP * scale elementwise; prints and returns the worst ratio |got - want| / scale."""
    d = np.abs(np.asarray(got, dtype=np.float64) - want)
    r = float((d / np.maximum(scale, 1e-300)).max())
    assert r <= BAR_STEP, f"{what}: worst |dev| / scale {r:.3e} > {BAR_STEP:.0e} at {np.unravel_index(int((d / np.maximum(scale, 1e-300)).argmax()), d.shape)}"
    return r


# ------------------------------------------------------------------------------ 1. the stand-alone step
def _step_inputs(B, F, T):
    shp = (B, F, 1, T)
    m = np.zeros(shp, np.float32)
    m[:, ::3, :, : max(1, T // 2)] = 1
    return dict(mo=syn.normal(SEED, "rs/mo", shp), x=syn.normal(SEED, "rs/x", shp), mask=m, motion=syn.normal(SEED, "rs/motion", shp))


def _xstart64(tab, mean, mo, x, t, mask, motion, clamp):
    """float64 x0-hat of the step's front end (blend on the raw output, MEAN conversion on float32-rounded entries, clamp)."""
    out = np.asarray(mo, np.float64)
    if mask is not None:
        out = out * (1 - mask) + np.asarray(motion, np.float64) * mask
    f = lambda name: rf._bc(rf._f32(np.asarray(tab[name])[t]), x)
    if mean == 1:
        out = f("sqrt_recip_alphas_cumprod") * x - f("sqrt_recipm1_alphas_cumprod") * out
    if mean == 2:
        c1, c2 = f("posterior_mean_coef1"), f("posterior_mean_coef2")
        out = (1.0 / c1) * out - (c2 / c1) * x
    return np.clip(out, -1, 1) if clamp else out


STEP_T = {"ddim20": [list(range(0, 7)), list(range(7, 14)), list(range(14, 20)) + [19]], "": [[0, 1, 500, 999, 999, 1, 0]]}


@pytest.mark.parametrize("mean", [0, 1, 2], ids=["x_start", "epsilon", "previous_x"])
@pytest.mark.parametrize("resp", ["ddim20", ""], ids=["ddim20-every-index", "full-0-1-500-999"])
def test_standalone_step_equals_the_float64_closed_form(resp, mean):
    """Schedule.step(sampler=REVERSE): a different index per clip (7 clips a call, every index of ddim20; 0, 1, 500, 999 of the full
    schedule), blend on / off, clamp on / off, noise=None and a NaN noise tensor.  x0-hat is compared with the float64 front end, the
    sample with the closed form applied to the KERNEL's x0-hat (so a MEAN conversion's own cancellation is not charged to the update);
    at the last index the sample must equal eps."""
    sch, tab, _ = sched(resp)
    n = len(tab["alphas_cumprod"])
    B, F, T = 7, 24, 10                                           # 240 elements a clip: one partly filled 256-thread block (several blocks: the next test)
    v = _step_inputs(B, F, T)
    worst = 0.0
    for ts in STEP_T[resp]:
        t = np.asarray(ts)
        for blend in (False, True):
            for clamp in (False, True):
                mk, mot = (v["mask"], v["motion"]) if blend else (None, None)
                kw = dict(mask=None if mk is None else cu(mk), motion=None if mot is None else cu(mot), clip_denoised=clamp, mean_type=mean)
                s, p = sch.step(cu(v["mo"]), cu(v["x"]), cu(t), None, REV(), **kw)
                nan = torch.full_like(s, float("nan"))
                s2, p2 = sch.step(cu(v["mo"]), cu(v["x"]), cu(t), nan, REV(), mask_noise=True, **kw)
                assert torch.equal(s, s2) and torch.equal(p, p2)                       # the noise tensor and mask_noise are never read
                s, p = s.cpu().numpy(), p.cpu().numpy()
                assert np.isfinite(s).all()
                p64 = _xstart64(tab, mean, v["mo"], v["x"], t, mk, mot, clamp)
                if mean == 0:
                    assert np.array_equal(p, p64.astype(np.float32))                    # blend and clamp are exact in fp32
                else:                                                                   # two products: relative to their magnitudes
                    f = lambda name: rf._bc(rf._f32(np.asarray(tab[name])[t]), v["x"])
                    raw = np.abs(_xstart64(tab, 0, v["mo"], v["x"], t, mk, mot, False))  # the blended model output the conversion acts on
                    mag = (np.abs(f("sqrt_recip_alphas_cumprod") * v["x"]) + f("sqrt_recipm1_alphas_cumprod") * raw if mean == 1 else
                           (raw + np.abs(f("posterior_mean_coef2") * v["x"])) / f("posterior_mean_coef1"))
                    if not clamp:
                        within(p, p64, mag, f"x0-hat mean {mean} t {ts}")
                if clamp:
                    assert np.abs(p).max() <= 1.0
                if blend:
                    m = v["mask"].astype(bool)
                    if mean == 0 and not clamp:
                        assert np.array_equal(p[m], v["motion"][m])
                want, scale = rf.closed_form(tab, p, v["x"], t)
                worst = max(worst, within(s, want, scale, f"sample mean {mean} t {ts} blend {blend} clamp {clamp}"))
                last = t == n - 1
                if last.any():
                    eps = rf.eps_of(tab, p, v["x"], t)
                    within(s[last], eps[last], scale[last], "the last index: sample == eps")
    print(f"\nstand-alone reverse step '{resp}' mean {mean}: worst |kernel - closed form| / scale {worst:.2e} (bar {BAR_STEP:.0e})")


def test_standalone_step_more_than_one_block_per_clip():
    """per_clip = 263 * 196 = 51548 elements: 202 blocks of 256 threads per clip, three clips at three indices."""
    sch, tab, _ = sched("ddim20")
    B, F, T = 3, 263, 196
    v = _step_inputs(B, F, T)
    t = np.array([0, 11, 19])
    s, p = sch.step(cu(v["mo"]), cu(v["x"]), cu(t), None, REV(), mask=cu(v["mask"]), motion=cu(v["motion"]))
    want, scale = rf.closed_form(tab, p.cpu().numpy(), v["x"], t)
    r = within(s.cpu().numpy(), want, scale, "sample")
    assert np.array_equal(p.cpu().numpy(), rf.blend(v["mo"], v["mask"], v["motion"]).astype(np.float32))
    print(f"\nworst ratio {r:.2e}")


# ------------------------------------------------------------------------------ 2. fused single steps against the reference
@pytest.mark.parametrize("path", ["small", "large"])
@pytest.mark.parametrize("tag,resp", [("xia", ""), ("xia", "100"), ("xia", "ddim20"), ("hml", "ddim20")],
                         ids=["xia-full", "xia-100", "xia-ddim20", "hml-ddim20"])
def test_fused_single_steps_vs_the_reference(tag, resp, path):
    """One-step loops at index 0, an interior index and the last index, with and without the inpainting pair: x0-hat within 1e-3
    relative L2 of the reference's, the sample within max(1, g(t)) * 1e-3 (g from the tables: 13.16 at index 0 of ddim20)."""
    g = rf.golden()
    v = rf.golden_inputs(tag)
    F, T, st = v["F"], v["T"], rf.STRIDE[tag]
    eng = make(F, T, 2, env={"MST_SMALL_M": 0} if path == "large" else None)
    sch, tab, _ = sched(resp)
    eng.set_text(cu(v["txt"]))
    for t in rf.INDICES[resp]:
        for pair in (0, 1):
            kw = dict(mask=cu(v["mask"]), motion=cu(v["motion"])) if pair else {}
            s, d = eng.sample_loop(sch, cu(v["x"]), t, t, REV(), dump_xstart=True, **kw)
            s, p = s.cpu().numpy()[..., ::st], d[0].cpu().numpy()[..., ::st]
            ep = rel_l2(p, g[f"{tag}|{resp}|{t}|{pair}|pred_xstart"])
            es = rel_l2(s, g[f"{tag}|{resp}|{t}|{pair}|sample"])
            gt = float(rf.g(tab, t))
            print(f"\n{tag} '{resp}' {path} t={t} pair={pair}: x0-hat {ep:.2e} (bar {TOL:.0e}), sample {es:.2e} (bar {max(1.0, gt) * TOL:.2e}, g = {gt:.2f})")
            assert ep <= TOL, (t, pair, ep)
            assert es <= max(1.0, gt) * TOL, (t, pair, es, gt)
            if pair:
                assert np.array_equal(p[:, :3], v["motion"][:, :3, :, ::st])


# ------------------------------------------------------------------------------ 3. trajectories on the fused paths
from plan_mirror import SMALL_M, plain_path, slices  # noqa: E402
from test_gpu_noise import FAMILIES, TRUNK_FAMILIES, draw_site, mask_of  # noqa: E402

EMB, VEC, SCA, RSCA = "k_embed_out:embed-staged", "k_gemm_dma:finish-vector", "k_embed_out:finish-scalar", "k_gemm_dma:finish-scalar"


def embeds_next(F, T, cfg, precise, graph):
    """Mirror of mst_sample_loop's `fuse_embed` / embed_next_fits: does step j's output projection embed step j + 1 (k_embed_out<.., KSN>)?"""
    kin = (F + 31) // 32
    nbw = (F + 127) // 128
    if cfg or precise or graph or T % 4:
        return 0
    return kin if (kin, nbw) in ((5, 2), (6, 2), (9, 3)) else 0


def row(id, F, T, B, resp="ddim20", t0=0, n=3, cfg=False, mask=None, env=None, expect=None, site=None, nsl=1, ksn=0, **variant):
    return pytest.param(dict(F=F, T=T, B=B, resp=resp, t0=t0, n=n, cfg=cfg, mask=mask, env=env or {}, expect=expect, site=site,
                             nsl=nsl, ksn=ksn, **variant), id=id)


# Where the rows start.  Check (b) holds the FORWARD to the project's bar, which is stated for clips at the data's scale (DESIGN section 2:
# unit-variance inputs; what amplifies the f16 operands' rounding is precise mode's business).  The synthetic denoiser's x0-hat is
# independent of x (random weights), so one step from index 0 of ddim20 -- x_1 = 14.2 x_0 - 13.2 x0-hat, g(0) = 13.16 -- throws a
# unit-variance clip far beyond ten sigma, where no inversion of a trained model goes (there x0-hat ~ x at index 0 and eps is O(1)); the
# forward of THAT clip measured 1.10e-3 .. 1.33e-3 against the oracle on an MI355X (seven rows, every tile path; 4.2e-4 at step 0 of the
# same rows, update 2e-7 and all bitwise properties intact).  So loops that start at index 0 and go on use the full schedule
# (g(0) = 0.455, the same t + 1 lookup at index 0) and the ddim20 rows start at index 8 or run to the last index; ddim20's index 0 is
# held by 1. (every index), 2. (both tile paths, both shapes, against the reference), the mirror's 5-step loop from index 0 (check (a),
# k steps == generator) and the 20-step round trip.  The <= 16-frame row (every activation hi + lo) does start at index 0 of ddim20.
TRAJ = [
    row("small-launch-T76-B2-root-mask-full-from0-ksn6", 181, 76, 2, resp="", mask="root", expect="small-launch-ln-in-gemm", site=EMB, ksn=6),
    row("small-tile-T76-B9-to-the-last-index-ksn6", 181, 76, 9, t0=17, expect="small-tile", site=EMB, ksn=6),
    row("fused-large-T76-B2-ksn6-to-the-last-index", 181, 76, 2, t0=17, env={"MST_SMALL_M": 0}, expect="fused-large-tile", site=EMB, ksn=6),
    row("fused-large-T196-B2-hml-ksn9-root-mask-full-from0", 263, 196, 2, resp="", mask="root", env={"MST_SMALL_M": 0}, expect="fused-large-tile", site=EMB, ksn=9),
    row("scalar-T75-B3-F190-resp100-to-the-last-index", 190, 75, 3, resp="100", t0=97, mask="third", expect="small-launch-ln-in-gemm", site=SCA),
    row("scalar-large-T75-B3-F190-full-from0", 190, 75, 3, resp="", env={"MST_SMALL_M": 0}, expect="fused-large-tile", site=SCA),
    row("short-T5-B2-third-mask-hi-lo", 181, 5, 2, mask="third", expect="small-tile-hi-lo", site=SCA),
    row("cfg2.5-small-T76-B2-full-from0", 181, 76, 2, resp="", cfg=True, mask="root", n=2, expect="small-launch-ln-in-gemm", site=EMB),
    row("cfg2.5-large-T76-B2", 181, 76, 2, cfg=True, n=2, t0=18, env={"MST_SMALL_M": 0}, expect="fused-large-tile", site=EMB),
    row("slices-cfg2.5-T76-B12-3x4", 181, 76, 12, cfg=True, t0=8, n=2, env={"MST_STREAMS": 3}, expect="small-tile", site=EMB, nsl=3),
    row("slices-T76-B24-3x8-ksn6-root-mask-full-from0", 181, 76, 24, resp="", mask="root", n=2, env={"MST_STREAMS": 3}, expect="small-tile", site=EMB, nsl=3, ksn=6),
    row("styles-3slots-T76-B6", 181, 76, 6, mask="root", t0=8, n=2, expect="style", site=EMB, ksn=6, styles=3),
    row("precise-T76-B2-ring-finish-vector", 181, 76, 2, mask="root", n=2, expect="small-tile-hi-lo", site=VEC, precise=True),
    row("precise-T61-B2-F150-ring-finish-scalar", 150, 61, 2, n=2, t0=18, expect="small-tile-hi-lo", site=RSCA, precise=True),
    row("trunk-resident-T196-B10-hml-ksn9", 263, 196, 10, t0=8, n=2, mask="root", expect="fused-large-tile", site=EMB, ksn=9, trunk=True),
    row("graph-replay-T76-B2-5steps-to-the-last-index", 181, 76, 2, t0=15, n=5, mask="root", env={"MST_GRAPH": 1, "MST_GRAPH_STEPS": 2},
        expect="small-launch-ln-in-gemm", site=EMB, graph=True),
]


@pytest.mark.parametrize("c", TRAJ)
def test_ascending_loop_on_every_fused_path(c):
    F, T, B, cfg, env, n, t0 = c["F"], c["T"], c["B"], c["cfg"], c["env"], c["n"], c["t0"]
    styles, trunk, precise, graph = c.get("styles", 0), c.get("trunk", False), c.get("precise", False), c.get("graph", False)
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
        fwd1 = lambda s, x, t, txt: sf.oracle_forward(F, s, x, t, txt)
    else:
        eng = make(F, T, mult * B, env, precise)
        w = weights(F)
        fwd1 = None
    if trunk:
        eng.set_trunk_groups(True)
    assert eng.loop_slices(B, cfg, T) == len(sl)
    sch, tab, tmap = sched(c["resp"])
    nidx = len(tmap)
    assert 0 <= t0 and t0 + n - 1 <= nidx - 1
    shp = (B, F, 1, T)
    x0 = syn.normal(SEED, "rt/x", shp)
    txt = syn.normal(SEED, "rt/txt", (B, 512))
    scale = np.full(B, 2.5, np.float32) if cfg else None
    mask = motion = None
    if c["mask"]:
        mask, motion = mask_of(c["mask"], B, F, T), syn.normal(SEED, "rt/motion", shp)
    eng.set_text(cu(txt), cfg=cfg)
    if styles:
        eng.set_styles(st)
    kw = dict(cfg=cfg, scale=None if scale is None else cu(scale), mask=None if mask is None else cu(mask),
              motion=None if motion is None else cu(motion), dump_xstart=True)

    def loop(x, a, b, **extra):
        out = eng.sample_loop(sch, x.clone(), a, b, REV(), **kw, **extra)
        torch.cuda.synchronize()
        return out

    final, dump = loop(cu(x0), t0, t0 + n - 1, seed=1)
    assert torch.isfinite(final).all() and dump.shape[0] == n
    # -- bit for bit: two runs, two seeds, a NaN-filled noise buffer of the right size, mask_noise either way
    for extra in (dict(seed=1), dict(seed=2 + (5 << 32)), dict(noise=torch.full((n,) + shp, float("nan"), device=dev())), dict(seed=1, mask_noise=False)):
        f2, d2 = loop(cu(x0), t0, t0 + n - 1, **extra)
        assert torch.equal(final, f2) and torch.equal(dump, d2), extra.keys()
    # -- a k-step loop == k one-step loops (what the progressive generator runs), x0-hat dump entry j == executed step j
    x, inter = cu(x0), []
    for j in range(n):
        x, d1 = loop(x, t0 + j, t0 + j, seed=9)
        assert torch.equal(d1[0], dump[j]), f"x0-hat of step {j}: {int((d1[0] != dump[j]).sum())} elements differ"
        inter.append(x)
    assert torch.equal(x, final)
    if trunk:
        eng.trunk_check()
    # -- (a) the update, exactly: x_{j+1} from the engine's own x0-hat_j and x_j; (b) the forward: x0-hat_j against the oracle at x_j
    xs = [x0] + [v.cpu().numpy() for v in inter]
    worst_a, worst_b = 0.0, 0.0
    for j in range(n):
        t = np.full(B, t0 + j)
        p = dump[j].cpu().numpy()
        want, sc = rf.closed_form(tab, p, xs[j], t)
        worst_a = max(worst_a, within(xs[j + 1], want, sc, f"x at index {t0 + j + 1}"))
        if t0 + j == nidx - 1:
            within(xs[j + 1], rf.eps_of(tab, p, xs[j], t), sc, "the last index: sample == eps")
        tt = torch.from_numpy(tmap[t])
        xin = torch.from_numpy(xs[j])
        if styles:
            ref = np.zeros(shp, np.float32)
            for s in range(styles):
                rows = [i for i in range(B) if st[i] == s]
                ref[rows] = fwd1(s, xin[rows], tt[rows], torch.from_numpy(txt[rows])).numpy()
        elif cfg:
            ref = denoiser.cfg_forward(w, PE, xin, tt, torch.from_numpy(txt), torch.from_numpy(scale)).numpy()
        else:
            ref = denoiser.forward(w, PE, xin, tt, torch.from_numpy(txt)).numpy()
        if mask is not None:
            ref = rf.blend(ref, mask, motion).astype(np.float32)
            m = mask.astype(bool)
            assert np.array_equal(p[m], motion[m]), "masked entries of x0-hat must be the motion, bit for bit"
        e = rel_l2(p, ref)
        worst_b = max(worst_b, e)
        assert e <= TOL, f"x0-hat of step {j} (index {t0 + j}): {e:.3e} vs the oracle forward"
    # -- a loop that is one slice of plain kernels: the families a profiled run launches, and that run equals this one
    checked = False
    if len(sl) == 1 and not (styles or trunk or graph):
        eng.profile(True, 1)
        try:
            pf, pd = loop(cu(x0), t0, t0 + n - 1, seed=1)
            fams = {k for k, v in eng.profile_read().items() if v[1]}
        finally:
            eng.profile(False)
        assert torch.equal(final, pf) and torch.equal(dump, pd)                          # (instrumented steps keep the embedding a launch of its own)
        assert FAMILIES[c["expect"]] | {"embed_out_step"} <= fams and not fams & (TRUNK_FAMILIES - FAMILIES[c["expect"]]), fams
        checked = True
    if trunk:
        eng.set_trunk_groups(False)
    print(f"\n{c['expect']} / {c['site']} / KSN {c['ksn']} / slices {sl}: update {worst_a:.2e} of scale (bar {BAR_STEP:.0e}), "
          f"x0-hat vs oracle {worst_b:.2e} (bar {TOL:.0e})" + (" / families confirmed by a profiled run" if checked else ""))


# ------------------------------------------------------------------------------ 4. bitwise properties
def test_one_slice_equals_three_slices():
    """MST_STREAMS 1 against 3 on the large-tile path at a fixed tile height (the slice plan otherwise picks the layer tail's): what
    differs is the slicing the reverse sampler is carried through -- element offsets, the slice's first clip, per-slice chaining."""
    F, T, B, n = 181, 76, 24, 3
    sch, _, _ = sched("ddim20")
    x0, txt = cu(syn.normal(SEED, "rb/x", (B, F, 1, T))), cu(syn.normal(SEED, "rb/txt", (B, 512)))
    mask, motion = cu(syn.root_horizontal_mask(B, F, T)), cu(syn.normal(SEED, "rb/motion", (B, F, 1, T)))
    outs = []
    for streams in (1, 3):
        eng = make(F, T, B, {"MST_STREAMS": streams, "MST_SMALL_M": 0, "MST_TAIL_NTB": 4})
        assert eng.loop_slices(B, False, T) == streams
        eng.set_text(txt)
        outs.append(eng.sample_loop(sch, x0.clone(), 17, 19, REV(), mask=mask, motion=motion, dump_xstart=True))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("path", ["small", "large"])
def test_a_clip_does_not_depend_on_its_neighbours(path):
    F, T, B = 181, 76, 3
    eng = make(F, T, B, {"MST_SMALL_M": 0} if path == "large" else None)
    sch, _, _ = sched("ddim20")
    res = []
    for k in (0, 1):
        x = syn.normal(SEED, f"rn/x{k}", (B, F, 1, T))
        txt = syn.normal(SEED, f"rn/txt{k}", (B, 512))
        motion = syn.normal(SEED, f"rn/motion{k}", (B, F, 1, T))
        x[1], txt[1], motion[1] = syn.normal(SEED, "rn/x", (F, 1, T)), syn.normal(SEED, "rn/t", (512,)), syn.normal(SEED, "rn/m", (F, 1, T))
        eng.set_text(cu(txt))
        res.append(eng.sample_loop(sch, cu(x), 0, 2, REV(), mask=cu(syn.root_horizontal_mask(B, F, T)), motion=cu(motion)))
    torch.cuda.synchronize()
    assert torch.equal(res[0][1], res[1][1])
    assert not torch.equal(res[0][0], res[1][0])


def _model():
    from test_gpu_boundary import F, PROMPTS, T, build
    c = build()
    B = 2
    y = {"y": {"text": PROMPTS[:B], "mask": torch.ones(B, 1, 1, T, device=dev())}}
    return c, (B, F, 1, T), y


def test_loop_entries_of_the_mirror_agree_bit_for_bit():
    """ddim_reverse_sample_loop (one native call) == its progressive generator (a native call per index) == per-step calls of
    ddim_reverse_sample's kernels through the engine; torch's generator is left where it was (nothing is drawn); dump_all_xstart
    gives the progressive x0-hats; a CPU-only callable goes through per-step ddim_reverse_sample."""
    c, shp, y = _model()
    d, m = c["ddim"], c["m"]
    x0 = cu(syn.normal(SEED, "rm/x", shp))
    k = 5
    torch.manual_seed(3)
    before = torch.get_rng_state()
    whole = d.ddim_reverse_sample_loop(m, x0, num_steps=k, clip_denoised=False, model_kwargs=y)
    assert torch.equal(torch.get_rng_state(), before), "the reverse loop drew from torch's generator"
    prog = list(d.ddim_reverse_sample_loop_progressive(m, x0, num_steps=k, clip_denoised=False, model_kwargs=y))
    assert len(prog) == k and all(o["sample"] is not None for o in prog)
    assert torch.equal(prog[-1]["sample"], whole)
    dump = d.ddim_reverse_sample_loop(m, x0, num_steps=k, clip_denoised=False, model_kwargs=y, dump_all_xstart=True)
    assert len(dump) == k and all(torch.equal(a, o["pred_xstart"]) for a, o in zip(dump, prog))
    assert torch.equal(x0, cu(syn.normal(SEED, "rm/x", shp))), "the caller's clip was modified"
    # every intermediate of the generator: the float64 update from its own x0-hat, to the step's bar
    _, tab, _ = sched("ddim20")
    x = x0.cpu().numpy()
    for j, o in enumerate(prog):
        want, sc = rf.closed_form(tab, o["pred_xstart"].cpu().numpy(), x, np.full(shp[0], j))
        within(o["sample"].cpu().numpy(), want, sc, f"generator step {j}")
        x = o["sample"].cpu().numpy()
    # the model as a plain callable: per-step ddim_reverse_sample (model call + the stand-alone kernel)
    plain = lambda xx, tt, **kw: m(xx, tt, **kw)
    img = x0
    for j in range(2):
        r = d.ddim_reverse_sample(plain, img, torch.full((shp[0],), j, device=dev()), clip_denoised=False, model_kwargs=y)
        want, sc = rf.closed_form(tab, r["pred_xstart"].cpu().numpy(), img.cpu().numpy(), np.full(shp[0], j))
        within(r["sample"].cpu().numpy(), want, sc, f"per-step call {j}")
        assert rel_l2(r["pred_xstart"].cpu().numpy(), prog[j]["pred_xstart"].cpu().numpy()) < TOL
        img = r["sample"]
    two = d.ddim_reverse_sample_loop(plain, x0, num_steps=2, clip_denoised=False, model_kwargs=y, device=dev())
    assert torch.equal(two, img)
    # full length by default
    assert len(list(d.ddim_reverse_sample_loop_progressive(m, x0, clip_denoised=False, model_kwargs=y))) == d.num_timesteps


# ------------------------------------------------------------------------------ 5. refusals
def test_refusals_name_their_reason():
    from mst_amd import _native as N
    from mst_amd.engine import SAMPLER_DDIM, SAMPLER_DDPM
    F, T, B = 181, 76, 2
    eng = make(F, T, B)
    sch, _, _ = sched("ddim20")
    eng.set_text(cu(syn.normal(SEED, "rr/txt", (B, 512))))
    x = cu(syn.normal(SEED, "rr/x", (B, F, 1, T)))
    keep = x.clone()
    with pytest.raises(RuntimeError, match="Reverse ODE only for deterministic path"):
        eng.sample_loop(sch, x, 0, 2, REV(), eta=0.5)
    with pytest.raises(RuntimeError, match="runs upward"):
        eng.sample_loop(sch, x, 2, 0, REV())
    with pytest.raises(RuntimeError, match=r"bad index range 18\.\.20 for 20 steps"):
        eng.sample_loop(sch, x, 18, 20, REV())
    with pytest.raises(RuntimeError, match="bad index range"):
        eng.sample_loop(sch, x, -1, 2, REV())
    with pytest.raises(RuntimeError, match="bad index range"):                           # the descending samplers still refuse an ascending range
        eng.sample_loop(sch, x, 0, 2, SAMPLER_DDIM)
    with pytest.raises(RuntimeError, match="bad sampler 3"):
        eng.sample_loop(sch, x, 0, 2, 3)
    torch.cuda.synchronize()
    assert torch.equal(x, keep), "a refused loop touched x"
    with pytest.raises(RuntimeError, match="Reverse ODE only for deterministic path"):
        sch.step(x, x, cu(np.array([0, 1])), None, REV(), eta=0.1)
    with pytest.raises(RuntimeError, match="bad sampler 3"):
        sch.step(x, x, cu(np.array([0, 1])), None, 3)
    g, t = torch.ones_like(x), cu(np.array([0, 1]))
    out = torch.empty_like(x)
    rc = N.lib().mst_step_backward(sch.handle, N.ptr(g), None, None, 0, N.ptr(t), B, x.numel() // B, REV(), C.c_float(0.0), None, N.ptr(out),
                                   N.stream_ptr(dev()))
    assert rc != 0
    msg = N.lib().mst_last_error().decode()
    assert "MST_SAMPLER_DDIM_REVERSE" in msg and "_with_grad" in msg, msg
    rc = N.lib().mst_step_backward(sch.handle, N.ptr(g), None, None, 0, N.ptr(t), B, x.numel() // B, SAMPLER_DDPM, C.c_float(0.0), None,
                                   N.ptr(out), N.stream_ptr(dev()))
    assert rc == 0                                                                       # ... and the samplers that have one still run
    torch.cuda.synchronize()
    c, shp, y = _model()
    with pytest.raises(AssertionError, match="Reverse ODE only for deterministic path"):
        c["ddim"].ddim_reverse_sample(c["m"], x, t, model_kwargs=y, eta=0.5)
    with pytest.raises(NotImplementedError, match="denoised_fn"):
        c["ddim"].ddim_reverse_sample(c["m"], x, t, model_kwargs=y, denoised_fn=lambda v: v)


# ------------------------------------------------------------------------------ 6. the round trip
def test_round_trip_against_the_reference():
    """The engine's full ddim20 inversion of the golden's content clip, decoded by ddim_sample_loop_from and by
    ddim_sample_loop(noise=latent): the two decodes agree bit for bit; latent and decoded clip against the reference's own round trip,
    free-running over 20 steps each, capped at g(0) * 1e-3 = 13.16e-3 (from the tables, not from a measurement).
    Measured on an MI355X: see docs/LAB_NOTES.md, "DDIM inversion"."""
    from mst_amd.diffusion import gaussian_diffusion as gd
    from mst_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    from test_gpu_boundary import PROMPTS, build
    m = build()["m"]
    d = SpacedDiffusion(use_timesteps=space_timesteps(1000, "ddim20"), betas=gd.get_named_beta_schedule("cosine", 1000),
                        model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE)
    g = rf.golden()
    x0 = cu(rf.golden_content())
    T = x0.shape[-1]
    y = {"y": {"text": [rf.PROMPT], "mask": torch.ones(1, 1, 1, T, device=dev())}}
    assert rf.PROMPT == PROMPTS[0]
    latent = d.ddim_reverse_sample_loop(m, x0, clip_denoised=False, model_kwargs=y)
    a = d.ddim_sample_loop_from(m, latent, 20, clip_denoised=False, model_kwargs=y)
    torch.manual_seed(1)
    b = d.ddim_sample_loop(m, tuple(x0.shape), noise=latent, clip_denoised=False, model_kwargs=y, eta=0.0)
    assert torch.equal(a, b)
    _, tab, _ = sched("ddim20")
    cap = float(rf.g(tab, 0)) * TOL
    el, ed = rel_l2(latent.cpu().numpy(), g["xia|inv20|latent"]), rel_l2(a.cpu().numpy(), g["xia|inv20|decoded"])
    back = rel_l2(a.cpu().numpy(), x0.cpu().numpy())
    print(f"\nround trip ddim20 x 20: latent vs reference {el:.3e}, decoded vs reference {ed:.3e} (cap {cap:.3e}); "
          f"decoded vs the content clip itself {back:.3e} (reference: {rel_l2(g['xia|inv20|decoded'], x0.cpu().numpy()):.3e})")
    assert el <= cap and ed <= cap
    # a partial inversion and its decode half: 7 up, 7 down, no q_sample and no draw in between
    part = d.ddim_reverse_sample_loop(m, x0, num_steps=7, clip_denoised=False, model_kwargs=y)
    dec = d.ddim_sample_loop_from(m, part, 7, clip_denoised=False, model_kwargs=y)
    assert torch.isfinite(dec).all() and dec.shape == x0.shape
    eng = m.mst_engine(1, T)
    m.mst_prepare(eng, y["y"], False)
    from mst_amd.engine import SAMPLER_DDIM
    mine = eng.sample_loop(d._schedule(dev()), part.clone(), 6, 0, SAMPLER_DDIM, seed=0)
    assert torch.equal(dec, mine), "ddim_sample_loop_from must start from x_t as it is"


# ------------------------------------------------------------------------------ 7. the recipe
def test_invert_once_decode_under_three_styles_as_one_batch():
    """INTEGRATION.md's recipe: invert 2 content clips under slot 0, repeat the latents 3 times, decode as ONE 6-clip batch with
    y['style']; each style's clips equal, bit for bit, that style's own single-style decode of the same latents.  Also under
    ClassifierFreeSampleModel."""
    from mst_amd.diffusion import gaussian_diffusion as gd
    from mst_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    from mst_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from test_gpu_style_bank import K, SHAPES, _bank
    F, T = SHAPES["xia"]
    bank, _ = _bank("xia")
    assert K == 3
    d = SpacedDiffusion(use_timesteps=space_timesteps(1000, "ddim20"), betas=gd.get_named_beta_schedule("cosine", 1000),
                        model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE)
    B = 2
    content = cu(syn.normal(SEED, "rc/content", (B, F, 1, T)))
    txt = cu(syn.normal(SEED, "rc/txt", (B, 512)))
    for model, extra in ((bank, {}), (ClassifierFreeSampleModel(bank), {"scale": cu(np.full(B, 2.5, np.float32))})):
        yi = {"y": {"text_embed": txt, "style": torch.zeros(B, dtype=torch.long), **extra}}
        latents = d.ddim_reverse_sample_loop(model, content, num_steps=8, clip_denoised=False, model_kwargs=yi)
        rep = lambda v: v.repeat(K, *([1] * (v.dim() - 1)))
        style = torch.arange(K).repeat_interleave(B)
        y6 = {"y": {"text_embed": rep(txt), "style": style, **{k: rep(v) for k, v in extra.items()}}}
        mixed = d.ddim_sample_loop_from(model, rep(latents), 8, clip_denoised=False, model_kwargs=y6)
        assert mixed.shape[0] == K * B and torch.isfinite(mixed).all()
        for s in range(K):
            ys = {"y": {**y6["y"], "style": torch.full((K * B,), s)}}
            alone = d.ddim_sample_loop_from(model, rep(latents), 8, clip_denoised=False, model_kwargs=ys)
            rows = (style == s).nonzero().flatten().tolist()
            assert torch.equal(mixed[rows], alone[rows]), s
        assert not torch.equal(mixed[0:B], mixed[B:2 * B])                                # the styles do differ
