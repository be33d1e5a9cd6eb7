"""Stochastic and guided windowed sampling on the GPU (k_window_noise in csrc/mst_window.h, mst_window_noise, mst_window_sample_loop,
windows.noise_windows, GaussianDiffusion.sample_loop_windows / p_sample_loop_windows).

The noise of a windowed loop is drawn in LONG-clip coordinates: entry j of the buffer is unfold(philox_normal(C, L, seed, step0 + j)),
bit for bit, so windows that share a long frame hold the same number for it, x_{t-1} stays linear in (x_t, x0-hat, noise) and the stitch
stays exact bookkeeping.  The loops are held, bit for bit, to the same loop driven step by step from Python (noise_windows for the
step, ONE one-step DenoiserEngine.sample_loop call on the windows, windows.stitch_): the same kernels on the same operands in the same
order.  Fixtures are those of tests/test_gpu_windows.py: the seeded Xia model (181 features), ddim20, skip_timesteps=12 (indices 7 .. 0)."""
import ctypes as C

import numpy as np
import pytest
import torch

import guide_fixture as gf
import mst_amd  # noqa: F401
from mst_amd import synthetic as syn
from conftest import SEED, rel_l2
from test_gpu_noise import BAR_A
from test_gpu_reverse import within
from test_gpu_windows import F_XIA, SKIP, cu, dev, long_inputs, same_bits
import window_noise_fixture as nf

pytestmark = pytest.mark.gpu

GUARD = 4096
HI = 1 << 32
DDPM, DDIM = 0, 1


@pytest.fixture(scope="module")
def xia():
    import loop_fixture as lf
    return lf.build_model(dev())


@pytest.fixture
def philox(xia):
    _, d = xia
    d.noise_source = "philox"
    yield d
    d.noise_source = "torch"
    d.__dict__.pop("noise_chunk_bytes", None)


def long_normal(Cn, F, L, seed, step):
    """mst_philox_normal of Cn clips of L frames -> [Cn,F,1,L]: what DenoiserEngine.philox_normal calls, at any feature count."""
    from mst_amd import _native as N
    out = torch.empty((Cn, F, 1, L), dtype=torch.float32, device=dev())
    N.check(N.lib().mst_philox_normal(N.ptr(out), Cn, F, L, C.c_uint64(seed), C.c_uint32(step), N.stream_ptr(dev())))
    return out


# ------------------------------------------------------------------------------------------ 1. the noise definition
NOISE_CASES = [
    ("W16-O4", [9, 16, 17, 40], 40, 16, 4, F_XIA),
    ("W17-O5", [9, 16, 17, 40], 40, 17, 5, F_XIA),
    ("L41-not-a-multiple-of-4", [9, 16, 17, 41], 41, 16, 4, F_XIA),
    ("one-clip-of-4096-frames", [4096], 4096, 196, 48, 3),                 # quads beyond a window, more than one block
    ("window-longer-than-L", [5, 11], 11, 16, 4, 7),                        # padding from frame L on: no long element behind it
]


@pytest.mark.parametrize("case", NOISE_CASES, ids=[c[0] for c in NOISE_CASES])
def test_noise_is_the_unfolded_long_draw(case, xia):
    from mst_amd import _native as N
    from mst_amd.diffusion.windows import WindowPlan, noise_windows, unfold
    _, lens, L, W, O, F = case
    seed, step0, n = 1234 + 3 * HI, 2, 3
    plan = WindowPlan(lens, W, O, dev(), long_frames=L)
    Nw = plan.n_windows
    total = n * Nw * F * W
    buf = torch.full((total + GUARD,), float("nan"), dtype=torch.float32, device=dev())
    N.check(N.lib().mst_window_noise(plan.handle, F, C.c_uint64(seed), C.c_uint32(step0), n, N.ptr(buf), N.stream_ptr(dev())))
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[total:]).all())                             # nothing behind the buffer
    got = buf[:total].view(n, Nw, F, 1, W)
    assert not bool(torch.isnan(got).any())                                 # every element written
    assert same_bits(noise_windows(plan, F, seed, step0, n), got)
    live = torch.zeros((len(lens), 1, 1, L), device=dev())
    for c, ln in enumerate(lens):
        live[c, ..., :ln] = 1
    for j in range(n):
        z = long_normal(len(lens), F, L, seed, step0 + j)
        if F == F_XIA and j == 0:
            eng = xia[0].mst_engine(len(lens), W)
            assert same_bits(eng.philox_normal(len(lens), L, seed, step0), z)
        assert same_bits(got[j], unfold((z * live).contiguous(), plan)), j
        for k in range(Nw):                                                 # exact zeros from the clip's length on
            pad = int(plan.win_lengths[k])
            assert not got[j, k, :, 0, pad:].any() and bool((got[j, k, :, 0, :pad] != 0).all())
    shared = 0
    for c in range(len(lens)):                                              # neighbours hold identical bits on shared frames
        for k in range(plan.clip_win0[c], plan.clip_win0[c + 1] - 1):
            dlt = int(plan.win_start[k + 1] - plan.win_start[k])
            assert same_bits(got[:, k, :, 0, dlt:], got[:, k + 1, :, 0, :W - dlt]), (c, k)
            shared += W - dlt
    assert shared > 0 or Nw == len(lens)
    assert not same_bits(got[0], got[1])                                    # another step, other numbers
    if total <= 1 << 20:                                                    # ... and the float64 statement, every value
        want = nf.window_noise(lens, W, O, F, L, seed, step0, n)
        dmax = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
        print(f"\nwindow noise vs the float64 statement {case[0]}: max |dev| {dmax:.3e} (bar {BAR_A:.1e})")
        assert dmax <= BAR_A


# ------------------------------------------------------------------------------------------ the loop driven from Python
def guide_long(lens, L, tag):
    """A TargetGuide on LONG operands: target, a mask mixed inside rows (zero past each clip), one weight per clip, the schedule's a_t."""
    from mst_amd.diffusion.guidance import TargetGuide
    Cn = len(lens)
    shp = (Cn, F_XIA, 1, L)
    m = (syn.uniform(SEED, f"wg/{tag}/m", shp, 0.0, 1.0) < 0.4).astype(np.float32)
    for c, n in enumerate(lens):
        m[c, ..., n:] = 0
    y = (3.0 * syn.normal(SEED, f"wg/{tag}/y", shp)).astype(np.float32)
    w = np.linspace(1.0, 4.0, Cn).astype(np.float32)
    return TargetGuide(cu(y), mask=cu(m), weight=cu(w), alphas_cumprod=gf.tables("")[0]["alphas_cumprod"])


def stepwise(d, model, plan, noise, init, kw, sampler, eta=0.0, seed=0, one_step_chunks=False, guide=None, dump=False,
             gradient_kind=None):
    """The windowed loop driven from Python -> (long, windows, [folded x0-hat per step]).  Noise of step k: the native loop's chunk
    c0 reads noise_windows(seed + c0, step 0 ..), so one chunk is (seed, step k) and chunks of one step are (seed + k, step 0).
    gradient_kind: a callable -- every step is ALSO taken, from the same windows, with MST_GUIDE_GRADIENT on the unfolded gradient of
    that callable on the folded long clip, and held to the target-kind step at tests/test_gpu_guided.py's bar (2e-5 of scale)."""
    from mst_amd.diffusion.gaussian_diffusion import _unwrap
    from mst_amd.diffusion.windows import fold, noise_windows, stitch_, unfold
    from mst_amd.engine import guide_args
    denoiser, cfg, _ = _unwrap(model)
    y = dict(kw["y"])
    idx = list(range(d.num_timesteps - SKIP))[::-1]
    t = torch.full((noise.shape[0],), idx[0], device=dev(), dtype=torch.long)
    x = unfold(d.q_sample(init, t, noise, model_kwargs=kw).contiguous(), plan)
    mask, motion = unfold(y["inpainting_mask"], plan), unfold(y["inpainted_motion"], plan)
    wc = plan.win_clip_tensor()
    yw = {"text": [y["text"][int(c)] for c in plan.win_clip]}
    for k in ("scale", "style"):
        if k in y:
            yw[k] = y[k][wc.to(y[k].device)]
    eng = denoiser.mst_engine(plan.n_windows * (2 if cfg is not None else 1), plan.window)
    denoiser.mst_prepare(eng, yw, cfg is not None)
    sch = d._schedule(dev())
    noisy = sampler == DDPM or eta != 0.0
    ga = None
    if guide is not None:
        ga = guide_args(x, target=unfold(guide.target.expand(noise.shape).contiguous(), plan),
                        mask=unfold(guide.mask.expand(noise.shape).contiguous(), plan), weight=guide.weight[wc], follow_schedule=True)
    dumps, worst = [], 0.0
    for k, i in enumerate(idx):
        nz = noise_windows(plan, F_XIA, seed + k, 0, 1)[0] if noisy and one_step_chunks else \
            noise_windows(plan, F_XIA, seed, k, 1)[0] if noisy else None
        call = lambda xx, g: eng.sample_loop(sch, xx, i, i, sampler, eta, cfg=cfg is not None, scale=yw.get("scale") if cfg is not None else None,
                                             mask=mask, motion=motion, mask_noise=True, clip_denoised=False, noise=nz, seed=0,
                                             dump_xstart=True, guide=g)
        if gradient_kind is not None:
            tl = torch.full((plan.n_clips,), i, device=dev(), dtype=torch.long)
            grad = unfold(d._cond_gradient(gradient_kind, fold(x, plan), tl, kw).contiguous(), plan)
            before = x.clone()
            a, da = call(x.clone(), guide_args(x, grad=grad))
        res = call(x, ga)
        if gradient_kind is not None:
            assert torch.equal(da, res[1])                                  # the same unguided x0-hat, bit for bit
            nzm = None if nz is None else (nz * (1 - mask)).cpu().numpy()
            _, scale = gf.guided(gf.tables("ddim20")[0], None if sampler == DDPM else eta, da[0].cpu().numpy(), before.cpu().numpy(),
                                 np.full(plan.n_windows, i), grad.cpu().numpy(), nzm)
            worst = max(worst, within(a.cpu().numpy(), x.cpu().numpy().astype(np.float64), scale, f"step {k}: gradient kind against target kind"))
        if dump:
            dumps.append(fold(res[1][0], plan))
        stitch_(x, plan)
    if gradient_kind is not None:
        print(f"\nper step, gradient kind on the long clip's gradient vs target kind: worst {worst:.2e} of scale (bar {gf.BAR_STEP:.0e})")
    return fold(x, plan), x, dumps


def loop_seed(ms):
    torch.manual_seed(ms)
    return int(torch.randint(0, 2 ** 31 - 1, (1,)).item())                  # the loop's only draw from torch


def check_agreement(plan, win, W):
    shared = 0
    for c in range(plan.n_clips):
        for k in range(plan.clip_win0[c], plan.clip_win0[c + 1] - 1):
            dlt = int(plan.win_start[k + 1] - plan.win_start[k])
            assert torch.equal(win[k, :, 0, dlt:], win[k + 1, :, 0, :W - dlt]), (c, k)
            shared += W - dlt
    assert shared > 0


LENS, L40 = [9, 16, 17, 40], 40


def run_case(d, model, plan, noise, init, kw, sampler, eta, ms=5, **extra):
    torch.manual_seed(ms)
    return d.sample_loop_windows(model, tuple(noise.shape), sampler="ddpm" if sampler == DDPM else "ddim", eta=eta, plan=plan,
                                 noise=noise, clip_denoised=False, model_kwargs=kw, skip_timesteps=SKIP, init_image=init, **extra)


# ------------------------------------------------------------------------------------------ 2. / 3. ancestral and stochastic DDIM
@pytest.mark.parametrize("sampler,eta,W,O", [(DDPM, 0.0, 16, 4), (DDPM, 0.0, 17, 5), (DDIM, 0.5, 17, 5)], ids=["ddpm-W16-O4", "ddpm-W17-O5", "ddim.5-W17-O5"])
def test_stochastic_loop_equals_stepwise(xia, philox, sampler, eta, W, O):
    """Lens 9, 16, 17, 40 in one batch: the native loop is the step-by-step loop bit for bit -- the long sample, the windows, the folded
    x0-hat of every step -- as one chunk and as chunks of one step (noise_chunk_bytes = 1: seed + c0, step 0); neighbours agree on shared
    frames; inpainted rows are the content's bits; zeros past a length; the free rows moved; another torch seed, another sample."""
    from mst_amd.diffusion.windows import WindowPlan
    model, d = xia
    noise, init, kw = long_inputs(f"s{sampler}{W}{O}", LENS, L40)
    plan = WindowPlan(LENS, W, O, dev(), long_frames=L40)
    seed = loop_seed(5)
    want_long, want_win, want_dump = stepwise(d, model, plan, noise, init, kw, sampler, eta, seed=seed, dump=True)
    if sampler == DDPM:                                                     # p_sample_loop_windows IS sample_loop_windows(sampler="ddpm")
        torch.manual_seed(5)
        got_long, got_win = d.p_sample_loop_windows(model, tuple(noise.shape), plan=plan, noise=noise, clip_denoised=False, model_kwargs=kw,
                                                    skip_timesteps=SKIP, init_image=init, return_windows=True)
    else:
        got_long, got_win = run_case(d, model, plan, noise, init, kw, sampler, eta, return_windows=True)
    assert torch.equal(got_win, want_win) and torch.equal(got_long, want_long)
    assert bool(torch.isfinite(got_long).all())
    check_agreement(plan, got_win, W)
    motion, mask = kw["y"]["inpainted_motion"], kw["y"]["inpainting_mask"]
    for c, n in enumerate(LENS):
        rows = mask[c, :, 0, 0] > 0
        assert int(rows.sum()) >= 1
        assert torch.equal(got_long[c, rows, 0, :n], motion[c, rows, 0, :n]), c
        assert not got_long[c, :, :, n:].any(), c
    assert not torch.equal(got_long[:, 5:], init[:, 5:])
    dump = run_case(d, model, plan, noise, init, kw, sampler, eta, dump_all_xstart=True)
    assert len(dump) == len(want_dump) == d.num_timesteps - SKIP
    for j, (a, b) in enumerate(zip(dump, want_dump)):
        assert a.shape == (len(LENS), F_XIA, 1, L40) and torch.equal(a, b), j
    # chunks of one step: seed + c0, step 0
    w1_long, w1_win, w1_dump = stepwise(d, model, plan, noise, init, kw, sampler, eta, seed=seed, one_step_chunks=True, dump=True)
    assert not torch.equal(w1_long, want_long)                              # other numbers from the second step on
    d.noise_chunk_bytes = 1
    try:
        c_dump, c_win = run_case(d, model, plan, noise, init, kw, sampler, eta, dump_all_xstart=True, return_windows=True)
    finally:
        d.__dict__.pop("noise_chunk_bytes", None)
    assert torch.equal(c_win, w1_win) and all(torch.equal(a, b) for a, b in zip(c_dump, w1_dump))
    other = run_case(d, model, plan, noise, init, kw, sampler, eta, ms=6)
    free = (mask == 0) & (kw["y"]["mask"].expand_as(mask))
    assert float((other != got_long)[free].float().mean()) > 0.99           # two torch seeds, two samples


# ------------------------------------------------------------------------------------------ 4. the deterministic subset
def test_deterministic_subset_is_ddim_sample_loop_windows(xia, philox):
    from mst_amd.diffusion.windows import WindowPlan
    model, d = xia
    noise, init, kw = long_inputs("det", LENS, L40)
    plan = WindowPlan(LENS, 17, 5, dev(), long_frames=L40)
    ref, ref_win = d.ddim_sample_loop_windows(model, tuple(noise.shape), plan=plan, noise=noise, clip_denoised=False, model_kwargs=kw,
                                              skip_timesteps=SKIP, init_image=init, return_windows=True)
    got, got_win = run_case(d, model, plan, noise, init, kw, DDIM, 0.0, return_windows=True)
    assert torch.equal(got, ref) and torch.equal(got_win, ref_win)
    dump = run_case(d, model, plan, noise, init, kw, DDIM, 0.0, dump_all_xstart=True)
    ref_dump = d.ddim_sample_loop_windows(model, tuple(noise.shape), plan=plan, noise=noise, clip_denoised=False, model_kwargs=kw,
                                          skip_timesteps=SKIP, init_image=init, dump_all_xstart=True)
    assert len(dump) == len(ref_dump) and all(torch.equal(a, b) for a, b in zip(dump, ref_dump))


# ------------------------------------------------------------------------------------------ 5. single full windows
def test_single_full_windows_equal_p_sample_loop(xia):
    """Lens 16, 16, 16 at W = L = 16, torch noise source: the long draw per step IS the plain loop's draw, the unfold is the identity,
    and both loops read the same buffer noise through the same step kernel: bit for bit."""
    model, d = xia
    assert d.noise_source == "torch"
    lens, W = [16, 16, 16], 16
    noise, init, kw = long_inputs("single", lens, W)
    shape = (len(lens), F_XIA, 1, W)
    torch.manual_seed(3)
    got = d.p_sample_loop_windows(model, None, window=W, overlap=4, lengths=lens, noise=noise, clip_denoised=False, model_kwargs=kw,
                                  skip_timesteps=SKIP, init_image=init)
    torch.manual_seed(3)
    ref = d.p_sample_loop(model, shape, noise=noise, clip_denoised=False, model_kwargs=kw, skip_timesteps=SKIP, init_image=init)
    assert got.shape == ref.shape and torch.equal(got, ref)
    torch.manual_seed(3)
    got = d.sample_loop_windows(model, None, sampler="ddim", eta=0.5, window=W, overlap=4, lengths=lens, noise=noise, clip_denoised=False,
                                model_kwargs=kw, skip_timesteps=SKIP, init_image=init)
    torch.manual_seed(3)
    ref = d.ddim_sample_loop(model, shape, noise=noise, clip_denoised=False, model_kwargs=kw, skip_timesteps=SKIP, init_image=init, eta=0.5)
    assert torch.equal(got, ref)
    torch.manual_seed(4)
    assert not torch.equal(d.p_sample_loop_windows(model, None, window=W, overlap=4, lengths=lens, noise=noise, clip_denoised=False,
                                                   model_kwargs=kw, skip_timesteps=SKIP, init_image=init), got)


# ------------------------------------------------------------------------------------------ 6. guided
@pytest.mark.parametrize("sampler,eta", [(DDPM, 0.0), (DDIM, 0.0), (DDIM, 0.5)], ids=["ddpm", "ddim0", "ddim.5"])
def test_guided_loops(xia, philox, monkeypatch, sampler, eta):
    """A TargetGuide on long operands (target, mask, per-clip weight, alphas_cumprod): the native windowed loop (MST_GUIDE_TARGET, one
    native call) equals, bit for bit, the Python-driven loop of one-step sample_loop calls with guide_args on the unfolded operands and
    stitch_ between them.

    The same guide behind a plain lambda takes the callable path: folded long clip -> cond_fn -> unfolded gradient -> one
    MST_GUIDE_GRADIENT step.  Two statements:
      per step   from the SAME windows, the gradient-kind step (the long clip's gradient, unfolded) against the target-kind step: the
                 same x0-hat bit for bit and the sample within 2e-5 of scale, the bar tests/test_gpu_guided.py applies to gradient kind
                 against target kind -- multiple 1 (asserted inside `stepwise`, every step, the figure printed);
      chained    the whole callable-path loop (8 steps) against the native one on the same noise (chunks of one step, as the callable
                 path runs): relative L2 of the long sample at most 1e-3, which is
                 50 x 2e-5.  Why a multiple, and why in L2: from the second step on the two loops evaluate the MODEL on inputs that
                 differ by an fp32 rounding; the model rounds its operands to 16 bits, so a few of them land on the other side of a
                 rounding boundary and x0-hat moves by 16-bit roundings, not fp32 ones, spread over the clip's tokens by attention.
                 No elementwise fp32 bar survives that; 1e-3 relative L2 is the project's own bar for two evaluations of this
                 model (tests/test_gpu_guided.py's loop bar, TOL of tests/test_gpu_reverse.py).  The measured figure is printed.
    Measured on an MI355X: per step at most 1.9e-7 of scale; chained 2.8e-4 relative L2 for all three samplers.
    The guide acts: the guided sample differs from the unguided one and lies closer to the target on the guide's masked, free entries."""
    from mst_amd.diffusion.windows import WindowPlan
    from mst_amd.engine import DenoiserEngine
    model, d = xia
    W, O = 17, 5
    noise, init, kw = long_inputs(f"g{sampler}{eta}", LENS, L40)
    plan = WindowPlan(LENS, W, O, dev(), long_frames=L40)
    guide = guide_long(LENS, L40, "a")
    fn = lambda x, t, **k: guide(x, t, **k)
    seed = loop_seed(5)
    want_long, want_win, want_dump = stepwise(d, model, plan, noise, init, kw, sampler, eta, seed=seed, guide=guide, dump=True, gradient_kind=fn)
    calls = []
    orig = DenoiserEngine.window_sample_loop
    monkeypatch.setattr(DenoiserEngine, "window_sample_loop", lambda self, *a, **k: (calls.append(k.get("guide")), orig(self, *a, **k))[1])
    got_long, got_win = run_case(d, model, plan, noise, init, kw, sampler, eta, cond_fn=guide, return_windows=True)
    assert len(calls) == 1 and calls[0] is not None and calls[0][0].kind == 2, "a TargetGuide loop is one native call"
    calls.clear()
    by_fn = run_case(d, model, plan, noise, init, kw, sampler, eta, cond_fn=fn)
    assert len(calls) == d.num_timesteps - SKIP and all(c is not None and c[0].kind == 1 for c in calls)
    assert torch.equal(got_win, want_win) and torch.equal(got_long, want_long)
    check_agreement(plan, got_win, W)
    dump = run_case(d, model, plan, noise, init, kw, sampler, eta, cond_fn=guide, dump_all_xstart=True)
    assert all(torch.equal(a, b) for a, b in zip(dump, want_dump))
    d.noise_chunk_bytes = 1                 # the callable path is one step a native call: its noise is chunk c0's, (seed + c0, step 0)
    try:
        native1 = run_case(d, model, plan, noise, init, kw, sampler, eta, cond_fn=guide)
    finally:
        d.__dict__.pop("noise_chunk_bytes", None)
    assert torch.equal(native1, got_long) == (sampler == DDIM and eta == 0.0)
    e = rel_l2(by_fn.cpu().numpy(), native1.cpu().numpy())
    print(f"\nguided windows, callable path against the native loop over {d.num_timesteps - SKIP} steps: relative L2 {e:.3e} (bar 1e-3)")
    assert e <= 1e-3
    plain = run_case(d, model, plan, noise, init, kw, sampler, eta)
    assert not torch.equal(plain, got_long)
    pick = (guide.mask > 0) & (kw["y"]["inpainting_mask"] == 0)
    assert int(pick.sum()) > 1000
    dist = lambda v: float((v - guide.target)[pick].abs().mean())
    print(f"mean |x - target| on the guide's free entries: guided {dist(got_long):.4f}, unguided {dist(plain):.4f}")
    assert dist(got_long) < dist(plain)
    for c, n in enumerate(LENS):
        assert not got_long[c, :, :, n:].any(), c


# ------------------------------------------------------------------------------------------ 7. CFG and a StyleBank
def test_ancestral_loop_under_cfg(xia, philox):
    from mst_amd.diffusion.windows import WindowPlan
    from mst_amd.model.cfg_sampler import ClassifierFreeSampleModel
    model, d = xia
    lens, L, W, O = [17, 40], 40, 17, 5
    noise, init, kw = long_inputs("scfg", lens, L)
    kw["y"]["scale"] = torch.tensor([2.5, 1.5], device=dev())
    cfg_model = ClassifierFreeSampleModel(model)
    plan = WindowPlan(lens, W, O, dev(), long_frames=L)
    want_long, want_win, _ = stepwise(d, cfg_model, plan, noise, init, kw, DDPM, seed=loop_seed(5))
    got_long, got_win = run_case(d, cfg_model, plan, noise, init, kw, DDPM, 0.0, return_windows=True)
    assert torch.equal(got_win, want_win) and torch.equal(got_long, want_long)
    assert not torch.equal(run_case(d, model, plan, noise, init, kw, DDPM, 0.0), got_long)       # the guidance did act


def test_ancestral_loop_with_a_style_bank():
    import style_fixture as sf
    from mst_amd.diffusion.windows import WindowPlan
    from mst_amd.model.mdm_forstyledataset import StyleDiffusion
    from mst_amd.model.style_bank import StyleBank
    from mst_amd.utils import model_util
    import loop_fixture as lf
    members = []
    for s in range(2):
        m = StyleDiffusion("", F_XIA, 1, 1, True, "rot6d", True, True, latent_dim=512, ff_size=1024, num_layers=8, num_heads=4,
                           dropout=0.1, activation="gelu", data_rep="hml_vec", cond_mode="text", cond_mask_prob=0.1,
                           arch="trans_enc", dataset="stylexia_posrot")
        missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in sf.style_weights(F_XIA, s).items()}, strict=False)
        assert not unexpected
        m.motion_enc.mdm_model.set_text_encoder(
            lambda texts: torch.stack([torch.from_numpy(syn.normal(SEED, "text/" + t, (512,))) for t in texts]))
        members.append(m.to(dev()).eval())
    bank = StyleBank(members)
    _, d, _ = model_util.creat_serval_diffusion(lf.diffusion_args(), StyleDiffusion, "ddim20")
    d.noise_source = "philox"
    lens, L, W, O = [20, 45], 45, 20, 5                                     # (the style-aware kernels take clips of 17 .. 207 frames)
    noise, init, kw = long_inputs("sbank", lens, L)
    plan = WindowPlan(lens, W, O, dev(), long_frames=L)
    res = {}
    for key, styles in (("mixed", [0, 1]), (1, [1, 1])):
        kw["y"]["style"] = torch.tensor(styles)
        res[key] = run_case(d, bank, plan, noise, init, kw, DDPM, 0.0)
    assert torch.equal(res["mixed"][1], res[1][1]) and not torch.equal(res["mixed"][0], res[1][0])
    kw["y"]["style"] = torch.tensor([0, 1])
    want_long, _, _ = stepwise(d, bank, plan, noise, init, kw, DDPM, seed=loop_seed(5))
    assert torch.equal(res["mixed"], want_long)


# ------------------------------------------------------------------------------------------ 8. refusals
def test_refusals(xia):
    """Each refusal by its message; every one is an argument check in front of any launch: x stays as it was."""
    from mst_amd import _native as N
    from mst_amd.diffusion.windows import WindowPlan, noise_windows
    model, d = xia
    lens, L, W, O = [9, 40], 40, 16, 4
    noise, init, kw = long_inputs("r", lens, L)
    plan = WindowPlan(lens, W, O, dev(), long_frames=L)
    call = lambda m=model, fn=d.sample_loop_windows, **k: fn(m, (2, F_XIA, 1, L), **{**dict(
        plan=plan, noise=noise, clip_denoised=False, model_kwargs=kw, skip_timesteps=SKIP, init_image=init), **k})
    keep = noise.clone()
    with pytest.raises(NotImplementedError, match="const_noise"):
        call(fn=d.p_sample_loop_windows, const_noise=True)
    with pytest.raises(ValueError, match="denoised_fn is not supported"):
        call(sampler="ddpm", denoised_fn=lambda x: x)
    with pytest.raises(ValueError, match="not the native denoiser"):
        call(m=lambda x, t, **k: x, sampler="ddpm")
    model.train()
    try:
        with pytest.raises(ValueError, match="training mode"):
            call(sampler="ddpm")
    finally:
        model.eval()
    with pytest.raises(ValueError, match="unknown sampler 'plms'"):
        call(sampler="plms")
    with pytest.raises(ValueError, match="window 224 is above the engine's limit of 223"):
        call(plan=None, window=224, overlap=8, sampler="ddpm")
    with pytest.raises(ValueError, match="the plan is for 2 clips of 40 frames"):
        d.p_sample_loop_windows(model, (2, F_XIA, 1, 39), plan=plan, noise=noise[..., :39], model_kwargs=kw)
    assert torch.equal(noise, keep)
    # the library's own (mst_window_sample_loop)
    eng = model.mst_engine(plan.n_windows, W)
    sch = d._schedule(dev())
    x = torch.zeros(plan.n_windows, F_XIA, 1, W, device=dev())
    buf = noise_windows(plan, F_XIA, 1, 0, 4)
    grad = torch.zeros_like(x)

    def native(batch=plan.n_windows, frames=W, sampler=DDIM, eta=0.0, noise_mode=1, noise_dev=None, guide=None, t_end=0):
        a = N.MstLoopArgs()
        a.batch, a.frames, a.sampler, a.eta, a.noise_mode, a.t_start, a.t_end = batch, frames, sampler, eta, noise_mode, 3, t_end
        a.x_dev = x.data_ptr()
        if noise_dev is not None:
            a.noise_dev = noise_dev.data_ptr()
        g = None
        if guide is not None:
            g = N.MstGuideArgs()
            g.kind, g.grad_dev = guide, grad.data_ptr()
        rc = N.lib().mst_window_sample_loop(eng.handle, sch.handle, C.byref(a), plan.handle, None if g is None else C.byref(g),
                                            N.stream_ptr(dev()))
        return rc, N.lib().mst_last_error().decode()
    for kwargs, what in ((dict(sampler=2), "sampler 2 is neither MST_SAMPLER_DDPM nor MST_SAMPLER_DDIM"),
                         (dict(sampler=3), "sampler 3 is neither MST_SAMPLER_DDPM nor MST_SAMPLER_DDIM"),
                         (dict(sampler=DDPM), "the in-kernel draw is keyed by window"),
                         (dict(eta=0.25), "fill a buffer with mst_window_noise"),
                         (dict(sampler=DDPM, noise_mode=0), "noise buffer missing"),
                         (dict(eta=0.25, noise_mode=0), "noise buffer missing"),
                         (dict(sampler=DDPM, noise_mode=0, noise_dev=buf, guide=1), "t_start 3 must equal t_end 0"),
                         (dict(guide=1), "t_start 3 must equal t_end 0"),
                         (dict(guide=7), "bad guide kind 7"),
                         (dict(batch=plan.n_windows - 1), "is not the plan's window count 4"),
                         (dict(frames=W - 1), "frames 15 is not the plan's window 16")):
        rc, msg = native(**kwargs)
        assert rc != 0 and msg.startswith("mst_window_sample_loop:") and what in msg, msg
    torch.cuda.synchronize()
    assert not x.any()                                                      # nothing ran


# ------------------------------------------------------------------------------------------ 9. no state left behind
def test_plain_loop_unchanged_around_a_windowed_one(xia, philox):
    model, d = xia
    T = 16
    noise, init, kw = long_inputs("sh", [16, 16], T)

    def plain():
        torch.manual_seed(9)
        return d.p_sample_loop(model, (2, F_XIA, 1, T), noise=noise, clip_denoised=False, model_kwargs=kw, skip_timesteps=SKIP, init_image=init)
    before = plain()
    lens, L = [9, 40], 40
    n2, i2, kw2 = long_inputs("sh2", lens, L)
    out = d.p_sample_loop_windows(model, (2, F_XIA, 1, L), window=16, overlap=4, lengths=lens, noise=n2, clip_denoised=False,
                                  model_kwargs=kw2, skip_timesteps=SKIP, init_image=i2)
    assert bool(torch.isfinite(out).all())
    guided = d.sample_loop_windows(model, (2, F_XIA, 1, L), sampler="ddim", eta=0.5, cond_fn=guide_long(lens, L, "h"), window=16, overlap=4,
                                   lengths=lens, noise=n2, clip_denoised=False, model_kwargs=kw2, skip_timesteps=SKIP, init_image=i2)
    assert bool(torch.isfinite(guided).all())
    assert torch.equal(before, plain())
