"""Guided sampling without a GPU: the float64 statement of both guided updates (tests/guide_fixture.py) against the reference's own
guided p_sample / ddim_sample outputs (tests/golden/guided.npz, made by tests/golden/make_golden_guided.py), the properties the
reference's forms have (the variance term vanishes at index 0, x0-hat never sees the guide), `TargetGuide.__call__` against the formula,
the ABI additions (header <-> ctypes <-> struct offsets) and every refusal that needs no device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import guide_fixture as gf
import mst_amd  # noqa: F401
from conftest import ROOT


def diffusion(resp="ddim20", inpainting=False, mean="START_X", var="FIXED_SMALL"):
    from mst_amd.diffusion import gaussian_diffusion as gd
    from mst_amd.diffusion.inpainting_gaussian_diffusion import InpaintingGaussianDiffusion
    from mst_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    cls = InpaintingGaussianDiffusion if inpainting else SpacedDiffusion
    return cls(use_timesteps=space_timesteps(1000, resp or [1000]), betas=gd.get_named_beta_schedule("cosine", 1000),
               model_mean_type=gd.ModelMeanType[mean], model_var_type=gd.ModelVarType[var], loss_type=gd.LossType.MSE)


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


# ------------------------------------------------------------------------------ the fixture against the reference
@pytest.mark.parametrize("tag,resp,t,variant", gf.single_step_cases(), ids=lambda v: str(v) if v != "" else "full")
def test_closed_forms_reproduce_every_reference_guided_step(tag, resp, t, variant):
    """The reference's fp32 guided sample of p_sample, ddim_sample(eta 0) and ddim_sample(eta 0.5), both a_t modes, from its own x0-hat,
    the seeded x, target and recorded noise: elementwise within BAR_STEP = 2e-5 of `scale`."""
    g = gf.golden()
    tab, _ = gf.tables(resp)
    v = gf.golden_inputs(tag)
    st = gf.STRIDE[tag]
    key = gf.key_of(tag, resp, t, variant)
    sub = lambda a: np.asarray(a)[..., ::st]
    x, y, m = sub(v["x"]), sub(v["y"]), sub(v["m"])
    pred = g[key + "|pred_xstart"]
    assert pred.shape == x.shape and pred.dtype == np.float32
    noise = sub(gf.step_noise(tag, key))
    if variant:
        noise = noise * (1 - sub(v["mask"]))                       # InpaintingGaussianDiffusion masks every draw
        assert np.array_equal(pred[:, :3], sub(v["motion"])[:, :3])
    worst = 0.0
    for sampler in gf.SAMPLERS:
        for follow in (0, 1):
            grad = gf.target_grad(tab, x, [t], y, m, gf.WEIGHT, follow)
            want, scale = gf.guided(tab, sampler, pred, x, [t], grad, noise)
            sample = g[f"{key}|{sampler}|{follow}|sample"]
            ratio = float((np.abs(sample - want) / scale).max())
            worst = max(worst, ratio)
            assert ratio <= gf.BAR_STEP, (sampler, follow, ratio)
            # a closed form that ignores the guide does not pass (away from index 0, where variance_0 = 0 and 1 - abar_0 is tiny)
            if t != 0:
                plain, _ = gf.guided(tab, sampler, pred, x, [t], np.zeros_like(grad), noise)
                assert float((np.abs(sample - plain) / scale).max()) > 10 * gf.BAR_STEP, (sampler, follow)
        if sampler == "ddpm" and t == 0:
            assert np.array_equal(g[f"{key}|ddpm|0|sample"], g[f"{key}|ddpm|1|sample"]), "variance_0 = 0: the guide cannot reach the sample"
    print(f"\n{key}: worst |ref - closed form| / scale = {worst:.2e} (bar {gf.BAR_STEP:.0e})")


@pytest.mark.parametrize("name,mean", [("eps", 1), ("prevx", 2)])
def test_closed_forms_reproduce_the_epsilon_and_previous_x_cases(name, mean):
    """An epsilon model and a previous-x model ("ddim20", index 10): the guided update acts behind the conversion to x0-hat.  (For the
    previous-x model the ancestral mean is the raw output; c1 pred + c2 x restates it from the stored x0-hat within the same bar.)"""
    g = gf.golden()
    tab, _ = gf.tables("ddim20")
    v = gf.golden_inputs("xia")
    st = gf.STRIDE["xia"]
    sub = lambda a: np.asarray(a)[..., ::st]
    x, y, m = sub(v["x"]), sub(v["y"]), sub(v["m"])
    pred, noise = g[f"xia|{name}|pred_xstart"], sub(gf.step_noise("xia", f"xia|{name}"))
    grad = gf.target_grad(tab, x, [10], y, m, gf.WEIGHT, 1)
    for sampler in ("ddpm", "ddim0.5"):
        want, scale = gf.guided(tab, sampler, pred, x, [10], grad, noise)
        ratio = float((np.abs(g[f"xia|{name}|{sampler}|sample"] - want) / scale).max())
        print(f"\n{name} {sampler}: {ratio:.2e}")
        assert ratio <= gf.BAR_STEP, (sampler, ratio)


def test_reference_loops_moved_by_the_guide():
    """The golden's own condition, on the stored file: the reference's guided and unguided 20-step loops differ by >= 0.05 relative
    L2, so an engine that ignores the guide cannot pass the whole-loop test."""
    g = gf.golden()
    for smp in ("ddim", "ddpm"):
        moved = rel_l2(g[f"xia|loop20|{smp}|guided"], g[f"xia|loop20|{smp}|plain"])
        print(f"\n{smp}: {moved:.3f}")
        assert np.isfinite(g[f"xia|loop20|{smp}|guided"]).all() and moved >= gf.MOVED


# ------------------------------------------------------------------------------ properties of the forms
@pytest.mark.parametrize("resp", ["", "100", "ddim20"], ids=["full", "100", "ddim20"])
def test_variance_term_is_exactly_zero_at_index_0_under_fixed_small(resp):
    tab, _ = gf.tables(resp)
    assert gf.variance_row(tab)[0] == 0.0 and gf.variance_row(tab, large=True)[0] > 0.0
    d = diffusion(resp)
    assert d._variance_tables()[0][0] == 0.0 and np.array_equal(d._variance_tables()[0], d.posterior_variance)
    big = diffusion(resp, var="FIXED_LARGE")._variance_tables()[0]
    assert big[0] == d.posterior_variance[1] and np.array_equal(big[1:], d.betas[1:])
    rng = np.random.default_rng(0)
    pred, x, grad, noise = (rng.standard_normal((2, 5, 1, 4)) for _ in range(4))
    a, _ = gf.guided_ddpm(tab, pred, x, [0, 0], 1e6 * grad, noise)
    b, _ = gf.guided_ddpm(tab, pred, x, [0, 0], 0 * grad, noise)
    assert np.array_equal(a, b)
    # it is the variance row, not exp(log_variance): the clipped log-variance is NOT zero there
    assert np.exp(d._variance_tables()[1][0]) > 0.0


def test_condition_mean_and_condition_score_of_the_mirror():
    """The torch forms (any device): condition_mean adds variance * g to the mean and nothing else; condition_score returns a copy
    whose pred_xstart / mean moved, the caller's dict -- and with it the x0-hat the samplers return -- untouched."""
    d = diffusion("ddim20")
    tab, _ = gf.tables("ddim20")
    rng = np.random.default_rng(1)
    shp = (3, 6, 1, 4)
    x, pred, tgt = (torch.from_numpy(rng.standard_normal(shp).astype(np.float32)) for _ in range(3))
    t = torch.tensor([0, 7, 19])
    from mst_amd.diffusion.guidance import TargetGuide
    guide = TargetGuide(tgt, weight=[0.5, 1.0, 2.0])
    grad = gf.target_grad(tab, x.numpy(), t.numpy(), tgt.numpy(), None, [0.5, 1.0, 2.0], 0)
    mean, var, logvar = d.q_posterior_mean_variance(pred, x, t)
    pmv = {"mean": mean, "variance": var, "log_variance": logvar, "pred_xstart": pred}
    new_mean = d.condition_mean(guide, pmv, x, t, model_kwargs={})
    want = mean.double().numpy() + gf.entry(tab, "posterior_variance", t.numpy(), x.numpy()) * grad
    assert np.allclose(new_mean.numpy(), want, rtol=0, atol=1e-5)
    assert torch.equal(new_mean[0], mean[0])                       # index 0: variance 0
    out = d.condition_score(guide, pmv, x, t, model_kwargs={})
    assert out is not pmv and pmv["pred_xstart"] is pred and torch.equal(pmv["mean"], mean)
    eps = (gf.entry(tab, "sqrt_recip_alphas_cumprod", t.numpy(), x.numpy()) * x.numpy() - pred.numpy()) / \
        gf.entry(tab, "sqrt_recipm1_alphas_cumprod", t.numpy(), x.numpy())
    eps = eps - np.sqrt(1 - gf.entry(tab, "alphas_cumprod", t.numpy(), x.numpy())) * grad
    pp = gf.entry(tab, "sqrt_recip_alphas_cumprod", t.numpy(), x.numpy()) * x.numpy() - gf.entry(tab, "sqrt_recipm1_alphas_cumprod", t.numpy(), x.numpy()) * eps
    assert np.allclose(out["pred_xstart"].numpy(), pp, rtol=0, atol=1e-4)
    assert [p for p in inspect.signature(d.condition_mean).parameters] == ["cond_fn", "p_mean_var", "x", "t", "model_kwargs"]
    assert [p for p in inspect.signature(d.condition_score).parameters] == ["cond_fn", "p_mean_var", "x", "t", "model_kwargs"]


# ------------------------------------------------------------------------------ TargetGuide
@pytest.mark.parametrize("follow", [0, 1])
@pytest.mark.parametrize("masked", [0, 1])
def test_target_guide_call_is_the_formula_also_under_a_respaced_map(follow, masked):
    """Directly (timesteps of the original process) and as SpacedDiffusion hands it over (respace.py:104-108: the cond_fn sees
    timestep_map[t]): the same numbers as the formula on the RESPACED table at the respaced index, which is what the kernel reads."""
    from mst_amd.diffusion.guidance import TargetGuide
    d = diffusion("ddim20")
    full = diffusion("")
    tab, tmap = gf.tables("ddim20")
    rng = np.random.default_rng(2)
    shp = (4, 6, 1, 5)
    x, tgt = (rng.standard_normal(shp).astype(np.float32) for _ in range(2))
    m = (rng.random(shp) < 0.5).astype(np.float32) if masked else None
    w = [0.0, 0.5, 1.0, 3.0]
    guide = TargetGuide(tgt, mask=m, weight=w, alphas_cumprod=full.alphas_cumprod if follow else None)
    t = np.array([0, 3, 11, 19])
    want = gf.target_grad(tab, x, t, tgt, m, w, follow)
    got = d._cond_gradient(guide, torch.from_numpy(x), torch.from_numpy(t), {"y": {}})
    assert got.dtype == torch.float32 and np.allclose(got.numpy(), want, rtol=1e-6, atol=1e-6)
    direct = guide(torch.from_numpy(x), torch.from_numpy(np.asarray(tmap)[t]))
    assert torch.equal(direct, got)
    assert np.array_equal(got.numpy()[0], np.zeros(shp[1:], np.float32))      # weight 0
    one = TargetGuide(tgt, weight=2.0)(torch.from_numpy(x), torch.from_numpy(t))
    assert np.allclose(one.numpy(), 2.0 * (tgt - x), rtol=1e-6, atol=1e-6)
    with pytest.raises(ValueError, match="rescaled"):
        guide(torch.from_numpy(x), torch.from_numpy(t).float() * 50.0)


def test_target_guide_table_is_checked_against_the_process_at_loop_entry():
    from mst_amd.diffusion.guidance import TargetGuide
    d, full = diffusion("ddim20"), diffusion("")
    x = torch.zeros(1, 4, 1, 4)
    with pytest.raises(ValueError, match="ORIGINAL process"):
        d._target_guide_args(TargetGuide(x, alphas_cumprod=d.alphas_cumprod), x)          # the respaced table: indexed by timestep_map it is another one
    with pytest.raises(ValueError, match="ORIGINAL process"):
        d._target_guide_args(TargetGuide(x, alphas_cumprod=full.alphas_cumprod[:500]), x)
    with pytest.raises(RuntimeError, match="GPU tensor"):                               # the right table passes the check (and then wants a device)
        d._target_guide_args(TargetGuide(x, alphas_cumprod=full.alphas_cumprod), x)


# ------------------------------------------------------------------------------ ABI
def _header():
    return open(os.path.join(ROOT, "include", "mst_engine.h")).read()


def test_guide_struct_header_ctypes_and_offsets_agree():
    from mst_amd import _native as N
    body = re.search(r"typedef struct mst_guide_args \{(.*?)\} mst_guide_args;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(ty.strip(), name) for ty, name in re.findall(r"([a-z_0-9 ]+?[ *]+)([a-z_]+);", body)]
    assert [n for _, n in fields] == [n for n, _ in N.MstGuideArgs._fields_] == \
        ["kind", "follow_schedule", "grad_dev", "target_dev", "mask_dev", "weight_dev"]
    for (ty, name), (_, ct) in zip(fields, N.MstGuideArgs._fields_):
        assert (ct is C.c_int32) == (ty == "int32_t") and (ct is C.c_void_p) == ty.endswith("*"), (ty, name)
    assert C.sizeof(N.MstGuideArgs) == 2 * 4 + 4 * 8
    assert [getattr(N.MstGuideArgs, n).offset for n, _ in N.MstGuideArgs._fields_] == [0, 4, 8, 16, 24, 32]
    # mst_loop_args and mst_plms_args keep their layout
    assert C.sizeof(N.MstLoopArgs) == 9 * 4 + 4 + 8 + 6 * 8 and C.sizeof(N.MstPlmsArgs) == 16
    assert re.search(r"enum \{ MST_GUIDE_GRADIENT = 1, MST_GUIDE_TARGET = 2 \};", _header())
    from mst_amd import engine
    assert (engine.GUIDE_GRADIENT, engine.GUIDE_TARGET) == (1, 2)


def test_new_entries_are_declared_bound_and_exported():
    import __graft_entry__ as g
    g.build()
    from mst_amd import _native as N
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = N.lib()
    for name, nargs in (("mst_schedule_set_variance", 2), ("mst_sample_loop_guided", 5), ("mst_step_epilogue_guided", 18)):
        decl = re.search(r"\b" + name + r"\s*\((.*?)\);", text, flags=re.S).group(1)
        assert len(decl.split(",")) == nargs == len(N.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    # the entries whose layout the issue keeps: same declarations as before
    assert re.search(r"mst_schedule_create\(int32_t num_steps, const float\* tables_host,\s*const int32_t\* timestep_map_host, int32_t device, mst_schedule\*\* out\);", text)
    assert "MST_NTAB = 9" in text
    assert N.SIGNATURES["mst_sample_loop_guided"][1][3] == C.POINTER(N.MstGuideArgs)
    assert N.SIGNATURES["mst_step_epilogue_guided"][1][14] == C.POINTER(N.MstGuideArgs)


def test_null_arguments_are_refused_without_a_gpu():
    from mst_amd import _native as N
    lib = N.lib()
    a, g = N.MstLoopArgs(), N.MstGuideArgs()
    assert lib.mst_sample_loop_guided(None, None, C.byref(a), C.byref(g), None) != 0
    assert b"mst_sample_loop_guided: null argument" in lib.mst_last_error()
    assert lib.mst_schedule_set_variance(None, None) != 0
    assert b"mst_schedule_set_variance" in lib.mst_last_error()
    assert lib.mst_step_epilogue_guided(None, None, None, None, None, None, None, 1, 1, 0, 0, 0.0, 0, 0, None, None, None, None) != 0
    assert b"mst_step_epilogue_guided" in lib.mst_last_error()


# ------------------------------------------------------------------------------ the mirror's host composition and refusals
class HostSchedule:
    """Schedule.step / step_guided on the host (float64 behind float32 tensors), recording how they were called."""

    def __init__(self, tab):
        self.tab, self.calls = tab, []

    def _run(self, mo, x, t, noise, grad, sampler, eta, mask, motion, mask_noise, clip_denoised, mean_type):
        self.calls.append(dict(guided=grad is not None, blend=mask is not None and motion is not None, mask_noise=mask_noise,
                               mean_type=mean_type, clip=clip_denoised))
        mk = None if mask is None or motion is None else mask.double().numpy()
        pred, raw = gf.xstart64(self.tab, mean_type, mo.double().numpy(), x.double().numpy(), t.numpy(), mk,
                                None if mk is None else motion.double().numpy(), clip_denoised)
        nz = noise.double().numpy() * ((1 - mask.double().numpy()) if mask_noise else 1.0)
        g = np.zeros_like(pred) if grad is None else grad.double().numpy()
        s, _ = gf.guided(self.tab, None if sampler == 0 else eta, pred, x.double().numpy(), t.numpy(), g, nz,
                         **({"raw_mean": raw} if sampler == 0 and mean_type == 2 else {}))
        f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
        return f(s), f(pred)

    def step(self, mo, x, t, noise, sampler=0, eta=0.0, mask=None, motion=None, mask_noise=False, clip_denoised=False, mean_type=0):
        return self._run(mo, x, t, noise, None, sampler, eta, mask, motion, mask_noise, clip_denoised, mean_type)

    def step_guided(self, mo, x, t, noise, guide, sampler=0, eta=0.0, mask=None, motion=None, mask_noise=False, clip_denoised=False,
                    mean_type=0):
        return self._run(mo, x, t, noise, guide, sampler, eta, mask, motion, mask_noise, clip_denoised, mean_type)


@pytest.fixture
def host(monkeypatch):
    from mst_amd import engine
    monkeypatch.setattr(engine, "guide_args", lambda x, grad=None, **kw: grad)          # (the stand-in takes the gradient tensor itself)

    def on(d, resp="ddim20"):
        h = HostSchedule(gf.tables(resp)[0])
        d._schedule = lambda device: h
        return h
    return on


@pytest.mark.parametrize("ddim", [0, 1])
def test_step_composition_cond_fn_and_denoised_fn(host, ddim):
    """p_sample / ddim_sample of the mirror over the host stand-in: a cond_fn is evaluated on x_t with the process's timesteps and goes to
    the guided step; a denoised_fn runs between the blend / conversion (host) and the step, which then sees an x_start prediction and
    no blend but still masks the noise; both together; x0-hat is the same with and without the guide."""
    d = diffusion("ddim20", inpainting=True)
    h = host(d)
    tab, tmap = gf.tables("ddim20")
    rng = np.random.default_rng(3)
    shp = (2, 6, 1, 4)
    x, mo, motion, tgt = (torch.from_numpy(rng.standard_normal(shp).astype(np.float32)) for _ in range(4))
    mask = torch.zeros(shp)
    mask[:, :2] = 1
    kw = {"y": {"inpainting_mask": mask, "inpainted_motion": motion}}
    t = torch.tensor([7, 19])
    seen = []

    def cond_fn(xx, tt, **k):
        seen.append((tt.clone(), sorted(k)))
        return 0.25 * (tgt - xx)
    run = (lambda **k: d.ddim_sample(lambda *a, **kk: mo, x, t, clip_denoised=False, model_kwargs=kw, eta=0.5, **k)) if ddim else \
        (lambda **k: d.p_sample(lambda *a, **kk: mo, x, t, clip_denoised=False, model_kwargs=kw, **k))
    torch.manual_seed(0)
    plain = run()
    torch.manual_seed(0)
    guided = run(cond_fn=cond_fn)
    assert torch.equal(seen[0][0], torch.from_numpy(np.asarray(tmap))[t]) and seen[0][1] == ["y"]
    assert torch.equal(plain["pred_xstart"], guided["pred_xstart"]) and not torch.equal(plain["sample"], guided["sample"])
    assert h.calls[-1] == dict(guided=True, blend=True, mask_noise=True, mean_type=0, clip=False)
    torch.manual_seed(0)
    ident = run(denoised_fn=lambda v: v)
    assert h.calls[-1] == dict(guided=False, blend=False, mask_noise=True, mean_type=0, clip=False)
    assert np.allclose(ident["sample"].numpy(), plain["sample"].numpy(), rtol=0, atol=1e-5)
    torch.manual_seed(0)
    both = run(denoised_fn=lambda v: v.clamp(-0.5, 0.5), cond_fn=cond_fn)
    assert h.calls[-1]["guided"] and not h.calls[-1]["blend"]
    assert float(both["pred_xstart"].abs().max()) <= 0.5


def test_refusals_that_need_no_device():
    d = diffusion("ddim20")
    x, t = torch.zeros(1, 4, 1, 4), torch.zeros(1, dtype=torch.long)
    model = lambda *a, **k: x
    with pytest.raises(NotImplementedError, match="guided PLMS is out of scope"):
        d.plms_sample(model, x, t, cond_fn=lambda *a, **k: x)
    with pytest.raises(NotImplementedError, match="guided PLMS is out of scope"):
        next(d.plms_sample_loop_progressive(model, (1, 4, 1, 4), noise=x, device="cpu", cond_fn=lambda *a, **k: x))
    with pytest.raises(NotImplementedError, match="ddim_reverse_sample: cond_fn / denoised_fn"):
        d.ddim_reverse_sample(model, x, t, denoised_fn=lambda v: v)
    with pytest.raises(AssertionError):
        d.p_sample_with_grad(model, x, t, cond_fn=lambda *a, **k: x)
    with pytest.raises(AssertionError):
        d.ddim_sample_with_grad(model, x, t, denoised_fn=lambda v: v)
    with pytest.raises(NotImplementedError, match="randomize_class"):
        next(d.p_sample_loop_progressive(model, (1, 4, 1, 4), noise=x, device="cpu", randomize_class=True, cond_fn=lambda *a, **k: x))
    prev = diffusion("ddim20", mean="PREVIOUS_X")
    with pytest.raises(NotImplementedError, match="previous-x"):
        prev.p_sample(model, x, t, denoised_fn=lambda v: v)
    with pytest.raises(AssertionError, match="gradient of x's shape"):
        d.p_sample(model, x, t, cond_fn=lambda xx, tt, **k: xx[:, :2])
    assert "cond_fn" in inspect.signature(d.p_sample).parameters and "cond_fn" not in inspect.signature(d.ddim_reverse_sample).parameters
