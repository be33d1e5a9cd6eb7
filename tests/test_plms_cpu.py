"""The PLMS sampler without a GPU: the float64 statement of the step (tests/plms_fixture.py) against the reference's own `plms_sample`
outputs (tests/golden/plms.npz, made by tests/golden/make_golden_plms.py), the coefficient table, the history bookkeeping of the
mirror's `plms_sample` (over a host stand-in for the device schedule), the public names and every Python-side refusal."""
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
import plms_fixture as pf
from conftest import ROOT

# the reference's parameter names, recorded from diffusion/gaussian_diffusion.py:1084-1096, :1168-1184, :1210-1226
REF_PLMS_SAMPLE = ["self", "model", "x", "t", "clip_denoised", "denoised_fn", "cond_fn", "model_kwargs", "cond_fn_with_grad", "order",
                   "old_out"]
REF_PLMS_LOOP = ["self", "model", "shape", "noise", "clip_denoised", "denoised_fn", "cond_fn", "model_kwargs", "device", "progress",
                 "skip_timesteps", "init_image", "randomize_class", "cond_fn_with_grad", "order"]


def diffusion(resp="ddim20", inpainting=False):
    from mst_amd.diffusion import gaussian_diffusion as gd
    from mst_amd.diffusion.inpainting_gaussian_diffusion import InpaintingGaussianDiffusion
    from mst_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    cls = InpaintingGaussianDiffusion if inpainting else SpacedDiffusion
    return cls(use_timesteps=space_timesteps(1000, resp or [1000]), betas=gd.get_named_beta_schedule("cosine", 1000),
               model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE)


def on_host(d, resp="ddim20"):
    """`d` with the device schedule replaced by the float64 host stand-in."""
    h = pf.HostSchedule(pf.tables(resp)[0])
    d._schedule = lambda device: h
    return h


# ------------------------------------------------------------------------------ the fixture against the reference
@pytest.mark.parametrize("tag,resp,t,pair", pf.single_step_cases(), ids=lambda v: str(v) if v != "" else "full")
def test_closed_form_reproduces_every_reference_multistep_step(tag, resp, t, pair):
    """The reference's fp32 sample at cur_order 1..4 from its own x0-hat, the seeded x and the seeded history, elementwise within
    BAR_STEP = 2e-5 of `scale` (measured: 2.6e-7 at worst): the bar the GPU tests use hides nothing the reference itself does."""
    g = pf.golden()
    tab, _ = pf.tables(resp)
    v = pf.golden_inputs(tag)
    st = pf.STRIDE[tag]
    x, hist = v["x"][..., ::st], [h[..., ::st] for h in v["hist"]]
    pred = g[f"{tag}|{resp}|{t}|{pair}|pred_xstart"]
    assert pred.shape == x.shape and pred.dtype == np.float32
    worst = 0.0
    for c in (1, 2, 3, 4):
        sample = g[f"{tag}|{resp}|{t}|{pair}|{c}|sample"]
        want, scale, _ = pf.closed_form(tab, pred, x, [t], hist[:c - 1])
        ratio = float((np.abs(sample - want) / scale).max())
        worst = max(worst, ratio)
        assert ratio <= pf.BAR_STEP, (c, ratio)
        if t == 0:
            assert np.array_equal(sample, pred)                   # sample IS pred at index 0, bit for bit
    print(f"\n{tag} '{resp}' t={t} pair={pair}: worst |ref - closed form| / scale over cur_order 1..4 = {worst:.2e}")
    if pair:                                                      # masked rows of x0-hat are the motion, bit for bit
        assert np.array_equal(pred[:, :3], v["motion"][:, :3, :, ::st])


@pytest.mark.parametrize("tag,t,pair", pf.euler_cases())
def test_closed_form_reproduces_the_reference_euler_step(tag, t, pair):
    """The first step of a chain (two evaluations).  The golden holds the sample, the first evaluation's x0-hat, the eps the history
    took and the model's raw second output: eps is the FIRST evaluation's, x_mid comes from pred itself, and the sample is the second
    half's closed form from the blended second output -- all within BAR_STEP of the products summed."""
    g = pf.golden()
    tab, _ = pf.tables("ddim20")
    v = pf.golden_inputs(tag)
    st = pf.STRIDE[tag]
    x, mask, motion = (v[k][..., ::st] for k in ("x", "mask", "motion"))
    pred, eps, sample, out2 = (g[f"{tag}|euler|{t}|{pair}|{k}"] for k in ("pred_xstart", "eps", "sample", "out2"))
    x_mid, _, eps64 = pf.euler_first(tab, pred, x, [t])
    srac, srm1, _ = pf._entries(tab, [t], x)
    r = float((np.abs(eps - eps64) * srm1 / (srac * np.abs(x) + np.abs(pred))).max())
    assert r <= pf.BAR_STEP, r                                     # the history takes eps of the FIRST evaluation
    pred2 = pf.blend(out2, mask, motion).astype(np.float32) if pair else out2
    want, scale = pf.euler_second(tab, pred2, x_mid, x, eps64, [t])
    ratio = float((np.abs(sample - want) / scale).max())
    print(f"\n{tag} euler t={t} pair={pair}: eps {r:.2e}, sample |ref - closed form| / scale = {ratio:.2e}")
    assert ratio <= pf.BAR_STEP
    plain, _, _ = pf.closed_form(tab, pred, x, [t])               # ... and it is not the one-evaluation step
    assert np.abs(sample - plain).max() > 1e-3
    if pair:
        assert np.array_equal(pred[:, :3], motion[:, :3])


# ------------------------------------------------------------------------------ the coefficient table
def test_coefficient_table_is_adams_bashforth():
    """Orders 1..4 of the reference (:1147-1154); each row sums to 1 (a constant eps is reproduced) and is exact for polynomials of
    degree < order in the step number (the Adams-Bashforth conditions); the magnitudes sum to what the whole-loop bar uses."""
    want = {1: [1], 2: [Fraction(3, 2), Fraction(-1, 2)], 3: [Fraction(23, 12), Fraction(-16, 12), Fraction(5, 12)],
            4: [Fraction(55, 24), Fraction(-59, 24), Fraction(37, 24), Fraction(-9, 24)]}
    for r, row in want.items():
        assert np.allclose(pf.COEF[r], [float(c) for c in row], rtol=0, atol=1e-16)
        assert sum(row) == 1
        for p in range(r):                                       # integral over [0, 1] of s^p from values at s = 0, -1, -2, ..
            assert sum(c * Fraction(-i) ** p for i, c in enumerate(row)) == Fraction(1, p + 1), (r, p)
    assert pf.A == {1: 1.0, 2: 2.0, 3: pytest.approx(44 / 12), 4: pytest.approx(160 / 24)}


# ------------------------------------------------------------------------------ history bookkeeping of the mirror
@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_history_bookkeeping_and_live_list(order):
    """A 6-step chain through `plms_sample` on the host stand-in: the list's length after each step, cur_order per step, the
    Euler step first (order > 1), `eps` (never eps') appended, and the SAME list object handed on and mutated, as in the reference."""
    d = diffusion()
    h = on_host(d)
    tab = h.tab
    rng = np.random.default_rng(order)
    shp = (2, 5, 1, 4)
    preds = [torch.from_numpy(rng.standard_normal(shp).astype(np.float32)) for _ in range(8)]
    it = iter(preds)
    model = lambda x, t, **kw: next(it)
    x = torch.from_numpy(rng.standard_normal(shp).astype(np.float32))
    old_out = {"old_eps": []} if order == 1 else None
    lens, lists, t0 = [], [], 15
    for k in range(6):
        t = torch.full((2,), t0 - k, dtype=torch.long)
        passed = None if old_out is None else old_out["old_eps"]
        before = None if passed is None else list(passed)
        out = d.plms_sample(model, x, t, clip_denoised=False, model_kwargs={}, order=order, old_out=old_out)
        assert set(out) == {"sample", "pred_xstart", "old_eps"} and isinstance(out["old_eps"], list)
        if passed is not None:
            assert out["old_eps"] is passed, "old_eps must be the caller's list, mutated"
        # what was appended is eps of THIS step's (first) evaluation
        eps = pf.eps_of(tab, out["pred_xstart"].numpy(), x.numpy(), t.numpy()).astype(np.float32)
        if order > 1:
            assert np.array_equal(out["old_eps"][-1].numpy(), eps)
            if before is not None:                               # the older entries moved up, the oldest dropped
                kept = before[-(order - 2):] if order > 2 else []
                assert all(a is b for a, b in zip(out["old_eps"][:-1], kept))
        lens.append(len(out["old_eps"]))
        lists.append(out["old_eps"])
        old_out, x = out, out["sample"]
    assert lens == [min(k + 1, order - 1) for k in range(6)]
    assert all(l is lists[0] for l in lists)
    want_calls = ([("step", 0, t0), ("euler", 0, t0)] if order > 1 else [("step", 1, t0)]) + \
        [("step", min(order, k + 1), t0 - k) for k in range(1, 6)]
    assert h.calls == want_calls
    # live-list semantics: the dict yielded at step 1 now shows the history as of step 5
    assert len(lists[0]) == lens[-1]


def test_single_step_equals_the_fixture_and_first_half_uses_pred_itself():
    d = diffusion()
    h = on_host(d)
    rng = np.random.default_rng(7)
    shp = (1, 6, 1, 8)
    f = lambda: torch.from_numpy(rng.standard_normal(shp).astype(np.float32))
    x, p1, p2, e1, e2 = f(), f(), f(), f(), f()
    t = torch.tensor([9])
    out = d.plms_sample(lambda *a, **k: p1, x, t, clip_denoised=False, order=3, old_out={"old_eps": [e2, e1]})
    want, _, _ = pf.closed_form(h.tab, p1.numpy(), x.numpy(), [9], [e1.numpy(), e2.numpy()])
    assert np.array_equal(out["sample"].numpy(), want.astype(np.float32))
    outs = iter([p1, p2])
    seen = []

    def model(xx, tt, **kw):
        seen.append((xx.clone(), tt.clone()))
        return next(outs)

    out = d.plms_sample(model, x, t, clip_denoised=False, order=2, old_out=None)
    x_mid, _, eps = pf.euler_first(h.tab, p1.numpy(), x.numpy(), [9])
    assert len(seen) == 2 and np.array_equal(seen[1][0].numpy(), x_mid.astype(np.float32))
    assert int(seen[0][1][0]) == d.timestep_map[9] and int(seen[1][1][0]) == d.timestep_map[8]     # the second evaluation is at t - 1
    want2, _ = pf.euler_second(h.tab, p2.numpy(), x_mid.astype(np.float32), x.numpy(), eps.astype(np.float32), [9])
    assert np.array_equal(out["sample"].numpy(), want2.astype(np.float32))
    assert len(out["old_eps"]) == 1 and np.array_equal(out["old_eps"][0].numpy(), eps.astype(np.float32))
    assert np.array_equal(out["pred_xstart"].numpy(), p1.numpy())                          # the FIRST evaluation's x0-hat
    out_c = d.plms_sample(lambda *a, **k: 3 * p1, x, t, clip_denoised=True, order=1, old_out={"old_eps": []})
    assert out_c["pred_xstart"].abs().max() <= 1


# ------------------------------------------------------------------------------ names and signatures
def test_signatures_are_the_reference_s_and_public_names():
    from mst_amd import _native as N
    from mst_amd import engine
    from mst_amd.diffusion.gaussian_diffusion import GaussianDiffusion as G
    assert list(inspect.signature(G.plms_sample).parameters) == REF_PLMS_SAMPLE
    assert list(inspect.signature(G.plms_sample_loop).parameters) == REF_PLMS_LOOP
    assert list(inspect.signature(G.plms_sample_loop_progressive).parameters) == REF_PLMS_LOOP
    p = inspect.signature(G.plms_sample).parameters
    assert (p["clip_denoised"].default, p["cond_fn_with_grad"].default, p["order"].default, p["old_out"].default) == (True, False, 2, None)
    p = inspect.signature(G.plms_sample_loop_progressive).parameters
    assert (p["skip_timesteps"].default, p["randomize_class"].default, p["order"].default, p["init_image"].default) == (0, False, 2, None)
    p = inspect.signature(G.plms_sample_loop_from).parameters
    assert list(p)[:5] == ["self", "model", "x_t", "num_steps", "order"] and p["order"].default == 2
    text = open(os.path.join(ROOT, "include", "mst_engine.h")).read()
    m = re.search(r"MST_SAMPLER_PLMS\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == engine.SAMPLER_PLMS == 3
    assert re.search(r"typedef struct mst_plms_args \{\s*int32_t order;[^}]*int32_t steps_done;[^}]*float\*\s*hist_dev;[^}]*\} mst_plms_args;", text)
    for name in ("mst_sample_loop_plms", "mst_plms_epilogue", "mst_plms_euler"):
        assert name in N.SIGNATURES and re.search(rf"\bint {name}\(", text)
    import ctypes as C
    assert C.sizeof(N.MstPlmsArgs) == 16 and N.MstPlmsArgs.hist_dev.offset == 8
    assert hasattr(engine.DenoiserEngine, "sample_loop_plms") and hasattr(engine.Schedule, "plms_step") and hasattr(engine.Schedule, "plms_euler")


# ------------------------------------------------------------------------------ refusals on the Python side
def test_python_side_refusals():
    d = diffusion()
    on_host(d)
    x, t = torch.zeros(1, 4, 1, 4), torch.full((1,), 5, dtype=torch.long)
    model = lambda *a, **k: x
    for bad in (0, 5, -1):
        with pytest.raises(ValueError, match="order is invalid"):
            d.plms_sample(model, x, t, order=bad, old_out={"old_eps": []})
        with pytest.raises(ValueError, match="order is invalid"):
            next(d.plms_sample_loop_progressive(model, (1, 4, 1, 4), noise=x, device="cpu", order=bad))
        with pytest.raises(ValueError, match="order is invalid"):
            d.plms_sample_loop_from(model, x, 3, order=bad, device="cpu")
    with pytest.raises(NotImplementedError, match="cond_fn"):
        d.plms_sample(model, x, t, cond_fn=lambda *a, **k: x)
    with pytest.raises(NotImplementedError, match="denoised_fn"):
        d.plms_sample(model, x, t, denoised_fn=lambda v: v)
    with pytest.raises(NotImplementedError, match="cond_fn"):
        next(d.plms_sample_loop_progressive(model, (1, 4, 1, 4), noise=x, device="cpu", cond_fn=lambda *a, **k: x, cond_fn_with_grad=True))
    with pytest.raises(NotImplementedError, match="randomize_class"):
        d.plms_sample_loop(model, (1, 4, 1, 4), noise=x, device="cpu", randomize_class=True)
    # a chain that starts at index 0 with order > 1: the reference would evaluate the model at index -1
    with pytest.raises(ValueError, match="cannot start at index 0"):
        d.plms_sample(model, x, torch.zeros(1, dtype=torch.long), order=2, old_out=None)
    with pytest.raises(ValueError, match="cannot start at index 0"):
        d.plms_sample_loop_from(model, x, 1, order=2, device="cpu")
    with pytest.raises(ValueError, match="cannot start at index 0"):
        d.plms_sample_loop(model, (1, 4, 1, 4), noise=x, device="cpu", skip_timesteps=19, init_image=None, order=3)
    assert d.plms_sample_loop_from(model, x, 1, order=1, device="cpu").shape == x.shape          # order 1 may: one evaluation, at index 0
    with pytest.raises(ValueError, match="num_steps"):
        d.plms_sample_loop_from(model, x, 21, device="cpu")
    # order 1 through the loop starts from an empty history instead of raising (the reference: TypeError)
    outs = list(d.plms_sample_loop_progressive(model, (1, 4, 1, 4), noise=x, device="cpu", order=1, clip_denoised=False))
    assert len(outs) == 20 and all(o["old_eps"] == [] for o in outs)
    # the reference's single step with order 1 and no old_out subscripts None: kept
    with pytest.raises(TypeError):
        d.plms_sample(model, x, t, order=1, old_out=None)


def test_loop_under_inpainting_diffusion_passes_model_kwargs_to_q_sample():
    """The reference's plms loop calls q_sample(init_image, t, img) without model_kwargs, which InpaintingGaussianDiffusion.q_sample
    needs (TypeError there); here the loop's set-up is the other loops' and hands them over."""
    d = diffusion(inpainting=True)
    on_host(d)
    x = torch.zeros(1, 4, 1, 4)
    seen = {}

    def q_sample(x_start, t, noise=None, model_kwargs=None):
        seen["kw"] = model_kwargs
        return x_start

    d.q_sample = q_sample
    kw = {"y": {"inpainting_mask": torch.zeros(1, 4, 1, 4), "inpainted_motion": x}}
    out = d.plms_sample_loop(lambda *a, **k: x, (1, 4, 1, 4), noise=x, device="cpu", skip_timesteps=17, init_image=x, model_kwargs=kw,
                             clip_denoised=False, order=2)
    assert seen["kw"] is kw and out.shape == x.shape
