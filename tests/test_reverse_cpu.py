"""DDIM inversion without a GPU: the float64 statement of the reverse step (tests/reverse_fixture.py) against the reference's own
`ddim_reverse_sample` outputs (tests/golden/reverse.npz, made by tests/golden/make_golden_reverse.py), the `alphas_cumprod_next`
lookup the kernels use instead of a table row, and the public names."""
import inspect
import os
import re

import numpy as np
import pytest

import mst_amd  # noqa: F401
import reverse_fixture as rf
from conftest import ROOT

RESPACINGS = ("", "100", "ddim20")


@pytest.mark.parametrize("tag,resp,t,pair", rf.single_step_cases(), ids=lambda v: str(v) if v != "" else "full")
def test_closed_form_reproduces_the_reference_step_from_its_own_xstart(tag, resp, t, pair):
    """sample == the closed form, elementwise within 1e-6 of A |pred| + b |x| (reverse_fixture: the magnitudes of the products that
    are summed): the reference's fp32 operations against float64 arithmetic on the same float32-rounded table entries (about five
    roundings of 2^-24 = 6e-8 each)."""
    g = rf.golden()
    tab, _ = rf.tables(resp)
    x = rf.golden_inputs(tag)["x"][..., ::rf.STRIDE[tag]]
    pred, sample = g[f"{tag}|{resp}|{t}|{pair}|pred_xstart"], g[f"{tag}|{resp}|{t}|{pair}|sample"]
    assert pred.shape == x.shape == sample.shape and pred.dtype == np.float32
    want, scale = rf.closed_form(tab, pred, x, [t])
    ratio = np.abs(sample - want) / scale
    print(f"\n{tag} '{resp}' t={t} pair={pair}: worst |ref - closed form| / (A |pred| + b |x|) = {ratio.max():.2e}, g(t) = {float(rf.g(tab, t)):.3f}")
    assert ratio.max() <= 1e-6
    if t == len(tab["alphas_cumprod"]) - 1:                       # acn = 0: the sample IS eps
        assert np.abs(sample - rf.eps_of(tab, pred, x, [t])).max() <= 1e-6 * np.abs(scale).max()
    if pair:                                                      # masked rows of x0-hat are the motion, bit for bit
        motion = rf.golden_inputs(tag)["motion"][..., ::rf.STRIDE[tag]]
        assert np.array_equal(pred[:, :3], motion[:, :3])


def test_float64_table_entries_would_miss_the_bar_at_the_first_index_of_the_full_schedule():
    """Why `coefs` rounds the entries as the reference's `.float()` does: at index 0 of the unrespaced schedule acn is 1 - 1e-4 and its
    float32 rounding moves sqrt(1 - acn) by more than the 1e-6 bar.  (If this ever stops holding, the rounding in the fixture is moot.)"""
    tab, _ = rf.tables("")
    acn = float(rf.acn_of(tab, 0))
    r32 = float(np.float32(acn))
    assert abs(np.sqrt(1 - r32) / np.sqrt(1 - acn) - 1) > 1e-6


@pytest.mark.parametrize("resp", RESPACINGS, ids=["full", "100", "ddim20"])
def test_alphas_cumprod_next_is_the_next_alphas_cumprod_and_zero_at_the_end(resp, golden):
    tab, _ = rf.tables(resp)
    n = len(tab["alphas_cumprod"])
    got = rf.acn_of(tab, np.arange(n))
    assert got[-1] == 0.0
    assert np.array_equal(got[:-1], tab["alphas_cumprod"][1:])
    assert np.array_equal(got, tab["alphas_cumprod_next"])                                # the oracle's table
    assert np.array_equal(got, golden["schedules"][f"cosine|{resp}|alphas_cumprod_next"])  # the reference's table
    # ... and the mirror's diffusion object has the same table and no engine row for it
    from mst_amd.diffusion.gaussian_diffusion import schedule_tables
    from mst_amd.engine import TABLE_ORDER
    mine, _ = schedule_tables("cosine", 1000, resp)
    assert np.array_equal(mine["alphas_cumprod_next"], got)
    assert "alphas_cumprod_next" not in TABLE_ORDER and len(TABLE_ORDER) == 9


def test_conditioning_of_the_reverse_step_is_what_the_issue_tabulates():
    """g(t) from oracle/schedule.py's tables (cosine, 1000 steps): the factors the tolerances of tests/test_gpu_reverse.py rest on."""
    for resp, g0, g1 in (("", 0.455, 0.455), ("100", 3.18, 0.618), ("ddim20", 13.16, 0.86)):
        tab, _ = rf.tables(resp)
        n = len(tab["alphas_cumprod"])
        g = rf.g(tab, np.arange(n))
        assert abs(g[0] - g0) < 0.005 * g0 + 0.005, (resp, g[0])
        assert g[1:].max() <= g1 + 0.005, (resp, g[1:].max())
        a, _ = rf.coefs(tab, np.arange(n))
        # |a(t)| IS g(t), up to the float32 rounding of the entries (largest at index 0 of the full schedule: 2.9e-4, through 1 - acn)
        assert np.allclose(np.abs(a), g, rtol=1e-3, atol=1e-6)


def test_mirror_signature_and_public_names():
    from mst_amd import engine
    from mst_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    assert str(inspect.signature(GaussianDiffusion.ddim_reverse_sample)) == \
        "(self, model, x, t, clip_denoised=True, denoised_fn=None, model_kwargs=None, eta=0.0)"
    assert str(inspect.signature(GaussianDiffusion.ddim_reverse_sample_loop)) == \
        "(self, model, x_start, num_steps=None, clip_denoised=True, model_kwargs=None, device=None, progress=False, dump_all_xstart=False)"
    p = inspect.signature(GaussianDiffusion.ddim_sample_loop_from).parameters
    assert list(p)[:5] == ["self", "model", "x_t", "num_steps", "eta"] and p["eta"].default == 0.0
    ref = inspect.signature(GaussianDiffusion.ddim_sample_loop).parameters
    assert set(p) - {"x_t", "num_steps"} <= set(ref)                                      # only keyword arguments ddim_sample_loop has
    assert hasattr(GaussianDiffusion, "ddim_reverse_sample_loop_progressive")
    text = open(os.path.join(ROOT, "include", "mst_engine.h")).read()
    m = re.search(r"MST_SAMPLER_DDIM_REVERSE\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == engine.SAMPLER_DDIM_REVERSE == 2
    assert (engine.SAMPLER_DDPM, engine.SAMPLER_DDIM) == (0, 1)


def test_reverse_step_refuses_eta_and_denoised_fn_before_touching_a_device():
    import torch
    from mst_amd.diffusion.gaussian_diffusion import schedule_tables  # noqa: F401
    from mst_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    from mst_amd.diffusion import gaussian_diffusion as gd
    d = SpacedDiffusion(use_timesteps=space_timesteps(1000, "ddim20"), betas=gd.get_named_beta_schedule("cosine", 1000),
                        model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE)
    x, t = torch.zeros(1, 4, 1, 4), torch.zeros(1, dtype=torch.long)
    with pytest.raises(AssertionError, match="Reverse ODE only for deterministic path"):
        d.ddim_reverse_sample(lambda *a, **k: x, x, t, eta=0.5)
    with pytest.raises(NotImplementedError, match="denoised_fn"):
        d.ddim_reverse_sample(lambda *a, **k: x, x, t, denoised_fn=lambda v: v)
    with pytest.raises(ValueError, match="num_steps"):
        next(d.ddim_reverse_sample_loop_progressive(lambda *a, **k: x, x, num_steps=21))
