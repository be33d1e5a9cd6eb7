"""Joint-space guidance without a GPU: the float64 statement of the likelihood (tests/joint_guide_fixture.py) against the reference's own
`recover_from_ric` under autograd (tests/golden/joint_guide.npz, made by tests/golden/make_golden_joint_guide.py) and against its own
central differences, the `keyframes` / `root_path` builders, the public names and signatures, and every refusal that needs no device."""
import inspect
import types

import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
import joint_guide_fixture as jf

# the reference's parameter names, recorded from diffusion/inpainting_gaussian_diffusion.py:66-77, :179-190 and
# diffusion/gaussian_diffusion.py:469, :508
REF_P_SAMPLE_WITH_GRAD = ["self", "model", "x", "t", "clip_denoised", "denoised_fn", "cond_fn", "model_kwargs", "pred_xstart_in_graph",
                          "const_noise"]
REF_DDIM_SAMPLE_WITH_GRAD = ["self", "model", "x", "t", "clip_denoised", "denoised_fn", "cond_fn", "model_kwargs", "eta",
                             "pred_xstart_in_graph"]
REF_CONDITION_WITH_GRAD = ["self", "cond_fn", "p_mean_var", "x", "t", "model_kwargs"]


def diffusion(resp="ddim20"):
    from mst_amd.diffusion import gaussian_diffusion as gd
    from mst_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    return SpacedDiffusion(use_timesteps=space_timesteps(1000, resp or [1000]), betas=gd.get_named_beta_schedule("cosine", 1000),
                           model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL,
                           loss_type=gd.LossType.MSE)


# ------------------------------------------------------------------------------ the fixture against the reference
@pytest.mark.parametrize("J,F,T,B,pattern", jf.GOLDEN_CASES)
def test_fixture_equals_the_reference_in_float64(J, F, T, B, pattern):
    g = jf.golden()
    key = f"J{J}|F{F}|T{T}|B{B}|{pattern}"
    case = jf.make_case(J, F, T, B, pattern)
    for k in ("x0", "mean", "std", "target", "weight", "scale", "lengths"):
        assert np.array_equal(case[k], g[f"{key}|{k}"]), k                 # the seeded inputs are the recorded ones
    own = jf.evaluate(case, torch.float64)
    for k in ("pos", "logp", "grad"):
        ref = g[f"{key}|{k}"]
        assert ref.dtype == np.float64 and own[k].shape == ref.shape
        gap = jf.distance(own[k], ref)
        print(f"\n{key} {k}: {gap:.3e}")
        assert gap <= 1e-12, (k, gap)
    assert np.abs(g[f"{key}|grad"]).max() > 0


@pytest.mark.parametrize("J,F,T,B,pattern", [(2, 7, 5, 1, "dense"), (22, 263, 7, 3, "late_joint"), (21, 190, 9, 3, "dense"),
                                             (22, 263, 12, 3, "root_xz")])
def test_gradient_equals_central_differences(J, F, T, B, pattern):
    """float64, eps = 1e-5: truncation (third derivatives of sin / cos times eps^2) and round-off (1e-16 / eps) are both below 1e-9 of
    the largest gradient entry; the bar is 1e-6.  Every coordinate of the smallest case, 64 seeded ones of the others -- the read
    channels and a few unread ones."""
    case = jf.make_case(J, F, T, B, pattern)
    grad = jf.evaluate(case, torch.float64)["grad"]
    t = {k: torch.from_numpy(case[k]).double() for k in ("x0", "mean", "std", "target", "weight", "scale")}
    n = grad.size
    rng = np.random.default_rng(J * 1000 + T)
    read = 4 + 3 * (J - 1)
    if n <= 64:
        picks = np.arange(n)
    else:
        b, f, tt = rng.integers(0, B, 64), np.concatenate([rng.integers(0, read, 56), rng.integers(0, F, 8)]), rng.integers(0, T, 64)
        picks = (b * F + f) * T + tt
    eps, worst = 1e-5, 0.0
    with torch.no_grad():
        for i in picks:
            vals = []
            for sgn in (1.0, -1.0):
                x = t["x0"].clone()
                x.view(-1)[i] += sgn * eps
                vals.append(float(jf.log_prob(x, t["mean"], t["std"], J, t["target"], t["weight"], t["scale"], case["lengths"])[0].sum()))
            worst = max(worst, abs((vals[0] - vals[1]) / (2 * eps) - grad.reshape(-1)[i]))
    rel = worst / np.abs(grad).max()
    print(f"\n{J} joints, {T} frames, {pattern}: worst |autograd - central difference| / max |grad| = {rel:.2e}")
    assert rel <= 1e-6


def test_structure_of_the_gradient():
    """What the kernel must reproduce exactly, shown on the yardstick: unread channels, padded frames and -- with one constraint in the
    last valid frame -- the velocity channels from that frame on carry no gradient."""
    J, F, T, B = 22, 263, 7, 3
    case = jf.make_case(J, F, T, B, "late_joint")
    g = jf.evaluate(case, torch.float64)["grad"]
    assert not g[:, 4 + 3 * (J - 1):].any()
    for b, n in enumerate(case["lengths"]):
        assert not g[b, :, :, n:].any() and not g[b, :3, :, n - 1:].any()
        if n > 1:
            assert g[b, :3, :, :n - 1].any()
    assert not jf.evaluate(jf.make_case(J, F, T, B, "zero"), torch.float64)["grad"].any()


# ------------------------------------------------------------------------------ the builders
def test_keyframes_builder():
    from mst_amd.diffusion.guidance import JointGuide
    tgt, w = JointGuide.keyframes((2, 10, 22), joints=[20, 0], frames=[4, 9], positions=[[1, 2, 3], [4, 5, 6]], weight=[2.0, 0.5])
    assert tgt.shape == w.shape == (2, 10, 22, 3) and tgt.dtype == w.dtype == torch.float32
    assert torch.equal(tgt[:, 4, 20], torch.tensor([[1., 2, 3]] * 2)) and torch.equal(w[:, 4, 20], torch.full((2, 3), 2.0))
    assert torch.equal(tgt[1, 9, 0], torch.tensor([4., 5, 6])) and torch.equal(w[0, 9, 0], torch.full((3,), 0.5))
    assert int((w != 0).sum()) == 2 * 2 * 3 and int((tgt != 0).sum()) == 2 * 2 * 3
    # per clip, per axis
    tgt, w = JointGuide.keyframes((2, 10, 22), joints=[3], frames=[0], positions=[[1, 2, 3]], weight=[[1.0, 0.0, 1.0]], clips=[1])
    assert not w[0].any() and torch.equal(w[1, 0, 3], torch.tensor([1.0, 0.0, 1.0]))
    tgt, w = JointGuide.keyframes((1, 4, 2), [], [], np.zeros((0, 3)))
    assert not w.any()
    for bad in (dict(joints=[22], frames=[0]), dict(joints=[0], frames=[10]), dict(joints=[0, 1], frames=[0])):
        with pytest.raises(ValueError, match="JointGuide.keyframes"):
            JointGuide.keyframes((2, 10, 22), positions=np.zeros((len(bad["joints"]), 3)), **bad)
    with pytest.raises(ValueError, match="weight must be >= 0"):
        JointGuide.keyframes((2, 10, 22), [0], [0], [[0, 0, 0]], weight=-1.0)


def test_root_path_builder():
    from mst_amd.diffusion.guidance import JointGuide
    xz = np.stack([np.arange(6), -np.arange(6)], axis=1).astype(np.float32)
    tgt, w = JointGuide.root_path((2, 6, 22), xz, weight=3.0, lengths=[6, 4])
    assert tgt.shape == w.shape == (2, 6, 22, 3)
    assert torch.equal(tgt[1, :, 0, 0], torch.arange(6.)) and torch.equal(tgt[0, :, 0, 2], -torch.arange(6.))
    assert not tgt[:, :, 0, 1].any() and not tgt[:, :, 1:].any()
    assert torch.equal(w[0, :, 0, 0], torch.full((6,), 3.0)) and torch.equal(w[1, :, 0, 2], torch.tensor([3., 3, 3, 3, 0, 0]))
    assert not w[:, :, 0, 1].any() and not w[:, :, 1:].any()
    _, w = JointGuide.root_path((2, 6, 22), np.zeros((2, 6, 2)), weight=np.arange(6.))
    assert torch.equal(w[1, :, 0, 0], torch.arange(6.))
    with pytest.raises(ValueError, match="JointGuide.root_path: xz"):
        JointGuide.root_path((2, 6, 22), np.zeros((5, 2)))


# ------------------------------------------------------------------------------ names and signatures
def test_signatures_are_the_reference_s_and_public_names():
    import ctypes as C
    from mst_amd import _native as N
    from mst_amd import engine
    from mst_amd.diffusion.gaussian_diffusion import GaussianDiffusion as G
    from mst_amd.diffusion.guidance import JointGuide
    assert list(inspect.signature(G.p_sample_with_grad).parameters) == REF_P_SAMPLE_WITH_GRAD
    assert list(inspect.signature(G.ddim_sample_with_grad).parameters) == REF_DDIM_SAMPLE_WITH_GRAD
    assert list(inspect.signature(G.condition_mean_with_grad).parameters) == REF_CONDITION_WITH_GRAD
    assert list(inspect.signature(G.condition_score_with_grad).parameters) == REF_CONDITION_WITH_GRAD
    p = inspect.signature(G.ddim_sample_with_grad).parameters
    assert (p["clip_denoised"].default, p["cond_fn"].default, p["eta"].default, p["pred_xstart_in_graph"].default) == (True, None, 0.0, False)
    assert inspect.signature(G.condition_score_with_grad).parameters["model_kwargs"].default is None
    assert list(inspect.signature(JointGuide.__init__).parameters) == ["self", "target", "weight", "mean", "std", "n_joints", "scale", "lengths"]
    assert list(inspect.signature(JointGuide.__call__).parameters) == ["self", "x", "t", "p_mean_var", "model_kwargs"]
    assert list(inspect.signature(engine.joint_guide).parameters) == ["x0", "mean", "std", "joints", "target", "weight", "scale", "lengths",
                                                                      "want_positions"]
    for name in ("mst_joint_guide", "mst_joint_guide_max_frames"):
        assert name in N.SIGNATURES
    assert len(N.SIGNATURES["mst_joint_guide"][1]) == 15 and N.SIGNATURES["mst_joint_guide_max_frames"] == (C.c_int, [])


def test_condition_with_grad_arithmetic_and_the_unscaled_t():
    """The two torch-op forms against the reference's statements (:478-482, :518-530): the cond_fn receives (x, t, p_mean_var) with the
    respaced index t itself, not timestep_map[t]."""
    d = diffusion("ddim20")
    rng = np.random.default_rng(3)
    f = lambda: torch.from_numpy(rng.standard_normal((2, 5, 1, 4)).astype(np.float32))
    x, pred, mean, g = f(), f(), f(), f()
    t = torch.tensor([7, 3])
    pmv = {"mean": mean, "variance": torch.full_like(x, 0.25), "log_variance": torch.zeros_like(x), "pred_xstart": pred}
    seen = []

    def cond_fn(xx, tt, p, **kw):
        seen.append((xx, tt, p, kw))
        return g

    out = d.condition_mean_with_grad(cond_fn, pmv, x, t, model_kwargs={"y": {"a": 1}})
    assert torch.equal(out, mean + 0.25 * g)
    assert seen[0][0] is x and seen[0][1] is t and seen[0][2] is pmv and seen[0][3] == {"y": {"a": 1}}
    sc = d.condition_score_with_grad(cond_fn, pmv, x, t)
    ab = torch.from_numpy(d.alphas_cumprod)[t].float().view(2, 1, 1, 1)
    eps = d._predict_eps_from_xstart(x, t, pred) - (1 - ab).sqrt() * g
    want = d._predict_xstart_from_eps(x, t, eps)
    assert torch.equal(sc["pred_xstart"], want) and torch.equal(sc["mean"], d.q_posterior_mean_variance(want, x, t)[0])
    assert pmv["pred_xstart"] is pred and seen[1][1] is t                       # the caller's dict is left as it was


# ------------------------------------------------------------------------------ refusals that need no device
def test_joint_guide_refusals():
    from mst_amd import engine
    from mst_amd.diffusion.guidance import JointGuide
    B, T, J, F = 2, 6, 22, 263
    y, w = torch.zeros(B, T, J, 3), torch.ones(B, T, J, 3)
    mean, std = torch.zeros(F), torch.ones(F)
    with pytest.raises(ValueError, match=r"target must be \[B, T, 22, 3\]"):
        JointGuide(torch.zeros(B, T, 21, 3), w, mean, std, J)
    with pytest.raises(ValueError, match="is not target's shape"):
        JointGuide(y, torch.ones(B, T, J, 1), mean, std, J)
    with pytest.raises(ValueError, match="weight must be >= 0"):
        JointGuide(y, -w, mean, std, J)
    with pytest.raises(ValueError, match="cannot hold 22 joints"):
        JointGuide(y, w, torch.zeros(66), torch.ones(66), J)
    with pytest.raises(ValueError, match="scale values for 2 clips"):
        JointGuide(y, w, mean, std, J, scale=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="lengths for 2 clips"):
        JointGuide(y, w, mean, std, J, lengths=[6])
    with pytest.raises(ValueError, match=r"lengths must be in 0\.\.6"):
        JointGuide(y, w, mean, std, J, lengths=[6, 7])
    guide = JointGuide(y, w, mean, std, J, scale=2.0, lengths=[6, 3])
    for shape in ((B, F, 1, T + 1), (B + 1, F, 1, T), (B, F - 1, 1, T), (B, F, T)):
        with pytest.raises(ValueError, match="JointGuide: x0 .* is not"):
            guide.log_prob_grad(torch.zeros(shape))
    with pytest.raises(RuntimeError, match="joint_guide: x0: the engine needs a GPU tensor"):      # no torch-op fallback
        engine.joint_guide(torch.zeros(B, F, 1, T), mean, std, J, y, w, 1.0)


def test_sampler_refusals():
    from mst_amd.diffusion.guidance import JointGuide, TargetGuide
    d = diffusion("ddim20")
    x, t = torch.zeros(1, 4, 1, 4), torch.zeros(1, dtype=torch.long)
    model = lambda *a, **k: x
    cond = lambda *a, **k: x
    for fn in (d.p_sample_with_grad, d.ddim_sample_with_grad):
        with pytest.raises(AssertionError, match="denoised_fn is not supported"):
            fn(model, x, t, denoised_fn=lambda v: v)
        with pytest.raises(NotImplementedError, match="cond_fn together with pred_xstart_in_graph"):
            fn(model, x, t, cond_fn=cond, pred_xstart_in_graph=True)
        with pytest.raises(ValueError, match="a TargetGuide is a cond_fn of"):
            fn(model, x, t, cond_fn=TargetGuide(x))
        cfg = types.SimpleNamespace(is_cfg_sampler=True, model=model)
        with pytest.raises(NotImplementedError, match="ClassifierFreeSampleModel"):
            fn(cfg, x, t, cond_fn=cond)
        with pytest.raises(AssertionError, match="runs on the GPU only"):
            fn(model, x, t, cond_fn=cond)
    with pytest.raises(NotImplementedError, match="cond_fn together with pred_xstart_in_graph"):
        d.ddim_sample_loop(model, (1, 4, 1, 4), noise=x, device="cpu", cond_fn=cond, cond_fn_with_grad=True, pred_xstart_in_graph=True)
    with pytest.raises(AssertionError, match="runs on the GPU only"):       # the loop no longer drops the cond_fn
        d.p_sample_loop(model, (1, 4, 1, 4), noise=x, device="cpu", cond_fn=cond, cond_fn_with_grad=True)
    assert JointGuide is not None
