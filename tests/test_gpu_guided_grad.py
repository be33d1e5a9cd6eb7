"""With-grad guided sampling on the GPU: p_sample_with_grad / ddim_sample_with_grad and the loops with cond_fn_with_grad=True, guided by
diffusion.guidance.JointGuide through the native training node, against the same steps on a torch-ops copy of the model
(tests/torch_reference.py) driven by the fixture's likelihood written in torch (tests/joint_guide_fixture.py).

The model is test_gpu_train.py's StyleDiffusion (181 features: 20 joints of the position-rotation row), seeded weights, eval mode,
trainable parameters; B = 2, T = 24, "ddim20" respacing.  Bars: the gradient with respect to x, TOL_GRAD = 1.5e-3 relative L2
(test_gpu_train.py's bar for this node); the sample, TOL_FWD = 1e-3; the returned pred_xstart bit-equal to the unguided with-grad
step's.  Every comparison prints its figure.

Measured on an MI355X (plain / inpainting + clamp): gradient with respect to x against the torch-ops model 1.20e-3 / 5.6e-4 for all
three samplers (the native node's own f16-operand error); a Python cond_fn through the native node against JointGuide 1.6e-4 / 3.2e-4;
sample 4.6e-4 / 1.3e-4 (ancestral), 3.0e-4 / 7.5e-5 (DDIM), 3.6e-4 / 9.1e-5 (DDIM eta 0.5); the guide moves a step by 0.24 .. 0.39 /
0.11 .. 0.18 of its norm, four guided steps end 6.3e-3 (ancestral) and 1.8e-2 (DDIM) from the unguided loops.  The file takes 6 s."""
import numpy as np
import pytest
import torch

import joint_guide_fixture as jf
import mst_amd  # noqa: F401
from conftest import rel_l2
from mst_amd import synthetic as syn
from torch_reference import use_torch_ops

pytestmark = pytest.mark.gpu

TOL_FWD = 1e-3
TOL_GRAD = 1.5e-3
B, F, T, J = 2, 181, 24, 20
SHAPE = (B, F, 1, T)
LENGTHS = (24, 17)
SAMPLERS = (("ddpm", None), ("ddim", 0.0), ("ddim", 0.5))
SCALE = (40.0, 25.0)


def dev():
    return torch.device("cuda")


def cu(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=dev(), dtype=dtype)


def style_model():
    from mst_amd.model.mdm_forstyledataset import StyleDiffusion
    m = StyleDiffusion("", F, 1, 1, True, "rot6d", True, True, latent_dim=512, ff_size=1024, num_layers=8, num_heads=4, dropout=0.1,
                       activation="gelu", data_rep="hml_vec", cond_mode="text", cond_mask_prob=0.0, arch="trans_enc",
                       dataset="stylexia_posrot")
    sd = {k: torch.from_numpy(syn.tensor_for(3, k, tuple(v.shape)).copy()) for k, v in m.state_dict().items()
          if not k.endswith(".pe") and "clip_model" not in k}
    m.load_state_dict(sd, strict=False)
    return m.to(dev()).eval()


def diffusion(inpainting):
    from mst_amd.diffusion import gaussian_diffusion as gd
    from mst_amd.diffusion.inpainting_gaussian_diffusion import InpaintingGaussianDiffusion
    from mst_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    cls = InpaintingGaussianDiffusion if inpainting else SpacedDiffusion
    return cls(use_timesteps=space_timesteps(1000, "ddim20"), betas=gd.get_named_beta_schedule("cosine", 1000),
               model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE)


@pytest.fixture(scope="module")
def ctx():
    """Two models with the same seeded weights (native, torch ops), the guide's operands and the inputs of every test."""
    case = jf.make_case(J, F, T, B, "dense", seed=jf.SEED + 1)
    case["lengths"] = np.asarray(LENGTHS, np.int32)
    # The guide's strength.  A guided sample is the unguided one plus a multiple of the cond_fn's gradient, so its error is the
    # unguided step's (1e-4) plus TOL_GRAD times the share of the guide term: held to TOL_FWD it needs that share below about half
    # of the sample.  Under the clamp and the inpainting mask most of the gradient is cut (|x0-hat| > 1, rows 0-2) and SCALE moves a
    # step by a tenth of its norm; without either the whole gradient passes and SCALE / 40 moves it by a few tenths.
    case["scale"] = np.asarray(SCALE, np.float32)
    from mst_amd.diffusion.guidance import JointGuide
    guide = JointGuide(case["target"], case["weight"], case["mean"], case["std"], J, scale=case["scale"])
    soft = JointGuide(case["target"], case["weight"], case["mean"], case["std"], J, scale=case["scale"] / 40)
    ops = {k: cu(case[k]) for k in ("mean", "std", "target", "weight", "scale")}
    lengths = cu(case["lengths"], torch.int32)

    def torch_cond_for(scale):
        def torch_cond(x, t, p_mean_var, **kw):
            """The fixture's likelihood in torch ops on x0-hat, then autograd to x: a plain Python with-grad cond_fn."""
            logp, _ = jf.log_prob(p_mean_var["pred_xstart"], ops["mean"], ops["std"], J, ops["target"], ops["weight"], scale,
                                  kw["y"]["lengths"])
            return torch.autograd.grad(logp.sum(), x)[0]
        return torch_cond

    y = {"text_embed": cu(syn.normal(3, "gg/emb", (B, 512))), "lengths": lengths}
    pair = dict(y, inpainting_mask=cu(syn.root_horizontal_mask(B, F, T)), inpainted_motion=cu(syn.normal(3, "gg/motion", SHAPE)))
    c = dict(native=style_model(), torch=use_torch_ops(style_model()), guide=guide, torch_cond=torch_cond_for(ops["scale"]), guide_soft=soft,
             torch_cond_soft=torch_cond_for(ops["scale"] / 40), case=case,
             x=cu(syn.normal(3, "gg/x", SHAPE)), t=torch.tensor([12, 5], device=dev()), plain={"y": y}, pair={"y": pair})
    # the unguided with-grad loops, BEFORE any guided call of this module (test_unguided_loops_are_untouched)
    c["before"] = unguided_loops(c)
    return c


def unguided_loops(c):
    out = {}
    for name in ("p_sample_loop", "ddim_sample_loop"):
        d = diffusion(True)
        torch.manual_seed(11)
        steps = list(getattr(d, name + "_progressive")(c["native"], SHAPE, noise=c["x"], model_kwargs=c["pair"], skip_timesteps=16,
                                                       init_image=c["pair"]["y"]["inpainted_motion"], cond_fn_with_grad=True))
        out[name] = [(s["sample"].detach().clone(), s["pred_xstart"].detach().clone()) for s in steps]
    return out


class Spy:
    """A cond_fn that keeps what it returned."""

    def __init__(self, fn):
        self.fn, self.g, self.seen = fn, None, None

    def __call__(self, x, t, p_mean_var, **kw):
        self.seen = (x, t, p_mean_var, kw)
        self.g = self.fn(x, t, p_mean_var, **kw).detach().clone()
        return self.g


def step(d, smp, eta, model, c, kw, clip, cond_fn=None, seed=5):
    torch.manual_seed(seed)
    if smp == "ddpm":
        return d.p_sample_with_grad(model, c["x"], c["t"], clip_denoised=clip, cond_fn=cond_fn, model_kwargs=kw)
    return d.ddim_sample_with_grad(model, c["x"], c["t"], clip_denoised=clip, cond_fn=cond_fn, model_kwargs=kw, eta=eta)


def open_nodes(model):
    """Native nodes that announced parameter gradients to the model's gradient sink (an unguided with-grad step does; its count stays
    when no backward pass follows)."""
    sink = model.__dict__.get("_mst_grad_sink")
    return 0 if sink is None else sink.open_nodes


def grads_untouched(model, announced):
    """3: every parameter still trainable and without a gradient, no backward pass of the sink begun, no node that announced one."""
    ps = [p for p in model.parameters() if p.requires_grad]
    assert len(ps) >= 96 and all(p.grad is None for p in ps)
    sink = model.__dict__.get("_mst_grad_sink")
    assert (sink is None or not sink.active) and open_nodes(model) == announced


@pytest.mark.parametrize("inpaint", [False, True], ids=["plain", "inpaint+clamp"])
@pytest.mark.parametrize("smp,eta", SAMPLERS)
def test_guided_step_native_vs_torch_ops(ctx, smp, eta, inpaint):
    """1-3: JointGuide through the native node against the fixture's cond_fn through the torch-ops model, the same cond_fn through the
    native node, the unguided step's pred_xstart, and the parameters' .grad."""
    c = ctx
    d = diffusion(inpaint)
    kw, clip = (c["pair"], True) if inpaint else (c["plain"], False)
    guide, cond = (c["guide"], c["torch_cond"]) if inpaint else (c["guide_soft"], c["torch_cond_soft"])
    a, b, p = Spy(guide), Spy(cond), Spy(cond)
    announced = open_nodes(c["native"])
    native = step(d, smp, eta, c["native"], c, kw, clip, a)
    grads_untouched(c["native"], announced)
    ref = step(d, smp, eta, c["torch"], c, kw, clip, b)
    python = step(d, smp, eta, c["native"], c, kw, clip, p)
    grads_untouched(c["native"], announced)
    plain = step(d, smp, eta, c["native"], c, kw, clip, None)
    # what the cond_fn saw: x requiring grad, the respaced index itself, pred_xstart in x's graph, constants beside it
    x, t, pmv, seen_kw = a.seen
    assert x.requires_grad and torch.equal(x.detach(), c["x"]) and t is c["t"] and seen_kw.keys() == kw.keys()
    assert set(pmv) == {"mean", "variance", "log_variance", "pred_xstart"} and pmv["pred_xstart"].requires_grad and pmv["mean"].requires_grad
    assert not pmv["variance"].requires_grad and not pmv["log_variance"].requires_grad
    assert torch.equal(pmv["pred_xstart"].detach(), plain["pred_xstart"])
    e_grad = rel_l2(a.g.cpu().numpy(), b.g.cpu().numpy())
    e_py = rel_l2(p.g.cpu().numpy(), a.g.cpu().numpy())
    e_fwd = rel_l2(native["sample"].cpu().numpy(), ref["sample"].cpu().numpy())
    moved = rel_l2(native["sample"].cpu().numpy(), plain["sample"].detach().cpu().numpy())      # (the unguided sample is in x0-hat's graph)
    print(f"\nguided {smp} eta {eta} {'inpaint+clamp' if inpaint else 'plain'}: grad wrt x vs torch ops {e_grad:.2e} (bar {TOL_GRAD}), "
          f"python cond_fn vs JointGuide {e_py:.2e}, sample {e_fwd:.2e} (bar {TOL_FWD}); guided vs unguided sample {moved:.2e}")
    assert float(a.g.abs().max()) > 0 and torch.isfinite(a.g).all()
    assert e_grad <= TOL_GRAD and e_py <= TOL_GRAD and e_fwd <= TOL_FWD
    assert torch.equal(native["pred_xstart"], plain["pred_xstart"]) and not native["pred_xstart"].requires_grad
    assert not native["sample"].requires_grad and moved > 0, "the step dropped its cond_fn"
    if inpaint:                                   # the blend cuts the masked rows from the model: x0-hat there is the motion, bit for bit
        assert torch.equal(native["pred_xstart"][:, :3], kw["y"]["inpainted_motion"][:, :3].clamp(-1, 1))
        assert float(native["pred_xstart"].abs().max()) <= 1.0


@pytest.mark.parametrize("name", ["p_sample_loop", "ddim_sample_loop"])
def test_guided_loops_equal_the_python_loop_and_differ_from_unguided(ctx, name):
    """4: four steps with cond_fn_with_grad=True, the loop entry and its progressive form, against p_sample_with_grad /
    ddim_sample_with_grad called step by step under the same seed, bit for bit; and not the unguided loop's result."""
    c = ctx
    d = diffusion(True)
    kw, init = c["pair"], c["pair"]["y"]["inpainted_motion"]
    announced = open_nodes(c["native"])
    args = dict(noise=c["x"], model_kwargs=kw, skip_timesteps=16, init_image=init, cond_fn_with_grad=True)
    torch.manual_seed(11)
    whole = getattr(d, name)(c["native"], SHAPE, cond_fn=c["guide"], **args)
    torch.manual_seed(11)
    prog = list(getattr(d, name + "_progressive")(c["native"], SHAPE, cond_fn=c["guide"], **args))
    torch.manual_seed(11)
    img = d.q_sample(init, torch.full((B,), 3, device=dev(), dtype=torch.long), c["x"], model_kwargs=kw)
    one = d.ddim_sample_with_grad if name.startswith("ddim") else d.p_sample_with_grad
    for k, i in enumerate((3, 2, 1, 0)):
        out = one(c["native"], img, torch.full((B,), i, device=dev(), dtype=torch.long), cond_fn=c["guide"], model_kwargs=kw)
        assert torch.equal(out["sample"], prog[k]["sample"]) and torch.equal(out["pred_xstart"], prog[k]["pred_xstart"]), (name, i)
        img = out["sample"]
    assert len(prog) == 4 and torch.equal(whole, img)
    plain = c["before"][name][-1][0]
    moved = rel_l2(whole.cpu().numpy(), plain.cpu().numpy())
    print(f"\n{name}: guided vs unguided after 4 steps {moved:.2e}")
    assert not torch.equal(whole, plain) and moved > 0, "the loop dropped its cond_fn"
    grads_untouched(c["native"], announced)


def test_unguided_loops_are_untouched(ctx):
    """5: with cond_fn=None the with-grad loops give, after everything above, the bits they gave before any guided call."""
    after = unguided_loops(ctx)
    for name, steps in ctx["before"].items():
        assert len(steps) == len(after[name]) == 4
        for (s0, p0), (s1, p1) in zip(steps, after[name]):
            assert torch.equal(s0, s1) and torch.equal(p0, p1), name


def test_refusals(ctx):
    """6."""
    from mst_amd.diffusion.guidance import JointGuide, TargetGuide
    from mst_amd.model.cfg_sampler import ClassifierFreeSampleModel
    c = ctx
    d = diffusion(False)
    announced = open_nodes(c["native"])
    m = style_model()
    m.cond_mask_prob = 0.1
    cfg = ClassifierFreeSampleModel(m)
    kw = {"y": dict(c["plain"]["y"], scale=torch.full((B,), 2.5, device=dev()))}
    for fn in (d.p_sample_with_grad, d.ddim_sample_with_grad):
        with pytest.raises(NotImplementedError, match="with-grad cond_fn on a ClassifierFreeSampleModel"):
            fn(cfg, c["x"], c["t"], cond_fn=c["guide"], model_kwargs=kw)
        with pytest.raises(NotImplementedError, match="cond_fn together with pred_xstart_in_graph"):
            fn(c["native"], c["x"], c["t"], cond_fn=c["guide"], model_kwargs=c["plain"], pred_xstart_in_graph=True)
        with pytest.raises(AssertionError, match="denoised_fn is not supported"):
            fn(c["native"], c["x"], c["t"], cond_fn=c["guide"], denoised_fn=lambda v: v, model_kwargs=c["plain"])
        with pytest.raises(ValueError, match="a TargetGuide is a cond_fn of"):
            fn(c["native"], c["x"], c["t"], cond_fn=TargetGuide(c["x"]), model_kwargs=c["plain"])
    with pytest.raises(NotImplementedError, match="with-grad cond_fn on a ClassifierFreeSampleModel"):
        d.ddim_sample_loop(cfg, SHAPE, noise=c["x"], cond_fn=c["guide"], model_kwargs=kw, cond_fn_with_grad=True, skip_timesteps=19)
    case = c["case"]
    # a guide that does not fit the step: other frame count, other clip count, other joint count for the features, bad lengths
    short = JointGuide(case["target"][:, :20], case["weight"][:, :20], case["mean"], case["std"], J)
    with pytest.raises(ValueError, match="JointGuide: x0 .* is not"):
        d.p_sample_with_grad(c["native"], c["x"], c["t"], cond_fn=short, model_kwargs=c["plain"])
    one = JointGuide(case["target"][:1], case["weight"][:1], case["mean"], case["std"], J)
    with pytest.raises(ValueError, match="JointGuide: x0 .* is not"):
        d.ddim_sample_with_grad(c["native"], c["x"], c["t"], cond_fn=one, model_kwargs=c["plain"])
    wide = JointGuide(case["target"], case["weight"], np.zeros(263, np.float32), np.ones(263, np.float32), J)
    with pytest.raises(ValueError, match="JointGuide: x0 .* is not"):
        d.p_sample_with_grad(c["native"], c["x"], c["t"], cond_fn=wide, model_kwargs=c["plain"])
    bad = {"y": dict(c["plain"]["y"], lengths=torch.tensor([24, 17, 3], device=dev()))}
    with pytest.raises(ValueError, match="3 lengths for 2 clips"):
        d.p_sample_with_grad(c["native"], c["x"], c["t"], cond_fn=c["guide"], model_kwargs=bad)
    grads_untouched(c["native"], announced)
