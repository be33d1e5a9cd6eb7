"""The operand contract on the GPU (DESIGN.md section 1 "Drop-in boundary"; host logic in tests/test_operand_contract_cpu.py).

Accepted: every non-canonical form of an operand the contract takes -- bool and float64 masks, a noise mask that broadcasts, a
one-element guidance scale, a non-contiguous model output -- gives BIT-identical results to the same call with the operand expanded,
cast and made contiguous beforehand.  Refused: the forms the reference's own assert (gaussian_diffusion.py:344) or torch's broadcast
refuses raise the same error class through the mirror's public methods, before anything is launched.

Shapes: Xia (181, 76) with B = 3 and (150, 61) with B = 2, "ddim20", 3-step loops."""
import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
import mst_amd.synthetic as syn
from mst_amd.engine import SAMPLER_DDIM, SAMPLER_DDIM_REVERSE, SAMPLER_DDPM, DenoiserEngine, Schedule

pytestmark = pytest.mark.gpu
SEED = 9117
SHAPES = [(181, 76, 3), (150, 61, 2)]
IDS = ["xia181x76_B3", "150x61_B2"]


def dev():
    return torch.device("cuda:0")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


_CACHE = {}


def schedule_ddim20():
    if "sch" not in _CACHE:
        from oracle import schedule
        tab, tmap = schedule.make("cosine", 1000, "ddim20")
        _CACHE["sch"] = Schedule(tab, tmap, dev())
    return _CACHE["sch"]


def engine(F, T, B):
    key = (F, T, B)
    if key not in _CACHE:
        eng = DenoiserEngine(F, T, 2 * B, device=dev())
        w = syn.denoiser_state(SEED, F)
        eng.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, pe=torch.from_numpy(syn.positional_table(5000, 512)))
        _CACHE[key] = eng
    return _CACHE[key]


def data(F, T, B):
    shape = (B, F, 1, T)
    d = {k: cu(syn.normal(SEED, f"oc/{k}/{F}", shape)) for k in ("out", "x", "noise", "motion")}
    d["mask"] = cu(syn.root_horizontal_mask(B, F, T))
    d["t"] = torch.tensor([0, 19, 7][:B], device=dev())
    rows = (syn.uniform(SEED, f"oc/rows/{F}", (1, F, 1, T), 0.0, 1.0) > 0.5).astype(np.float32)       # [1, F, 1, T]
    frames = (syn.uniform(SEED, f"oc/frames/{F}", (B, 1, 1, T), 0.0, 1.0) > 0.3).astype(np.float32)   # [B, 1, 1, T]
    d["noise_masks"] = {"1F1T": cu(rows), "B11T": cu(frames), "BF11": cu(rows[..., :1].repeat(B, 0)), "T": cu(frames[0, 0, 0])}
    return shape, d


def canon(v, shape):
    return v.to(torch.float32).expand(shape).contiguous()


def same(a, b):
    for u, v in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert torch.equal(u, v)


STEPS = [(SAMPLER_DDPM, 0.0), (SAMPLER_DDIM, 0.5), (SAMPLER_DDIM_REVERSE, 0.0)]
STEP_IDS = ["ddpm", "ddim_eta0.5", "reverse"]


@pytest.mark.parametrize("F,T,B", SHAPES, ids=IDS)
@pytest.mark.parametrize("sampler,eta", STEPS, ids=STEP_IDS)
def test_step_accepts_every_form_bit_for_bit(F, T, B, sampler, eta):
    shape, d = data(F, T, B)
    sch = schedule_ddim20()
    noise = None if sampler == SAMPLER_DDIM_REVERSE else d["noise"]
    base = sch.step(d["out"], d["x"], d["t"], noise, sampler, eta, mask=d["mask"], motion=d["motion"], mask_noise=True)
    # the inpainting pair: bool and float64 masks, a float64 motion, a model output that is a permuted view
    strided = d["out"].permute(0, 3, 2, 1).contiguous().permute(0, 3, 2, 1)
    assert not strided.is_contiguous() and torch.equal(strided, d["out"])
    for form, kw in (("bool", dict(mask=d["mask"] > 0.5)), ("float64", dict(mask=d["mask"].double())),
                     ("float64 motion", dict(motion=d["motion"].double())), ("strided output", dict(out=strided))):
        a = dict(out=d["out"], mask=d["mask"], motion=d["motion"])
        a.update(kw)
        same(sch.step(a["out"], d["x"], d["t"], noise, sampler, eta, mask=a["mask"], motion=a["motion"], mask_noise=True), base)
    if sampler == SAMPLER_DDIM_REVERSE:
        return                                     # no noise term: no noise mask
    # a noise mask alone (no motion) in every shape that broadcasts to the noise
    for form, m in d["noise_masks"].items():
        want = sch.step(d["out"], d["x"], d["t"], noise, sampler, eta, mask=canon(m, shape), mask_noise=True)
        same(sch.step(d["out"], d["x"], d["t"], noise, sampler, eta, mask=m, mask_noise=True), want)
        same(sch.step(d["out"], d["x"], d["t"], noise, sampler, eta, mask=m > 0.5, mask_noise=True), want)
    t_pos = torch.clamp(d["t"], min=1)             # (the noise term is switched off at index 0: make sure a mask matters somewhere)
    free = sch.step(d["out"], d["x"], t_pos, noise, sampler, eta)
    masked = sch.step(d["out"], d["x"], t_pos, noise, sampler, eta, mask=d["noise_masks"]["B11T"], mask_noise=True)
    assert not torch.equal(free[0], masked[0]) and torch.equal(free[1], masked[1])


@pytest.mark.parametrize("F,T,B", SHAPES, ids=IDS)
def test_q_sample_accepts_every_form_bit_for_bit(F, T, B):
    shape, d = data(F, T, B)
    sch = schedule_ddim20()
    free = sch.q_sample(d["motion"], d["t"], d["noise"])
    for form, m in dict(d["noise_masks"], full=d["mask"]).items():
        want = sch.q_sample(d["motion"], d["t"], d["noise"], canon(m, shape))
        assert not torch.equal(want, free)
        same(sch.q_sample(d["motion"], d["t"], d["noise"], m), want)
        same(sch.q_sample(d["motion"], d["t"], d["noise"], m > 0.5), want)
        same(sch.q_sample(d["motion"], d["t"], d["noise"], m.double()), want)
    same(sch.q_sample(d["motion"].double(), d["t"], d["noise"].permute(0, 3, 2, 1).contiguous().permute(0, 3, 2, 1), d["mask"]),
         sch.q_sample(d["motion"], d["t"], d["noise"], d["mask"]))


@pytest.mark.parametrize("F,T,B", SHAPES, ids=IDS)
def test_forward_and_loop_with_a_one_element_scale(F, T, B):
    shape, d = data(F, T, B)
    eng, sch = engine(F, T, B), schedule_ddim20()
    eng.set_text(cu(syn.normal(SEED, "oc/txt", (B, 512))), cfg=True)
    full = torch.full((B,), 2.5, device=dev())
    want = eng.forward(d["x"], d["t"], scale=full, cfg=True)
    for form, s in (("[1]", torch.tensor([2.5], device=dev())), ("0-dim", torch.tensor(2.5, device=dev())), ("float", 2.5),
                    ("[B,1,1,1] float64", full.double().view(-1, 1, 1, 1)), ("host", torch.tensor([2.5]))):
        same(eng.forward(d["x"], d["t"], scale=s, cfg=True), want)
    assert not torch.equal(want, eng.forward(d["x"], d["t"], scale=torch.full((B,), 1.0, device=dev()), cfg=True))
    with pytest.raises(ValueError, match=rf"scale: {B + 1} values for {B} clips"):
        eng.forward(d["x"], d["t"], scale=torch.ones(B + 1, device=dev()), cfg=True)
    # 3-step loops: CFG with a [1] scale, bool / float64 pair, a broadcast noise mask alone
    nz = cu(np.stack([syn.normal(SEED, f"oc/nz{k}/{F}", shape) for k in range(3)]))
    for sampler, eta in ((SAMPLER_DDPM, 0.0), (SAMPLER_DDIM, 0.5)):
        def loop(**kw):
            return eng.sample_loop(sch, d["x"].clone(), 2, 0, sampler, eta, cfg=True, noise=nz, **kw)
        want = loop(scale=full, mask=d["mask"], motion=d["motion"])
        same(loop(scale=torch.tensor([2.5], device=dev()), mask=d["mask"] > 0.5, motion=d["motion"]), want)
        same(loop(scale=2.5, mask=d["mask"].double(), motion=d["motion"].double()), want)
        for form in ("1F1T", "B11T"):
            m = d["noise_masks"][form]
            same(loop(scale=torch.tensor([2.5], device=dev()), mask=m), loop(scale=full, mask=canon(m, shape)))
    with pytest.raises(AssertionError, match="inpainting_mask"):
        eng.sample_loop(sch, d["x"].clone(), 2, 0, noise=nz, mask=d["noise_masks"]["1F1T"], motion=d["motion"])
    with pytest.raises(AssertionError, match="inpainted_motion"):
        eng.sample_loop(sch, d["x"].clone(), 2, 0, noise=nz, mask=d["mask"], motion=d["motion"][:1])


@pytest.mark.parametrize("F,T,B", SHAPES, ids=IDS)
@pytest.mark.parametrize("sampler,eta", STEPS[:2], ids=STEP_IDS[:2])
def test_fused_step_node_forward_and_backward(F, T, B, sampler, eta):
    from mst_amd.diffusion.fused_ops import FusedStepFn
    shape, d = data(F, T, B)
    sch = schedule_ddim20()
    ws, wp = cu(syn.normal(SEED, f"oc/ws/{F}", shape)), cu(syn.normal(SEED, f"oc/wp/{F}", shape))

    def run(mask, motion, clip):
        o = d["out"].clone().requires_grad_(True)
        s, p = FusedStepFn.apply(o, d["x"], d["t"], d["noise"], mask, motion, sch, sampler, eta, True, clip)
        ((s * ws).sum() + (p * wp).sum()).backward()
        return s.detach(), p.detach(), o.grad
    for clip in (False, True):
        want = run(d["mask"], d["motion"], clip)
        assert float(want[2][:, :3].abs().max()) == 0.0 and float(want[2].abs().max()) > 0.0
        same(run(d["mask"] > 0.5, d["motion"], clip), want)
        same(run(d["mask"].double(), d["motion"].double(), clip), want)
        for form in ("1F1T", "B11T"):
            m = d["noise_masks"][form]
            same(run(m, None, clip), run(canon(m, shape), None, clip))
    with pytest.raises(AssertionError, match="inpainting_mask"):
        run(d["noise_masks"]["1F1T"], d["motion"], False)


# ------------------------------------------------------------------------------------------ refused forms, through the mirror
def mirror():
    from mst_amd.diffusion import gaussian_diffusion as gd
    from mst_amd.diffusion.inpainting_gaussian_diffusion import InpaintingGaussianDiffusion
    from mst_amd.diffusion.respace import space_timesteps
    return InpaintingGaussianDiffusion(use_timesteps=space_timesteps(1000, "ddim20"), betas=gd.get_named_beta_schedule("cosine", 1000),
                                       model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL,
                                       loss_type=gd.LossType.MSE)


REFUSED = {   # operand form -> error class of the contract table
    "pair mask [1,F,1,T]": (lambda d, B: dict(inpainting_mask=d["noise_masks"]["1F1T"], inpainted_motion=d["motion"]), AssertionError),
    "pair mask [B,1,1,T]": (lambda d, B: dict(inpainting_mask=d["noise_masks"]["B11T"], inpainted_motion=d["motion"]), AssertionError),
    "one-clip motion": (lambda d, B: dict(inpainting_mask=d["mask"], inpainted_motion=d["motion"][:1]), AssertionError),
    "noise mask of another F": (lambda d, B: dict(inpainting_mask=torch.ones(B, d["x"].shape[1] + 1, 1, d["x"].shape[3], device=dev())),
                                RuntimeError),
    "noise mask of rank 5": (lambda d, B: dict(inpainting_mask=d["mask"][None]), RuntimeError),
}


@pytest.mark.parametrize("form", sorted(REFUSED))
@pytest.mark.parametrize("entry", ["p_sample", "ddim_sample", "p_sample_loop", "ddim_sample_with_grad"])
def test_refused_forms_raise_through_the_mirror(entry, form):
    F, T, B = SHAPES[1]
    shape, d = data(F, T, B)
    make_y, err = REFUSED[form]
    kwargs = {"y": make_y(d, B)}
    diff = mirror()
    calls = []

    def model(x, t, **kw):                       # any model callable: the steps run through the stand-alone kernels
        calls.append(1)
        return x * 0.5
    with pytest.raises(err):
        if entry == "p_sample":
            diff.p_sample(model, d["x"], d["t"], clip_denoised=False, model_kwargs=kwargs)
        elif entry == "ddim_sample":
            diff.ddim_sample(model, d["x"], d["t"], clip_denoised=False, model_kwargs=kwargs, eta=0.5)
        elif entry == "p_sample_loop":
            diff.p_sample_loop(model, shape, noise=d["x"], clip_denoised=False, model_kwargs=kwargs, device=dev(), skip_timesteps=17)
        else:
            diff.ddim_sample_with_grad(model, d["x"], d["t"], clip_denoised=False, model_kwargs=kwargs)
    assert len(calls) <= 1                       # refused at the first step, nothing ran on


def test_the_mirror_takes_a_broadcast_noise_mask():
    """What the reference's `noise *= 1. - y['inpainting_mask']` accepts runs, and equals the expanded mask bit for bit."""
    F, T, B = SHAPES[1]
    shape, d = data(F, T, B)
    diff = mirror()
    model = lambda x, t, **kw: x * 0.5
    m = d["noise_masks"]["B11T"]
    outs = []
    for mask in (m, canon(m, shape)):
        torch.manual_seed(3)
        a = diff.p_sample(model, d["x"], d["t"], clip_denoised=False, model_kwargs={"y": {"inpainting_mask": mask}})
        torch.manual_seed(3)
        q = diff.q_sample(d["motion"], d["t"], model_kwargs={"y": {"inpainting_mask": mask}})
        outs.append((a["sample"], a["pred_xstart"], q))
    same(outs[0], outs[1])
