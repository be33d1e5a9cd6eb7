"""The operand contract of the Python handles (engine._operand, DESIGN.md section 1 "Drop-in boundary") without a GPU.

The kernels behind Schedule.q_sample / step / step_guided, DenoiserEngine.forward / sample_loop and FusedStepFn read every operand as
base + i over B * per_clip elements (B for `scale`): whatever reaches the library must be a float32 contiguous tensor of exactly that
many elements.  Part one holds the helper's three rules; part two drives the entry points with the library replaced by a recording
stub (and the device check, which is separate from the shape logic, switched off) and checks every pointer handed over."""
import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
from mst_amd import engine as E
from lib_stub import install, stub_engine, stub_schedule

B, F, T = 3, 5, 7
SHAPE = (B, F, 1, T)


def _full(seed=0):
    return torch.randn(SHAPE, generator=torch.Generator().manual_seed(seed))


def _mask01(shape, seed=1):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) > 0.4).float()


# ------------------------------------------------------------------------------------------ the helper's rules
FORMS = {
    "full": lambda: _mask01(SHAPE),
    "1F1T": lambda: _mask01((1, F, 1, T)),
    "B11T": lambda: _mask01((B, 1, 1, T)),
    "BF11": lambda: _mask01((B, F, 1, 1)),
    "bool": lambda: _mask01(SHAPE) > 0.5,
    "float64": lambda: _mask01(SHAPE).double(),
    "permuted_view": lambda: _mask01((T, 1, F, B)).permute(3, 2, 1, 0),
    "wrong_F": lambda: _mask01((B, F + 1, 1, T)),
    "wrong_rank": lambda: _mask01((1, B, F, 1, T)),
}
BROADCASTS = {"full", "1F1T", "B11T", "BF11", "bool", "float64", "permuted_view"}
EQUAL = {"full", "bool", "float64", "permuted_view"}


def _check_result(got, src):
    assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == SHAPE
    assert got.numel() == B * F * T
    assert torch.equal(got, src.to(torch.float32).expand(SHAPE))


@pytest.mark.parametrize("form", sorted(FORMS))
def test_equal_rule(form):
    src = FORMS[form]()
    assert not (form == "permuted_view" and src.is_contiguous())
    if form in EQUAL:
        _check_result(E._fit(src, SHAPE, "inpainting_mask", E.RULE_EQUAL), src)
    else:
        with pytest.raises(AssertionError, match="inpainting_mask"):          # the reference's assert (gaussian_diffusion.py:344)
            E._fit(src, SHAPE, "inpainting_mask", E.RULE_EQUAL)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_broadcast_rule(form):
    src = FORMS[form]()
    if form in BROADCASTS:
        _check_result(E._fit(src, SHAPE, "noise mask", E.RULE_BROADCAST), src)
        noise = _full()
        assert torch.equal(noise * (1.0 - E._fit(src, SHAPE, "noise mask", E.RULE_BROADCAST)), noise * (1.0 - src.float()))
    else:
        with pytest.raises(RuntimeError, match="noise mask"):                 # what `noise *= 1. - mask` raises in torch, operand named
            E._fit(src, SHAPE, "noise mask", E.RULE_BROADCAST)
        with pytest.raises(RuntimeError):
            _full().mul_(1.0 - src.float())


@pytest.mark.parametrize("val,ok", [(torch.tensor([2.5]), True), (torch.tensor(2.5), True), (2.5, True), (np.float64(2.5), True),
                                    (torch.tensor([[1.0], [2.0], [3.0]]), True), (torch.tensor([1.0, 2.0, 3.0]).double(), True),
                                    (torch.tensor([1.0, 2.0]), False), (torch.ones(B + 1), False), (torch.ones(0), False)])
def test_scale_rule(val, ok):
    if not ok:
        n = torch.as_tensor(val).numel()
        with pytest.raises(ValueError, match=rf"scale: {n} values for {B} clips"):
            E._fit(val, (B,), "scale", E.RULE_SCALE)
        return
    got = E._fit(val, (B,), "scale", E.RULE_SCALE)
    assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (B,)
    want = torch.as_tensor(np.asarray(val) if not isinstance(val, torch.Tensor) else val).float().reshape(-1)
    assert torch.equal(got, want.expand(B))


def test_device_check_is_apart_from_the_shape_logic():
    m = _mask01((1, F, 1, T))
    assert tuple(E._fit(m, SHAPE, "m", E.RULE_BROADCAST).shape) == SHAPE       # no device needed
    with pytest.raises(RuntimeError, match="m: the engine needs a GPU tensor"):
        E._operand(m, SHAPE, "m", E.RULE_BROADCAST)
    with pytest.raises(AssertionError):                                        # the shape is judged first: a wrong operand never reaches a device
        E._operand(m, SHAPE, "m", E.RULE_EQUAL)


def test_pair_and_noise_mask_roles():
    """With a motion the mask is half of the inpainting pair (shape equality); alone it is only ever the noise mask (broadcast)."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(E, "_need_gpu", lambda t, what: t)
        m, mo = E._mask_pair(_mask01((B, 1, 1, T)), None, SHAPE, None)
        assert mo is None and tuple(m.shape) == SHAPE and m.is_contiguous()
        with pytest.raises(AssertionError, match="inpainting_mask"):
            E._mask_pair(_mask01((B, 1, 1, T)), _full(), SHAPE, None)
        with pytest.raises(AssertionError, match="inpainted_motion"):
            E._mask_pair(_mask01(SHAPE), _full()[:1], SHAPE, None)
        m, mo = E._mask_pair(_mask01(SHAPE) > 0.5, _full().double(), SHAPE, None)
        assert m.dtype == mo.dtype == torch.float32 and tuple(m.shape) == tuple(mo.shape) == SHAPE


# ------------------------------------------------------------------------------------------ the entry points over a recording stub
@pytest.fixture
def stub(monkeypatch):
    return install(monkeypatch)


_schedule = stub_schedule


def _engine():
    return stub_engine(F)


def _all_full(tensors):
    for t in tensors:
        if t.dtype == torch.int64:
            assert t.numel() == B
            continue
        assert t.dtype == torch.float32 and t.is_contiguous(), (t.dtype, t.shape)
        assert t.numel() == B * F * T, tuple(t.shape)


T_IDX = torch.tensor([0, 5, 19])
NONCANON = {"bool": lambda: _mask01(SHAPE) > 0.5, "float64": lambda: _mask01(SHAPE).double(),
            "permuted_view": lambda: _mask01((T, 1, F, B)).permute(3, 2, 1, 0)}
NOISE_MASKS = dict(NONCANON, **{"1F1T": lambda: _mask01((1, F, 1, T)), "B11T": lambda: _mask01((B, 1, 1, T)),
                                "BF11": lambda: _mask01((B, F, 1, 1)), "T": lambda: _mask01((T,))})


@pytest.mark.parametrize("form", sorted(NOISE_MASKS))
def test_q_sample_hands_over_full_size_buffers(stub, form):
    _schedule().q_sample(_full(), T_IDX, _full(1), NOISE_MASKS[form]())
    (name, args), = stub.lib.calls
    assert name == "mst_q_sample" and args[5] == B and args[6] == F * T
    assert len(stub.seen) == 5
    _all_full(stub.seen)


def test_q_sample_refusals(stub):
    with pytest.raises(AssertionError, match="noise"):
        _schedule().q_sample(_full(), T_IDX, _full()[:1], None)
    with pytest.raises(RuntimeError, match="noise mask"):
        _schedule().q_sample(_full(), T_IDX, _full(1), _mask01((B, F + 1, 1, T)))
    assert not stub.lib.calls


@pytest.mark.parametrize("guided", [False, True], ids=["step", "step_guided"])
@pytest.mark.parametrize("form", sorted(NOISE_MASKS))
def test_step_with_a_noise_mask_alone(stub, form, guided):
    sch = _schedule()
    mo = _full(2).permute(0, 3, 2, 1).contiguous().permute(0, 3, 2, 1)          # a non-contiguous model output
    assert not mo.is_contiguous()
    if guided:
        guide = E.guide_args(_full(), grad=_full(3)[:1])                         # (guide operands broadcast too)
        sch.step_guided(mo, _full(), T_IDX, _full(1), guide, mask=NOISE_MASKS[form](), mask_noise=True)
        assert guide[1][0].numel() == B * F * T
    else:
        sch.step(mo, _full(), T_IDX, _full(1), mask=NOISE_MASKS[form](), mask_noise=True)
    (name, args), = stub.lib.calls
    assert name == ("mst_step_epilogue_guided" if guided else "mst_step_epilogue_mt") and args[7] == B and args[8] == F * T
    assert len(stub.seen) == 7                                                   # out, x, noise, mask, t, sample, xstart (motion: NULL)
    _all_full(stub.seen)


@pytest.mark.parametrize("form", sorted(NONCANON))
def test_step_with_the_inpainting_pair(stub, form):
    _schedule().step(_full(2), _full(), T_IDX, _full(1), mask=NONCANON[form](), motion=_full(4).double(), mask_noise=True)
    assert len(stub.seen) == 8
    _all_full(stub.seen)


@pytest.mark.parametrize("bad", ["mask_1F1T", "mask_B11T", "motion_one_clip", "model_output_one_clip", "noise_one_clip", "mask_wrong_F"])
def test_step_refuses_what_the_reference_asserts(stub, bad):
    kw = dict(model_output=_full(2), x=_full(), t=T_IDX, noise=_full(1), mask=_mask01(SHAPE), motion=_full(4))
    kw.update({"mask_1F1T": dict(mask=_mask01((1, F, 1, T))), "mask_B11T": dict(mask=_mask01((B, 1, 1, T))),
               "motion_one_clip": dict(motion=_full(4)[:1]), "model_output_one_clip": dict(model_output=_full(2)[:1]),
               "noise_one_clip": dict(noise=_full(1)[:1]), "mask_wrong_F": dict(mask=_mask01((B, F + 1, 1, T)))}[bad])
    with pytest.raises(AssertionError):
        _schedule().step(**kw)
    assert not stub.lib.calls


@pytest.mark.parametrize("scale", [2.5, torch.tensor([2.5]), torch.tensor(2.5), torch.tensor([[1.0], [2.0], [3.0]]).double()],
                         ids=["float", "one_element", "zero_dim", "Bx1_float64"])
def test_forward_scale(stub, scale):
    _engine().forward(_full(), T_IDX, scale=scale, cfg=True)
    (name, args), = stub.lib.calls
    assert name == "mst_forward"
    x, t, sc, out = stub.seen
    assert t.numel() == B
    assert sc.dtype == torch.float32 and sc.is_contiguous() and sc.numel() == B
    assert x.numel() == out.numel() == B * F * T


def test_forward_refuses_a_scale_of_another_size(stub):
    with pytest.raises(ValueError, match=r"scale: 2 values for 3 clips"):
        _engine().forward(_full(), T_IDX, scale=torch.ones(2), cfg=True)
    assert not stub.lib.calls


def _loop_args(stub):
    (name, args), = stub.lib.calls
    assert name == "mst_sample_loop"
    return args[2]._obj


@pytest.mark.parametrize("form", sorted(NOISE_MASKS))
def test_sample_loop_operands(stub, form):
    eng = _engine()
    noise = torch.randn((3,) + SHAPE)
    eng.sample_loop(_schedule(), _full(), 2, 0, cfg=True, scale=torch.tensor([2.0]), mask=NOISE_MASKS[form](), noise=noise)
    a = _loop_args(stub)
    by_ptr = {t.data_ptr(): t for t in eng._loop_keepalive}
    assert by_ptr[a.scale_dev].numel() == B and by_ptr[a.scale_dev].is_contiguous()
    assert by_ptr[a.noise_dev].numel() == 3 * B * F * T
    m = by_ptr[a.inpainting_mask_dev]
    assert m.dtype == torch.float32 and m.is_contiguous() and m.numel() == B * F * T
    assert not a.inpainted_motion_dev


def test_sample_loop_pair_and_refusals(stub):
    eng = _engine()
    eng.sample_loop(_schedule(), _full(), 2, 0, mask=_mask01(SHAPE) > 0.5, motion=_full(4).double(), seed=1)
    a = _loop_args(stub)
    by_ptr = {t.data_ptr(): t for t in eng._loop_keepalive}
    for p in (a.inpainting_mask_dev, a.inpainted_motion_dev):
        assert by_ptr[p].dtype == torch.float32 and by_ptr[p].is_contiguous() and by_ptr[p].numel() == B * F * T
    stub.lib.calls.clear()
    with pytest.raises(AssertionError, match="inpainting_mask"):
        eng.sample_loop(_schedule(), _full(), 2, 0, mask=_mask01((1, F, 1, T)), motion=_full(4), seed=1)
    with pytest.raises(AssertionError, match="inpainted_motion"):
        eng.sample_loop(_schedule(), _full(), 2, 0, mask=_mask01(SHAPE), motion=_full(4)[:1], seed=1)
    with pytest.raises(ValueError, match="scale: 2 values for 3 clips"):
        eng.sample_loop(_schedule(), _full(), 2, 0, cfg=True, scale=torch.ones(2), seed=1)
    with pytest.raises(AssertionError):                                          # numel right, per-step shape wrong
        eng.sample_loop(_schedule(), _full(), 2, 0, noise=torch.randn(3, B, T, 1, F))
    with pytest.raises(AssertionError):
        eng.sample_loop(_schedule(), _full(), 2, 0, noise=torch.randn((2,) + SHAPE))
    assert not stub.lib.calls


@pytest.mark.parametrize("form", ["pair_bool", "pair_float64", "noise_1F1T", "noise_B11T"])
def test_fused_step_node_saves_the_buffer_forward_used(stub, form):
    from mst_amd.diffusion.fused_ops import FusedStepFn
    mask = {"pair_bool": _mask01(SHAPE) > 0.5, "pair_float64": _mask01(SHAPE).double(), "noise_1F1T": _mask01((1, F, 1, T)),
            "noise_B11T": _mask01((B, 1, 1, T))}[form]
    motion = _full(4) if form.startswith("pair") else None
    out = _full(2).requires_grad_(True)
    sample, pred = FusedStepFn.apply(out, _full(), T_IDX, _full(1), mask, motion, _schedule(), E.SAMPLER_DDPM, 0.0, True, False)
    fwd_mask = stub.seen[3]
    assert fwd_mask.numel() == B * F * T and fwd_mask.dtype == torch.float32 and fwd_mask.is_contiguous()
    n_fwd = len(stub.seen)
    _all_full(stub.seen)
    # the stub wrote nothing: give the outputs values so that backward has finite inputs, then run it
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr("mst_amd.diffusion.fused_ops._cuda_f32", lambda t, what: t)
        (sample.sum() + pred.sum()).backward()
    name, args = stub.lib.calls[-1]
    assert name == "mst_step_backward" and args[6] == B and args[7] == F * T and args[4] == int(motion is not None)
    bwd = stub.seen[n_fwd:]
    _all_full(bwd)
    if motion is not None:                                                        # k_step_backward reads the mask only for a blend
        assert any(t.data_ptr() == fwd_mask.data_ptr() for t in bwd), "backward must get the buffer forward used"


def test_fused_step_node_refuses_a_broadcast_pair(stub):
    from mst_amd.diffusion.fused_ops import FusedStepFn
    with pytest.raises(AssertionError, match="inpainting_mask"):
        FusedStepFn.apply(_full(2).requires_grad_(True), _full(), T_IDX, _full(1), _mask01((1, F, 1, T)), _full(4), _schedule(),
                          E.SAMPLER_DDPM, 0.0, True, False)
    assert not stub.lib.calls
