"""What the modules' weight watch rests on, without a GPU.

`_EngineHost.mst_engine` and `StyleBank.mst_engine` decide what to upload from `p._version` and `p.data_ptr()` of every watched
parameter.  Which writes move those two is torch's behaviour, not ours: it is pinned here, so that a torch upgrade that changes it fails
in this file first and not as a silently stale (or twice uploaded) engine.  The writes the watch cannot see are why
`mst_weights_changed()` exists.  Also here: `copy.deepcopy` of a module that holds engines."""
import copy
import ctypes

import pytest
import torch

import mst_amd  # noqa: F401


def _mark(p):
    return p._version, p.data_ptr()


def _param():
    return torch.nn.Parameter(torch.linspace(-1.0, 1.0, 12).reshape(3, 4).clone())


def _no_grad_copy(p):
    with torch.no_grad():
        p.copy_(torch.zeros_like(p))


def _no_grad_mul(p):
    with torch.no_grad():
        p.mul_(2.0)


def _load_state_dict(p):
    m = torch.nn.Module()
    m.w = p
    m.load_state_dict({"w": torch.zeros(3, 4)})


def _sgd(p):
    p.grad = torch.ones_like(p)
    torch.optim.SGD([p], lr=0.1).step()


def _adamw(p):
    p.grad = torch.ones_like(p)
    torch.optim.AdamW([p], lr=0.1).step()


SEEN = {"no_grad copy_": _no_grad_copy, "no_grad mul_": _no_grad_mul, "detach().add_": lambda p: p.detach().add_(1.0),
        "load_state_dict": _load_state_dict, "SGD.step": _sgd, "AdamW.step": _adamw,
        "increment_version": lambda p: torch.autograd.graph.increment_version(p)}
UNSEEN = {"data.copy_": lambda p: p.data.copy_(torch.zeros_like(p)), "data.mul_": lambda p: p.data.mul_(2.0),
          "data.normal_": lambda p: p.data.normal_(), "data.add_": lambda p: p.data.add_(1.0),
          "data.zero_": lambda p: p.data.zero_()}


@pytest.mark.parametrize("how", sorted(SEEN))
def test_writes_that_bump_the_version(how):
    p = _param()
    before, values = _mark(p), p.detach().clone()
    SEEN[how](p)
    assert p._version > before[0], how
    assert p.data_ptr() == before[1], how            # in place: the version alone says it
    if how != "increment_version":
        assert not torch.equal(p.detach(), values)


@pytest.mark.parametrize("how", sorted(UNSEEN))
def test_writes_through_data_move_neither_version_nor_pointer(how):
    """The blind spot: the values change, the watch's two signals do not.  (If this starts to fail, torch now reports these writes: the
    explicit `mst_weights_changed()` is then redundant, not wrong.)"""
    p = _param()
    before, values = _mark(p), p.detach().clone()
    UNSEEN[how](p)
    assert not torch.equal(p.detach(), values)
    assert _mark(p) == before, how


def test_assigning_data_moves_the_pointer_only():
    p = _param()
    before = _mark(p)
    keep = p.data                                     # (the old storage stays alive: the new one cannot take its address)
    p.data = torch.zeros(3, 4)
    assert p._version == before[0] and p.data_ptr() != before[1] and keep.data_ptr() == before[1]


def test_to_keeps_the_parameter_objects():
    """`mst_engine` builds its watch list once: the Parameter objects must survive `.to()`, `.float()` and `load_state_dict`."""
    m = torch.nn.Linear(4, 3)
    ids = [id(p) for p in m.parameters()]
    m.double().float().to("cpu")
    m.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})
    assert [id(p) for p in m.parameters()] == ids


def test_state_dict_tensors_share_storage_with_the_parameters():
    """`DenoiserEngine._remember_source` keeps the state dict's tensors: an in-place step must show through them."""
    m = torch.nn.Linear(4, 3)
    sd = m.state_dict()
    with torch.no_grad():
        m.weight.add_(1.0)
    assert sd["weight"].data_ptr() == m.weight.data_ptr() and torch.equal(sd["weight"], m.weight.detach())


# ------------------------------------------------------------------------------------------------- deepcopy, the explicit calls
class _Handle:
    """What a DenoiserEngine is to `copy`: an object that owns a ctypes pointer."""

    def __init__(self):
        self.handle = ctypes.c_void_p(0x1000)
        self.precise = None

    def set_precise(self, on):
        self.precise = bool(on)


@pytest.fixture(scope="module")
def model():
    import contextlib
    import io
    import loop_fixture as lf
    from mst_amd.model.mdm_forstyledataset import StyleDiffusion
    from mst_amd.utils import model_util
    with contextlib.redirect_stdout(io.StringIO()):
        m, _, _ = model_util.creat_serval_diffusion(lf.diffusion_args(), StyleDiffusion, "ddim20")
    return m.eval()


def _as_if_it_had_run(m):
    """The entries a native call leaves behind (model/mdm_forstyledataset.py, model/native_stack.py), with stand-in engines."""
    from mst_amd.model.native_stack import stack_parameters
    for host in (m, m.motion_enc, m.motion_enc.mdm_model):
        host.__dict__["_mst_engines"] = {"cuda:0": {"eng": _Handle(), "rows": 2, "frames": 76, "version": (1, 2, 3)},
                                         ("cuda:0", "chain"): {"eng": _Handle(), "rows": 1, "frames": 76, "version": (1, 2, 3)}}
        host.__dict__["_mst_sources"] = host._engine_sources()
    stack_parameters(m.seqTransEncoder)               # caches `_mst_stack_params` on the (plain) encoder module
    m.__dict__["_mst_chain_acc"] = (None, torch.zeros(3), [])


def test_a_ctypes_pointer_refuses_to_be_copied():
    """Why the default deepcopy of a module that has run cannot work: it walks into the engines' handles."""
    with pytest.raises(ValueError, match="pointers cannot be pickled"):
        copy.deepcopy(ctypes.c_void_p(0x1000))
    with pytest.raises(ValueError, match="pointers cannot be pickled"):
        copy.deepcopy(_Handle())


def test_deepcopy_leaves_the_engines_behind(model):
    _as_if_it_had_run(model)
    model.set_precise(True)
    twin = copy.deepcopy(model)
    left = sorted({k for m in twin.modules() for k in m.__dict__ if k.startswith("_mst_")})
    assert left == ["_mst_precise"], left              # the setting travels, the caches do not
    assert twin.__dict__["_mst_precise"] is True
    assert "_mst_engines" in model.__dict__ and "_mst_stack_params" in model.seqTransEncoder.__dict__      # the original keeps its own
    assert type(twin) is type(model) and twin.training == model.training
    a, b = dict(model.named_parameters()), dict(twin.named_parameters())
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] is not b[k] and a[k].data_ptr() != b[k].data_ptr() and torch.equal(a[k], b[k]), k
        assert a[k].requires_grad == b[k].requires_grad, k
    sa, sb = model.state_dict(), twin.state_dict()
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
    # one prior inside the copy, as inside the original (the copy's watch lists name the COPY's parameters)
    assert twin._prior() is twin.motion_enc.mdm_model
    own = {id(p) for p in twin.parameters()}
    assert all(id(p) in own for p in twin._engine_sources()[2])
    with torch.no_grad():
        next(twin.seqTransEncoder.parameters()).add_(1.0)
    assert not torch.equal(next(twin.seqTransEncoder.parameters()), next(model.seqTransEncoder.parameters()))
    model.set_precise(False)
    for m in model.modules():
        for k in [k for k in m.__dict__ if k.startswith("_mst_")]:
            del m.__dict__[k]


def test_deepcopy_of_a_bank(model):
    from mst_amd.model.style_bank import StyleBank
    bank = StyleBank([model, copy.deepcopy(model)])
    bank.__dict__["_mst_bank"] = {"eng": _Handle(), 1: (0, 1, 2)}
    twin = copy.deepcopy(bank)
    assert "_mst_bank" not in twin.__dict__ and "_mst_bank" in bank.__dict__
    assert len(twin.members) == 2 and twin.members[0] is not bank.members[0]
    del bank.__dict__["_mst_bank"]


def test_weights_changed_drops_every_recorded_version(model):
    """Every engine of the module and of the engine hosts inside it (motion encoder, prior) forgets its version, so its next call
    uploads everything; the epoch that a StyleBank compares moves."""
    _as_if_it_had_run(model)
    hosts = (model, model.motion_enc, model.motion_enc.mdm_model)
    model.mst_weights_changed()
    for h in hosts:
        assert [e["version"] for e in h.__dict__["_mst_engines"].values()] == [None, None]
        assert h.__dict__["_mst_epoch"] == 1
    model.mst_weights_changed()
    assert model.__dict__["_mst_epoch"] == 2
    for m in model.modules():
        for k in [k for k in m.__dict__ if k.startswith("_mst_")]:
            del m.__dict__[k]


def test_module_precise_switch_reaches_the_engines_it_holds(model):
    _as_if_it_had_run(model)
    model.set_precise(True)
    assert [e["eng"].precise for e in model.__dict__["_mst_engines"].values()] == [True, True]
    assert model.__dict__["_mst_precise"] is True
    assert [e["eng"].precise for e in model.motion_enc.__dict__["_mst_engines"].values()] == [None, None]     # another host: its own switch
    model.set_precise(False)
    assert [e["eng"].precise for e in model.__dict__["_mst_engines"].values()] == [False, False]
    for m in model.modules():
        for k in [k for k in m.__dict__ if k.startswith("_mst_")]:
            del m.__dict__[k]


def test_bank_weights_changed_reaches_every_member(model):
    from mst_amd.model.style_bank import StyleBank
    bank = StyleBank([model, copy.deepcopy(model), copy.deepcopy(model)])
    bank.mst_weights_changed()
    assert [m.__dict__["_mst_epoch"] for m in bank.members] == [1, 1, 1]
    for m in model.modules():
        for k in [k for k in m.__dict__ if k.startswith("_mst_")]:
            del m.__dict__[k]
