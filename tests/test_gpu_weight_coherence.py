"""Every derived weight copy of an engine follows a reload of the tensor it was made from (the table of copies).

An engine keeps, per weight, the plain f16 matrix, its transpose, the fused kernels' fragment streams (wqkv, wtail, wtail_bwd), the
small-launch block packings (wsm_*), the packed pose projections and the timestep-embedding table; dirty flags say which of them are
older than the plain matrices.  The suite's other tests load an engine once and use it, and the flags start `true`; here ONE engine that
has RUN is changed, one tensor at a time, and used again.

The comparison rule: after a change the warm engine gives the BITS of a second engine that took a full load of the new state -- same
kernels, same inputs, same seeds, and the project asserts bit reproducibility elsewhere, so the bar is `torch.equal`.  The visibility
rule: each change moves the fp32 oracle's forward by at least 5e-3 relative L2 (weight_fixture.assert_visible, asserted inside the
test), so a stale copy cannot pass for rounding; and one case per tensor group holds the second engine to the oracle at TOL = 1e-3, so
"both stale" cannot pass either.

Sections: 1. the one-tensor reload matrix; 2. the modules' version watch (every way a script changes parameters, regrowth, the two
engine slots, the precise switch, deepcopy, two fine-tune iterations, the motion encoder's own watch); 3. bulk reloads, precise-mode
transitions, and a reload between the capture and the replay of a graph (MST_GRAPH=1) and under the resident trunk (MST_TRUNK=1);
4. the style bank."""
import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
from conftest import rel_l2
import weight_fixture as wf

pytestmark = pytest.mark.gpu
F, T, LP, PRIOR, TOL = wf.F, wf.T, wf.LP, wf.PRIOR, wf.TOL
cu, dev = wf.cu, wf.dev


# =============================================================================================== 1. one-tensor reload matrix
CASES = wf.matrix_cases()
# one case per tensor group is also held to the oracle at TOL: the FIRST of each group (fewest perturbations piled up under it) ...
ORACLE_CASES = {CASES.index(f"{LP}0.self_attn.in_proj_weight"), CASES.index("input_process.poseEmbedding.weight"),
                CASES.index("embed_timestep.time_embed.0.weight")}
# The LAST case, the positional table, lies over all 34 other perturbations, the conditioning tensors at 3 w + 0.5 among them: a
# checkpoint as ill-conditioned as the stress weights of tests/test_gpu_parity.py, where f16 operands themselves leave the 1e-3 bar
# (fresh engine 1.65e-3 from the oracle there, and the oracle with f16-rounded GEMM operands 1.6e-3 .. 1.8e-3 depending on the host's
# f16 arithmetic).  In the matrix that case is compared bit for bit like the others; the table's reload is held to the oracle at TOL
# where TOL is the project's bar, on the base state: test_positional_table_reload_alone_meets_the_oracle.
_M = {"warm": None, "other": None, "k": -1}


def _reload_one(eng, k):
    """Case k: ONLY tensor k goes up, through load_tensor."""
    name = CASES[k]
    w, pe = wf.state_after(k)
    eng.load_tensor(name, torch.from_numpy(pe if name == wf.PE else w[wf.state_key(name)]))


@pytest.mark.parametrize("k", range(len(CASES)), ids=CASES)
def test_one_tensor_reload_on_a_warm_engine(k):
    """ONE warm engine changed cumulatively: case k reloads only tensor k, then every consumer of a derived copy runs (which clears
    every flag again for case k + 1).  A second engine takes a full load_state_dict of the same state -- created fresh for the first
    and the last case and for every even case in between, re-used for the odd ones (107 uploads into an engine that has run: the
    other way to the same state).  The re-used engine goes through the same flag code as the warm one, so a flag assignment missing
    from a load would leave both stale in the same way; the fresh engine of the next case has no stale copy to share."""
    from mst_amd.engine import DenoiserEngine
    st = _M
    if st["warm"] is None or st["k"] >= k:                      # first case, or a case run again: start over from the base state
        st["warm"], st["other"], st["k"] = wf.make_engine(*wf.state_after(-1), wf.MAX_ROWS), None, -1
        wf.consumers(st["warm"])                                # warm: every flag cleared, every copy built from the OLD weights
    for j in range(st["k"] + 1, k):                             # (a case selected on its own: catch up, one tensor at a time, with
        _reload_one(st["warm"], j)                              # the consumers after each: the flag history of the full run)
        wf.consumers(st["warm"])
    old, new = wf.state_after(k - 1), wf.state_after(k)
    ref_new = wf.oracle_forward(*new, key=k)
    wf.assert_visible(wf.oracle_forward(*old, key=k - 1), ref_new, CASES[k])
    _reload_one(st["warm"], k)
    st["k"] = k
    if st["other"] is None or k % 2 == 0 or k == len(CASES) - 1:
        st["other"] = DenoiserEngine(F, T, wf.MAX_ROWS, device=dev())
    wf.load_all(st["other"], *new)
    a, b = wf.consumers(st["warm"]), wf.consumers(st["other"])
    wf.assert_same_bits(a, b, CASES[k])
    if k in ORACLE_CASES:
        e = rel_l2(b["forward/small"].cpu().numpy(), ref_new)
        print(f"{CASES[k]}: fresh engine vs oracle {e:.3e}")
        assert e < TOL


def test_positional_table_reload_alone_meets_the_oracle():
    """The positional table reloaded ALONE into a warm engine with the base weights (well conditioned: the parity bar applies): the
    bits of a fresh engine, and that engine within TOL of the fp32 oracle.  The table feeds the frames' positional rows and, through
    the timestep MLP, the 1000-row timestep-embedding table (temb_table_valid)."""
    w, pe = wf.state_after(-1)
    warm = wf.make_engine(w, pe, wf.MAX_ROWS)
    wf.consumers(warm)
    new = wf.bump(pe)
    ref = wf.oracle_forward(w, new)
    wf.assert_visible(wf.oracle_forward(w, pe, key=-1), ref, wf.PE)
    warm.load_tensor(wf.PE, torch.from_numpy(new))
    a, b = wf.consumers(warm), wf.consumers(wf.make_engine(w, new, wf.MAX_ROWS))
    wf.assert_same_bits(a, b, wf.PE)
    e = rel_l2(b["forward/small"].cpu().numpy(), ref)
    print(f"{wf.PE} alone: fresh engine vs oracle {e:.3e}")
    assert e < TOL


# =============================================================================================== 2. module level: the version watch
# A StyleDiffusion that has RUN is changed in each way a training script changes parameters; afterwards the `no_grad` call and the
# training call (output and all 96 stack gradients) give the bits of a model built fresh and given `model.state_dict()`.
_B = {}


def _blank_model():
    """A StyleDiffusion as loop_fixture.build_model makes it, without the seeded weights (the caller loads a state)."""
    import loop_fixture as lf
    from mst_amd.model.mdm_forstyledataset import StyleDiffusion
    from mst_amd.utils import model_util
    model, _B["ddim"], _ = model_util.creat_serval_diffusion(lf.diffusion_args(), StyleDiffusion, "ddim20")
    return model.to(dev()).eval()


def _new_model():
    """A model with the loop fixture's seeded weights (generated once, kept on the CPU, never mutated)."""
    if "sd" not in _B:
        import loop_fixture as lf
        _B["sd"] = {k: v.detach().cpu().clone() for k, v in lf.build_model(torch.device("cpu"))[0].state_dict().items()}
    return _fresh(_B["sd"])


def _fresh(sd):
    m = _blank_model()
    missing, unexpected = m.load_state_dict({k: v.detach().clone() for k, v in sd.items()}, strict=False)
    assert not unexpected and not missing
    return m


def _state_np(model):
    sd = model.state_dict()
    w = {k: v.detach().cpu().numpy().copy() for k, v in sd.items() if not k.endswith(".pe")}
    return w, sd[PRIOR + wf.PE].detach().cpu().numpy().reshape(-1, 512).copy()


def _stack(model):
    from mst_amd.model.native_stack import stack_parameters
    return stack_parameters(model.seqTransEncoder)


def _calls(model, B=2):
    """The `no_grad` model call and the training call (one native node; eval mode: no dropout, no condition mask) at B clips."""
    i = wf._inputs()
    x, t, y = i["xl"][:B], i["tl"][:B], {"text_embed": i["txtl"][:B]}
    if B == 2:
        x, t, y = i["xs"], i["ts"], {"text_embed": i["txts"]}                  # the oracle's probe
    with torch.no_grad():
        out = model(x, t, y)
    for p in model.parameters():
        p.grad = None
    o = model(x, t, y)
    (o * i["dl"][:B]).sum().backward()
    torch.cuda.synchronize()
    g = [p.grad for p in _stack(model)]
    assert len(g) == 96 and all(a is not None for a in g)
    return {"no_grad": out, "train": [o.detach()] + [a.clone() for a in g]}


def _p(model, name):
    return dict(model.named_parameters())[name]


STACK_T, PRIOR_T = "seqTransEncoder.layers.0.linear1.weight", PRIOR + "input_process.poseEmbedding.weight"
LR = 3e-3            # one Adam step moves every stack element by about lr: the oracle moves by far more than 5e-3 (asserted)


def _bumped(p):
    return torch.from_numpy(wf.bump(p.detach().cpu().numpy())).to(p.device)


def _change(model, how):
    """Each way of changing parameters; the model has run, and its stack tensors hold the gradients of that run."""
    if how in ("fused_adamw", "torch_adamw"):
        from mst_amd.optim import FusedAdamW
        cls = FusedAdamW if how == "fused_adamw" else torch.optim.AdamW
        cls(model.parameters_wo_enc(), lr=LR, weight_decay=0.01).step()
    elif how in ("stack_inplace", "prior_inplace", "both_inplace"):
        with torch.no_grad():
            for name in {"stack_inplace": [STACK_T], "prior_inplace": [PRIOR_T], "both_inplace": [STACK_T, PRIOR_T]}[how]:
                _p(model, name).copy_(_bumped(_p(model, name)))
    elif how == "load_state_dict":
        sd = model.state_dict()
        sd = {k: (_bumped(v) if k in (STACK_T, PRIOR_T) else v.clone()) for k, v in sd.items()}
        model.load_state_dict(sd)
    elif how == "data_assign":                                   # a new tensor: the pointer moves, the version does not
        for name in (STACK_T, PRIOR_T):
            _p(model, name).data = _bumped(_p(model, name))
    elif how == "data_write":                                    # moves neither: the explicit call is the signal
        for name in (STACK_T, PRIOR_T):
            _p(model, name).data.mul_(1.25)
        model.mst_weights_changed()
    else:
        raise AssertionError(how)


CHANGES = ["fused_adamw", "torch_adamw", "stack_inplace", "prior_inplace", "both_inplace", "load_state_dict", "data_assign", "data_write"]


@pytest.mark.parametrize("how", CHANGES)
def test_module_follows_a_parameter_change(how):
    model = _new_model()
    _calls(model)                                                # warm: engines loaded, versions recorded, gradients present
    _B["old"] = _state_np(model)
    _change(model, how)
    wf.assert_visible(_B["old"], _state_np(model), how)
    wf.assert_same_bits(_calls(model), _calls(_fresh(model.state_dict())), how)


def test_module_change_then_regrown_engine_then_smaller_call():
    """A change, a call that makes mst_engine build a larger engine (its version starts empty: a full load), then a smaller call."""
    model = _new_model()
    _calls(model, 2)
    old = _state_np(model)
    _change(model, "stack_inplace")
    wf.assert_visible(old, _state_np(model), "regrow")
    fresh = _fresh(model.state_dict())
    wf.assert_same_bits(_calls(model, 5), _calls(fresh, 5), "regrown")
    wf.assert_same_bits(_calls(model, 2), _calls(fresh, 2), "smaller call after the regrowth")


def _slot_forward(model, slot):
    i = wf._inputs()
    eng = model.mst_engine(2, T, slot=slot)
    model.mst_prepare(eng, {"text_embed": i["txts"]}, False)
    out = eng.forward(i["xs"], i["ts"])
    torch.cuda.synchronize()
    return {"forward": out}


def test_module_each_engine_slot_keeps_its_own_version():
    """The module's engine and the "chain" side engine both hold the old weights; after a change, using one must not mark the other
    as current."""
    model = _new_model()
    for slot in (None, "chain"):
        _slot_forward(model, slot)
    old = _state_np(model)
    _change(model, "both_inplace")
    wf.assert_visible(old, _state_np(model), "slots")
    fresh = _fresh(model.state_dict())
    want = _slot_forward(fresh, None)
    assert model.mst_engine(2, T) is not model.mst_engine(2, T, slot="chain")
    for slot in ("chain", None):
        wf.assert_same_bits(_slot_forward(model, slot), want, f"slot {slot}")


def test_module_precise_switch_reaches_regrown_and_side_engines():
    """model.set_precise(True) on a model that has run: the engine it owns, the larger one built later and the "chain" side engine are
    all precise, and give the bits of a fresh model switched before its first call."""
    model = _new_model()
    plain = _calls(model, 2)["no_grad"]
    model.set_precise(True)
    fresh = _fresh(model.state_dict())
    fresh.set_precise(True)
    i = wf._inputs()
    for B in (2, 5):                                             # 5 clips: a larger engine is built
        with torch.no_grad():
            y = {"text_embed": (i["txts"] if B == 2 else i["txtl"][:B])}
            x, t = (i["xs"], i["ts"]) if B == 2 else (i["xl"][:B], i["tl"][:B])
            a, b = model(x, t, y), fresh(x, t, y)
        assert model.mst_engine(B, T)._precise_on
        assert torch.equal(a, b), B
        if B == 2:
            assert not torch.equal(a, plain)                     # (precise mode is another arithmetic: the switch did something)
            ref = wf.oracle_forward(*_state_np(model))
            assert rel_l2(a.cpu().numpy(), ref) < TOL and rel_l2(plain.cpu().numpy(), ref) < TOL
    assert model.mst_engine(2, T, slot="chain")._precise_on
    wf.assert_same_bits(_slot_forward(model, "chain"), _slot_forward(fresh, "chain"), "chain")


def test_deepcopy_of_a_model_that_has_run_is_independent():
    """copy.deepcopy leaves the engines behind: the copy builds its own, and a step on the original leaves the copy as it was."""
    import copy
    from mst_amd.optim import FusedAdamW
    model = _new_model()
    before = _calls(model)
    twin = copy.deepcopy(model)
    assert not any(k.startswith("_mst_") and k != "_mst_precise" for m in twin.modules() for k in m.__dict__)
    old = _state_np(model)
    FusedAdamW(model.parameters_wo_enc(), lr=LR, weight_decay=0.01).step()
    wf.assert_visible(old, _state_np(model), "deepcopy")
    wf.assert_same_bits(_calls(twin), before, "the copy, after the original's step")
    wf.assert_same_bits(_calls(model), _calls(_fresh(model.state_dict())), "the original, after its step")
    assert twin.mst_engine(2, T) is not model.mst_engine(2, T)



def _finetune_iteration(model, seed):
    """One fine-tune iteration as train/training_loop.py issues it (the text-to-motion call, the chained single-clip DDIM steps, the
    frozen motion encoder, backward), at 2 clips of the small shape, every draw seeded; -> (loss terms, the 96 gradients)."""
    i, d = wf._inputs(), dev()
    B, emb = wf.B_SMALL, wf._inputs()["txts"][:1]
    t2m, content, style = i["xs"], i["motion"][:1].contiguous(), i["motion"][1:2].contiguous()
    y1 = {"y": {"text": ["a"], "text_embed": emb, "mask": torch.ones(1, 1, 1, T, device=d),
                "inpainting_mask": i["mask"][:1].contiguous(), "inpainted_motion": content}}
    yB = {"y": {"text": ["a"] * B, "text_embed": emb.expand(B, -1).contiguous(), "mask": torch.ones(B, 1, 1, T, device=d),
                "inpainting_mask": i["mask"], "inpainted_motion": t2m}}
    torch.manual_seed(seed)
    np.random.seed(seed)
    tt = torch.randint(0, 6, (B,), generator=torch.Generator(device="cpu").manual_seed(seed)).to(d)
    model.zero_grad()
    terms = _B["ddim"].few_shot_style_finetune_losses(model, t2m, tt, content, style, skip_steps=700, model_kwargs=y1,
                                                      model_t2m_kwargs=yB, semantic_guidance=1, use_ddim=1, Ls=10)
    terms["loss"].backward()
    torch.cuda.synchronize()
    g = [p.grad for p in _stack(model)]
    assert all(a is not None for a in g)
    return {"terms": [terms[k].detach().clone() for k in ("loss", "rot_mse", "text_cosine")], "grads": [a.clone() for a in g]}


def test_second_finetune_iteration_reads_the_stepped_weights():
    """Iteration 1, opt.step(), iteration 2: its loss terms and all 96 gradients are those of a fresh model loaded with the post-step
    state and run with the same seeds (dropout on: the seeds are part of the comparison).  An engine, a chained side engine or a
    motion-encoder engine that kept the pre-step weights would differ: the step moves the ORACLE's forward by over 5e-3."""
    from mst_amd.optim import FusedAdamW
    model = _new_model().train()
    opt = FusedAdamW(model.parameters_wo_enc(), lr=LR, weight_decay=0.0)
    _finetune_iteration(model, 11)
    old = _state_np(model)
    opt.step()
    wf.assert_visible(old, _state_np(model), "opt.step() between two fine-tune iterations")
    fresh = _fresh(model.state_dict()).train()
    a, b = _finetune_iteration(model, 12), _finetune_iteration(fresh, 12)
    assert len(a["grads"]) == 96
    wf.assert_same_bits(a, b, "iteration 2")



def _menc_calls(me):
    """The frozen motion encoder as the fine-tune objective uses it: the `no_grad` call and the call inside an autograd graph (its
    INPUT gradient), 75 frames with a padded tail on clip 1."""
    i = wf._inputs()
    y = {"mask": i["keep_me"][:, 2:].reshape(wf.B_SMALL, 1, 1, T - 1).to(dev())}
    with torch.no_grad():
        mu, _ = me(i["xme"], y)
    x = i["xme"].clone().requires_grad_(True)
    mu2, _ = me(x, y)
    (mu2 * i["dmu"]).sum().backward()
    torch.cuda.synchronize()
    return {"no_grad": mu, "train": [mu2.detach(), x.grad]}


def _menc_oracle(model):
    from oracle import denoiser
    i = wf._inputs()
    w, pe = _state_np(model)
    return denoiser.motion_encoder(w, pe, i["xme"].cpu().numpy(), i["keep_me"][:, 2:].numpy()).numpy()


def test_motion_encoder_module_reloaded_after_it_has_run():
    """The MotionEncoder is an engine host of its own (its own engines, version tuple and sources: its stack, the prior's
    projections).  After it has run: a stack tensor written in place under no_grad, then load_state_dict; after each, forward and
    backward give the bits of the encoder of a model built fresh from the same state.  Visibility on the oracle's motion encoder."""
    model = _new_model()
    me = model.motion_enc
    _menc_calls(me)
    name = "motion_enc.seqTransEncoder.layers.0.linear1.weight"
    ref = _menc_oracle(model)
    with torch.no_grad():
        _p(model, name).copy_(_bumped(_p(model, name)))
    ref1 = _menc_oracle(model)
    wf.assert_visible(ref, ref1, "motion encoder, in place")
    fresh = _fresh(model.state_dict()).motion_enc
    got = _menc_calls(fresh)
    wf.assert_same_bits(_menc_calls(me), got, "motion encoder, in place")
    sd = {k: (_bumped(v) if k in ("seqTransEncoder.layers.7.self_attn.in_proj_weight", "mdm_model.input_process.poseEmbedding.weight")
              else v.clone()) for k, v in me.state_dict().items()}
    me.load_state_dict(sd)
    wf.assert_visible(ref1, _menc_oracle(model), "motion encoder, load_state_dict")
    wf.assert_same_bits(_menc_calls(me), _menc_calls(_fresh(model.state_dict()).motion_enc), "motion encoder, load_state_dict")


# =============================================================================================== 3. bulk reloads and precise mode
def _all_layers_bumped(w):
    """Every stack tensor of layers 0 and 7 perturbed (the matrix's 24 tensors, in one go)."""
    return {k: (wf.bump(v) if k.startswith((LP + "0.", LP + "7.")) else v) for k, v in w.items()}


def test_load_layers_on_a_warm_engine():
    """All 96 stack tensors in one launch (what an optimizer step sends) into an engine whose every derived copy is current."""
    w, pe = wf.state_after(-1)
    warm = wf.make_engine(w, pe, wf.MAX_ROWS)
    wf.consumers(warm)
    new = _all_layers_bumped(w)                                  # layers 0 and 7 change (the matrix's 24 tensors), the other 72 go up as they were
    wf.assert_visible((w, pe), (new, pe), "load_layers")
    warm.load_layers(wf.layer_list(new))
    wf.assert_same_bits(wf.consumers(warm), wf.consumers(wf.make_engine(new, pe, wf.MAX_ROWS)), "load_layers")


def _style_run(eng, styles, B):
    i = wf._inputs()
    x, t, txt = (i["xs"], i["ts"], i["txts"]) if B == wf.B_SMALL else (i["xl"], i["tl"], i["txtl"])
    eng.set_text(txt)
    eng.set_styles(styles)
    out = eng.forward(x, t)
    torch.cuda.synchronize()
    return out


def test_slot_reloads_on_a_warm_engine_under_styles():
    """load_layers_slot for slot 1, then a slot-0 change, while styles are set, at a small and a large batch (wsm_* and wqkv / wtail
    of the slot are both read); then style_slots grown from 3 to 4 after use: the earlier slots give the bits they gave before."""
    import style_fixture as sf
    eng = sf.make_engine(F, T, wf.B_LARGE, 3)
    st = {B: [(0, 1, 1, 2, 0, 2)[i % 6] for i in range(B)] for B in (wf.B_SMALL, wf.B_LARGE)}
    for B in st:
        _style_run(eng, st[B], B)                                # warm: every slot's copies built
    states = [dict(sf.style_weights(F, s)) for s in range(3)]
    for slot in (1, 0):
        old = states[slot]
        new = states[slot] = _all_layers_bumped(old)
        wf.assert_visible((old, sf.pe()), (new, sf.pe()), f"slot {slot}")
        eng.load_layers_slot(slot, sf.layer_list(new))
        fresh = sf.make_engine(F, T, wf.B_LARGE, 1)
        fresh.style_slots(3)
        for s in range(3):
            fresh.load_layers_slot(s, sf.layer_list(states[s]))
        for B in st:
            assert torch.equal(_style_run(eng, st[B], B), _style_run(fresh, st[B], B)), (slot, B)
    before = {B: _style_run(eng, st[B], B) for B in st}
    eng.style_slots(4)
    eng.load_layers_slot(3, sf.layer_list(sf.style_weights(F, 1)))
    for B in st:
        assert torch.equal(_style_run(eng, st[B], B), before[B]), B
    alone = sf.make_engine(F, T, wf.B_LARGE, 2)                  # slot 1 of this engine: style 1's original stack
    for B in st:
        rows = [i for i in range(B) if st[B][i] == 1]
        assert torch.equal(_style_run(eng, [3] * B, B)[rows], _style_run(alone, [1] * B, B)[rows]), B


def test_precise_mode_transitions_on_a_warm_engine():
    """default -> precise (re-upload from the remembered sources, one of them mutated in place since its load: its CURRENT values go
    up) -> default + load_layers -> precise again (only the layer tensors lack their lo halves).  Each state equals a fresh engine
    created in that mode.  Precise mode is the sampling path's; the training consumers run in the default states."""
    from mst_amd.engine import DenoiserEngine
    w, pe = wf.state_after(-1)
    sd = {k: torch.from_numpy(v.copy()) for k, v in w.items()}
    eng = DenoiserEngine(F, T, wf.MAX_ROWS, device=dev())
    eng.load_state_dict(sd, pe=torch.from_numpy(pe))
    wf.consumers(eng)
    name = f"{LP}0.linear1.weight"
    sd[name].mul_(1.25).add_(0.01 * torch.sign(sd[name]))        # in place, after the load: the engine holds a reference
    w1 = dict(w)
    w1[name] = sd[name].numpy().copy()
    wf.assert_visible((w, pe), (w1, pe), "mutated source")

    def fresh(state, precise):
        e = DenoiserEngine(F, T, wf.MAX_ROWS, device=dev())
        e.set_precise(precise)
        wf.load_all(e, state, pe)
        return e

    eng.set_precise(True)
    a, b = wf.consumers(eng, training=False), wf.consumers(fresh(w1, True), training=False)
    wf.assert_same_bits(a, b, "default -> precise")
    ref = wf.oracle_forward(w1, pe)
    assert rel_l2(b["forward/small"].cpu().numpy(), ref) < TOL
    w2 = _all_layers_bumped(w1)
    wf.assert_visible((w1, pe), (w2, pe), "load_layers after precise")
    keep = wf.layer_list(w2)
    eng.set_precise(False)
    eng.load_layers(keep)
    wf.assert_same_bits(wf.consumers(eng), wf.consumers(fresh(w2, False)), "precise -> default + load_layers")
    eng.set_precise(True)
    wf.assert_same_bits(wf.consumers(eng, training=False), wf.consumers(fresh(w2, True), training=False), "-> precise again")



def _loop(eng, B, frames, steps, seed=31):
    """An inpainting DDPM loop of `steps` steps with in-kernel noise on B clips (inputs seeded per shape, the same for every engine)."""
    from mst_amd.engine import SAMPLER_DDPM
    key = ("loop", B, frames)
    if key not in _B:
        n = lambda tag, shape: cu(syn_normal(f"wc/loop/{B}/{frames}/{tag}", shape))
        _B[key] = (n("x", (B, F, 1, frames)), n("motion", (B, F, 1, frames)), n("txt", (B, 512)),
                   cu(wf.syn.root_horizontal_mask(B, F, frames)))
    x, motion, txt, mask = _B[key]
    eng.set_text(txt)
    out = eng.sample_loop(wf._schedule(), x.clone(), steps - 1, 0, SAMPLER_DDPM, mask=mask, motion=motion, seed=seed)
    torch.cuda.synchronize()
    return out


def syn_normal(tag, shape):
    return wf.syn.normal(wf.SEED, tag, shape)


POSE = ("input_process.poseEmbedding.weight", "input_process.poseEmbedding.bias", "output_process.poseFinal.weight",
        "output_process.poseFinal.bias", "embed_timestep.time_embed.0.weight")


def _reload_for_a_loop(eng, w):
    """What a loop reads, changed on a warm engine: layers 0 and 7 through load_layers (wqkv, wtail, wsm_*), the pose projections
    (their packings) and one timestep-MLP matrix (the loop's hoisted timestep rows) through load_tensor.  -> the new state."""
    new = _all_layers_bumped(w)
    for name in POSE:
        new[PRIOR + name] = wf.bump_name(name, w[PRIOR + name])
    eng.load_layers(wf.layer_list(new))
    for name in POSE:
        eng.load_tensor(name, torch.from_numpy(new[PRIOR + name]))
    return new


@pytest.mark.parametrize("B", [17, 26], ids=["small-launch", "two-kernel"])
def test_reload_then_graph_replayed_loop(monkeypatch, B):
    """MST_GRAPH=1 (read at creation): capture, reload, replay.  8 steps at 2 steps per graph: the first loop runs 2 steps from the
    host, captures and replays 3 times; the loop after the reload is 4 replays of THAT graph and not one host-enqueued step, so the
    repacking launches cannot hide inside a step the host enqueues.  It must give the bits of a host-enqueued loop on a fresh engine
    with the new weights.  17 clips run the small-launch kernels in 2 slices (wsm_*), 26 clips the two-kernel path (wqkv, wtail)."""
    w, pe = wf.state_after(-1)
    monkeypatch.setenv("MST_GRAPH", "1")
    monkeypatch.setenv("MST_GRAPH_STEPS", "2")
    graph = wf.make_engine(w, pe, B)
    monkeypatch.setenv("MST_GRAPH", "0")
    host = wf.make_engine(w, pe, B)
    assert torch.equal(_loop(graph, B, T, 8), _loop(host, B, T, 8))              # captured here
    new = _reload_for_a_loop(graph, w)
    wf.assert_visible((w, pe), (new, pe), "reload between capture and replay")
    fresh = wf.make_engine(new, pe, B)                                           # host-enqueued (MST_GRAPH=0), never ran the old weights
    want = _loop(fresh, B, T, 8)
    assert torch.equal(_loop(graph, B, T, 8), want)
    assert not torch.equal(want, _loop(host, B, T, 8))
    assert torch.equal(_loop(graph, B, T, 9), _loop(fresh, B, T, 9))             # (and with a host-enqueued head: 1 step + 4 replays)


def test_reload_then_resident_trunk_loop(monkeypatch):
    """MST_TRUNK=1 (read at creation): the stack of a step as one resident launch, which reads wqkv / wtail through a table of
    pointers built at its first launch.  196 frames, 12 clips (the shapes the trunk takes); loop, reload, loop: the bits of the
    two-launches-per-layer path on a fresh engine with the new weights, and no hand-off wait gave up."""
    w, pe = wf.state_after(-1)
    B, frames = 12, 196
    monkeypatch.setenv("MST_TRUNK", "1")
    trunk = wf.make_engine(w, pe, B, frames=frames)
    monkeypatch.delenv("MST_TRUNK")
    plain = wf.make_engine(w, pe, B, frames=frames)
    assert torch.equal(_loop(trunk, B, frames, 3), _loop(plain, B, frames, 3))
    trunk.trunk_check()
    new = _reload_for_a_loop(trunk, w)
    wf.assert_visible((w, pe), (new, pe), "reload under the resident trunk")
    want = _loop(wf.make_engine(new, pe, B, frames=frames), B, frames, 3)
    assert torch.equal(_loop(trunk, B, frames, 3), want)
    trunk.trunk_check()
    assert not torch.equal(want, _loop(plain, B, frames, 3))


# =============================================================================================== 4. the style bank (module level)
def _bank_call(bank, B):
    i = wf._inputs()
    st = torch.tensor([(0, 1, 1, 2, 0, 2)[k % 6] for k in range(B)])
    with torch.no_grad():
        out = bank(i["xl"][:B], i["tl"][:B], {"text_embed": i["txtl"][:B], "style": st})
    torch.cuda.synchronize()
    return out, st


def _fresh_bank(models):
    from test_gpu_style_bank import _bank
    bank, fresh = _bank("xia")
    for a, b in zip(fresh, models):
        a.load_state_dict(b.state_dict())
    return bank


def test_bank_follows_its_members():
    """A StyleBank that has run: an optimizer step on member 1 changes only style 1's clips; a prior tensor written on member 0 (the
    bank's slot 0 carries the shared prior: a full reload); a larger batch (the bank's engine is rebuilt: every slot goes up again).
    After each, the bank gives the bits of a bank built fresh from its members' state."""
    from test_gpu_style_bank import _bank
    bank, models = _bank("xia")
    B = 6
    out0, st = _bank_call(bank, B)
    old = _state_np(models[1])
    params = models[1].parameters_wo_enc()
    g = torch.Generator(device="cpu").manual_seed(5)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).to(p.device)
    torch.optim.AdamW(params, lr=LR, weight_decay=0.0).step()
    wf.assert_visible(old, _state_np(models[1]), "a step on member 1")
    out1, _ = _bank_call(bank, B)
    rows, other = (st == 1).nonzero().flatten().tolist(), (st != 1).nonzero().flatten().tolist()
    assert torch.equal(out1[other], out0[other])
    assert torch.equal(out1, _bank_call(_fresh_bank(models), B)[0])
    i = wf._inputs()
    with torch.no_grad():                                        # member 1 alone, the same batch: the same kernels on the same rows
        own = models[1](i["xl"][:B], i["tl"][:B], {"text_embed": i["txtl"][:B]})
    assert torch.equal(out1[rows], own[rows])
    old = _state_np(models[0])
    with torch.no_grad():
        _p(models[0], PRIOR_T).copy_(_bumped(_p(models[0], PRIOR_T)))
    wf.assert_visible(old, _state_np(models[0]), "a prior tensor of member 0")
    fresh = _fresh_bank(models)
    assert torch.equal(_bank_call(bank, B)[0], _bank_call(fresh, B)[0])
    assert torch.equal(_bank_call(bank, 14)[0], _bank_call(fresh, 14)[0])    # regrowth
    assert torch.equal(_bank_call(bank, B)[0], _bank_call(fresh, B)[0])
    # a write through .data on member 2 moves neither version nor pointer: bank.mst_weights_changed() is the signal (the member's epoch)
    old = _state_np(models[2])
    _p(models[2], STACK_T).data.mul_(1.25)
    wf.assert_visible(old, _state_np(models[2]), "p.data.mul_ on member 2")
    bank.mst_weights_changed()
    got, want = _bank_call(bank, B)[0], _bank_call(_fresh_bank(models), B)[0]
    assert torch.equal(got, want)
    rows2 = (st == 2).nonzero().flatten().tolist()
    assert not torch.equal(got[rows2], out1[rows2])


def test_precise_switch_on_a_bank_is_refused_not_ignored():
    """The style-aware kernels have no precise variant (the engine refuses styles in precise mode).  member 0's switch reaches the
    bank's engine, built before or after the switch, so a bank call then RAISES instead of running in default precision; switched
    off again, the bank gives the bits it gave before."""
    from test_gpu_style_bank import _bank
    bank, models = _bank("xia")
    before = _bank_call(bank, 6)[0]
    models[0].set_precise(True)                                  # a running bank
    with pytest.raises(RuntimeError, match="precise"):
        _bank_call(bank, 6)
    with pytest.raises(RuntimeError, match="precise"):
        _bank_call(bank, 14)                                     # ... and the larger engine it builds now
    assert models[0].mst_engine(14, T, slot="style_bank")._precise_on
    models[0].set_precise(False)
    assert torch.equal(_bank_call(bank, 6)[0], before)
    bank2, models2 = _bank("xia")                                # a bank built after the switch
    models2[0].set_precise(True)
    with pytest.raises(RuntimeError, match="precise"):
        _bank_call(bank2, 6)
