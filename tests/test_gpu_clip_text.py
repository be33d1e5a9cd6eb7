"""The native CLIP text tower (csrc/mst_clip.h, mst_amd.model.clip_text) on the GPU against tests/golden/clip_text.npz: the float64
output of Hugging Face's CLIPTextModelWithProjection on tests/clip_text_fixture.py's seeded weights and token rows, with the fp32 and
fp16 modules' own distances to it (`d32`, `d16`, per prompt, max |a - f64| / max |f64|).

  1. every golden case, every prompt: finite, and the kernel's distance at most that prompt's d16 -- the error of the arithmetic the
     reference itself runs in (fp16 after clip.model.convert_weights).  No margin: the kernel's residual stream is fp32.
  2. a prompt's embedding is the same bits alone, at any position of a batch of 3 or 33, with zeros or arbitrary ids behind its
     end-of-text token, at context 22 padded to 77 or at context 77, on the default or a side stream.
  3. the 12-layer case is one of the cases of 1.
  4. through the model: use_native_text_encoder, encode_text == encode_tokens(tokenize(...)), and a 3-step ddim_sample_loop given
     y['text'] equals the loop given the embedding as y['text_embed'], bit for bit.
  5. every ABI refusal is named and leaves the output buffer untouched.

Each case prints `clip_text: <case> prompt <k> (end <e>) got <distance> d16 <d16> d32 <d32> ratio <got / d16>`.

Measured on an MI355X: kernel 1.4e-4 .. 4.7e-4 where d16 is 5.8e-4 .. 9.9e-4 and d32 3.2e-7 .. 7.6e-7; worst kernel / d16 ratio 0.644
(2 layers, end-of-text at 32), 0.285 at 12 layers, 0.597 at context 22.  The file takes 5 s (22 tests)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import clip_text_fixture as cf
import mst_amd  # noqa: F401
from conftest import GOLDEN
from mst_amd import _native as N
from mst_amd.model.clip_text import ClipTextEncoder, SimpleTokenizer

pytestmark = pytest.mark.gpu
MERGES = os.path.join(GOLDEN, "clip_toy_merges.txt")
_ENC = {}


def dev():
    return torch.device("cuda")


def encoder(layers):
    if layers not in _ENC:
        _ENC[layers] = ClipTextEncoder.from_state_dict(cf.state_dict(layers), dev())
    return _ENC[layers]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "clip_text.npz"))


@pytest.mark.parametrize("case", list(cf.CASES))
def test_every_prompt_is_within_the_fp16_modules_own_distance(case, golden):
    layers, _, ends = cf.CASES[case]
    got = encoder(layers).encode_tokens(torch.from_numpy(cf.case_ids(case))).cpu().numpy()
    assert got.shape == (len(ends), cf.WIDTH) and got.dtype == np.float32
    assert np.isfinite(got).all()
    dist, d16, d32 = cf.distance(got, golden[case + "|f64"]), golden[case + "|d16"], golden[case + "|d32"]
    for k, e in enumerate(ends):
        print(f"clip_text: {case} prompt {k} (end {e}) got {dist[k]:.3e} d16 {d16[k]:.3e} d32 {d32[k]:.3e} ratio {dist[k] / d16[k]:.3f}")
    assert (dist <= d16).all(), f"{case}: worst kernel / d16 ratio {float((dist / d16).max()):.3f}"


def test_a_prompt_encodes_to_the_same_bits_wherever_it_stands():
    enc = encoder(2)
    ids = cf.case_ids("l2")
    alone = torch.cat([enc.encode_tokens(torch.from_numpy(ids[k:k + 1])) for k in range(len(ids))])
    whole = enc.encode_tokens(torch.from_numpy(ids).to(dev()))                  # ids on the device
    assert torch.equal(alone, whole)
    for k in range(len(ids)):                                                   # every position of a batch of 3
        others = [ids[(k + 3) % len(ids)], ids[(k + 7) % len(ids)]]
        for pos in range(3):
            rows = others[:pos] + [ids[k]] + others[pos:]
            assert torch.equal(enc.encode_tokens(torch.from_numpy(np.stack(rows)))[pos], alone[k]), (k, pos)
    big = np.stack([ids[(5 * j + 2) % len(ids)] for j in range(33)])            # a batch of 33: every prompt three times, shuffled
    out = enc.encode_tokens(torch.from_numpy(big))
    for j in range(33):
        assert torch.equal(out[j], alone[(5 * j + 2) % len(ids)]), j


def test_nothing_behind_end_of_text_reaches_the_embedding():
    enc = encoder(2)
    zeros, junk = cf.case_ids("l2"), cf.case_ids("l2", tail="ids")
    assert (zeros != junk).any()
    assert torch.equal(enc.encode_tokens(torch.from_numpy(zeros)), enc.encode_tokens(torch.from_numpy(junk)))


def test_context_22_padded_to_77_is_context_77():
    enc = encoder(2)
    padded = cf.case_ids("c22")                                                  # built at 22 columns, zero-padded to 77
    short = padded[:, :22]
    wide = np.stack([cf.token_row("c22", k, e, 77) for k, e in enumerate(cf.CASES["c22"][2])])
    assert np.array_equal(wide[:, :22], short) and padded.shape[1] == 77
    a, b, c = (enc.encode_tokens(torch.from_numpy(np.ascontiguousarray(x))) for x in (padded, short, wide))
    assert torch.equal(a, b) and torch.equal(a, c)


def test_a_side_stream_gives_the_same_bits():
    enc = encoder(2)
    ids = torch.from_numpy(cf.case_ids("l2"))
    ref = enc.encode_tokens(ids)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = enc.encode_tokens(ids)
    side.synchronize()
    assert torch.equal(ref, got)


def test_through_the_model_text_and_text_embed_are_the_same_loop():
    from loop_fixture import F, T, build_model
    model, d = build_model(dev())
    mdm = model.motion_enc.mdm_model
    tok = SimpleTokenizer(MERGES)
    sd = cf.state_dict(2)
    keep = tok.vocab_size                                                        # the toy vocabulary's size: its last id is end-of-text
    sd["token_embedding.weight"] = np.ascontiguousarray(sd["token_embedding.weight"][:keep])
    enc = mdm.use_native_text_encoder(sd, MERGES)
    prompts = ["a person walks proudly"]
    emb = mdm.encode_text(prompts)
    want = 22 if mdm.dataset in ("humanml", "kit") else 77
    direct = enc.encode_tokens(tok.tokenize(prompts, context_length=want))
    assert emb.dtype == torch.float32 and emb.shape == (1, 512) and torch.equal(emb, direct)
    noise = torch.from_numpy(cf.syn.normal(cf.SEED, "clip/loop/noise", (1, F, 1, T))).to(dev())
    rest = {"mask": torch.ones(1, 1, 1, T, device=dev()),
            "inpainting_mask": torch.from_numpy(cf.syn.root_horizontal_mask(1, F, T)).to(dev()),
            "inpainted_motion": torch.from_numpy(cf.syn.normal(cf.SEED, "clip/loop/motion", (1, F, 1, T))).to(dev())}
    run = lambda y: d.ddim_sample_loop(model, (1, F, 1, T), noise=noise.clone(), clip_denoised=False, model_kwargs={"y": dict(rest, **y)},
                                       skip_timesteps=17, eta=0.0)
    a = run({"text": prompts})
    b = run({"text_embed": emb})
    assert torch.isfinite(a).all() and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------ ABI refusals
def _call(enc, out, **over):
    """mst_clip_encode on two one-token-pair prompts with one argument replaced."""
    lib = N.lib()
    ids = torch.tensor([[cf.SOT, cf.EOT], [cf.SOT, cf.EOT]], dtype=torch.int32, device=dev())
    lens = torch.tensor([2, 2], dtype=torch.int32, device=dev())
    offs = torch.tensor([0, 2], dtype=torch.int32, device=dev())
    ws = torch.empty(4 * 11264, dtype=torch.uint8, device=dev())
    w = N.MstClipWeights()
    C.memmove(C.byref(w), C.byref(enc._w), C.sizeof(w))
    for k in ("width", "heads", "ffn", "layers", "context", "tok_emb"):
        if k in over:
            setattr(w, k, over.pop(k))
    a = dict(ids=N.ptr(ids), batch=2, stride=2, lens=N.ptr(lens), offs=N.ptr(offs), rows=4, ws=N.ptr(ws), nbytes=ws.numel(),
             out=N.ptr(out))
    a.update(over)
    rc = lib.mst_clip_encode(C.byref(w), a["ids"], a["batch"], a["stride"], a["lens"], a["offs"], a["rows"], a["ws"], a["nbytes"],
                             a["out"], N.stream_ptr(dev()))
    torch.cuda.synchronize()
    return rc, lib.mst_last_error().decode()


REFUSALS = [("width", dict(width=768), "width 768"), ("heads", dict(heads=12), "heads 12"), ("ffn", dict(ffn=3072), "ffn 3072"),
            ("layers", dict(layers=0), "layers 0"), ("context", dict(context=78), "context 78"), ("table", dict(tok_emb=None), "null tensor"),
            ("ids", dict(ids=None), "null operand"), ("batch", dict(batch=0), "batch 0"), ("stride", dict(stride=78), "78 ids a prompt"),
            ("rows", dict(rows=5), "5 packed rows"), ("rows_low", dict(rows=1), "1 packed rows"), ("workspace", dict(nbytes=4 * 11264 - 1), "workspace of")]


@pytest.mark.parametrize("name,over,says", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_abi_refusals_are_named_and_touch_nothing(name, over, says):
    enc = encoder(2)
    out = torch.full((2, cf.WIDTH), -7.0, device=dev())
    rc, msg = _call(enc, out, **over)
    assert rc != 0 and msg.startswith("mst_clip_encode:") and says in msg, msg
    assert bool((out == -7.0).all())


def test_the_unrefused_call_of_the_refusal_harness_runs():
    enc = encoder(2)
    out = torch.full((2, cf.WIDTH), -7.0, device=dev())
    rc, msg = _call(enc, out)
    assert rc == 0, msg
    ref = enc.encode_tokens(torch.tensor([[cf.SOT, cf.EOT]]))
    assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[0])


def test_pack_and_plan_refusals_are_named():
    lib = N.lib()
    src = torch.zeros(64, 64, device=dev())
    dst = torch.full((64, 64), -7.0, dtype=torch.float16, device=dev())
    for n, k, says in ((40, 64, "40 output rows"), (64, 48, "48 input columns")):
        assert lib.mst_clip_pack_weight(N.ptr(src), 0, n, k, N.ptr(dst), N.stream_ptr(dev())) != 0
        assert says in lib.mst_last_error().decode()
    assert lib.mst_clip_pack_weight(None, 0, 64, 64, N.ptr(dst), N.stream_ptr(dev())) != 0
    torch.cuda.synchronize()
    assert bool((dst == -7.0).all())
    # f32 and f16 sources pack to the same halves
    w = torch.from_numpy(cf.state_dict(2)["transformer.resblocks.0.mlp.c_fc.weight"]).to(dev())
    a, b = torch.empty_like(w, dtype=torch.float16), torch.empty_like(w, dtype=torch.float16)
    assert lib.mst_clip_pack_weight(N.ptr(w), 0, w.shape[0], w.shape[1], N.ptr(a), N.stream_ptr(dev())) == 0
    h = w.half()
    assert lib.mst_clip_pack_weight(N.ptr(h), 1, w.shape[0], w.shape[1], N.ptr(b), N.stream_ptr(dev())) == 0
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a.float().flatten().sort().values, w.flatten().sort().values)
