"""CPU-side checks of the native CLIP text path (mst_amd.model.clip_text, csrc/mst_clip.h): the float64 numpy statement of the tower
(tests/clip_text_fixture.py) against the stored float64 goldens, the tokenizer against the golden ids, the state-dict layouts, every
Python-side refusal, and the ABI's shape (header, SIGNATURES, struct sizes, host-side refusals, the planner)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import clip_text_fixture as cf
import mst_amd  # noqa: F401
from conftest import GOLDEN
from mst_amd import _native as N
from mst_amd.model import clip_text as ct

MERGES = os.path.join(GOLDEN, "clip_toy_merges.txt")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "clip_text.npz"))


@pytest.mark.parametrize("case", list(cf.CASES))
def test_float64_statement_matches_the_golden(case, golden):
    """The statement and the oracle are both float64 and differ by float64 rounding in another order of summation.  The bar per prompt
    is the oracle's fp32 module's distance d32 scaled by the ratio of the unit roundoffs, 2^-53 / 2^-24, with a factor 64 of headroom
    for the order: a statement of other arithmetic (another activation, mask, scale or epsilon) misses it by orders of magnitude.
    Measured: 1.3e-15 against bars from 1.9e-14."""
    layers = cf.CASES[case][0]
    dist = cf.distance(cf.forward64(cf.state_dict(layers), cf.case_ids(case)), golden[case + "|f64"])
    bar = 64 * golden[case + "|d32"] * 2.0 ** -29
    print(f"clip_text statement: {case} worst {dist.max():.2e} bar {bar.min():.2e}")
    assert (dist <= bar).all()
    assert golden[case + "|f64"].shape == (len(cf.CASES[case][2]), 512)
    assert (golden[case + "|d32"] < golden[case + "|d16"]).all()


def test_golden_file_holds_every_case_and_is_small(golden):
    assert sorted(golden.files) == sorted(f"{c}|{k}" for c in cf.CASES for k in ("f64", "d32", "d16"))
    assert os.path.getsize(os.path.join(GOLDEN, "clip_text.npz")) < os.path.getsize(os.path.join(GOLDEN, "guided.npz"))


def test_tokenizer_matches_the_golden_ids():
    g = np.load(os.path.join(GOLDEN, "clip_tokens.npz"))
    tok = ct.SimpleTokenizer(MERGES)
    assert tok.vocab_size == 512 + len(cf.TOY_MERGES) + 2
    got = tok.tokenize(cf.TOY_STRINGS)
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(cf.TOY_STRINGS), 77)
    assert np.array_equal(got.numpy(), g["ids"])
    assert (got[:, 0] == tok.sot).all() and (got.max(dim=1).values == tok.eot).all()


def test_gzipped_merges_read_the_same(tmp_path):
    import gzip
    p = tmp_path / "merges.txt.gz"
    with open(MERGES, "rb") as fh:
        p.write_bytes(gzip.compress(fh.read()))
    a, b = ct.SimpleTokenizer(MERGES), ct.SimpleTokenizer(str(p))
    assert a.encoder == b.encoder and a.ranks == b.ranks


def test_truncation_puts_end_of_text_last():
    tok = ct.SimpleTokenizer(MERGES)
    long = cf.TOY_STRINGS[-1]
    for ctx in (22, 77):
        row = tok.tokenize([long], context_length=ctx)[0]
        assert row[-1] == tok.eot and int(row.argmax()) == ctx - 1 and (row[:-1] < tok.eot).all() and (row > 0).all()
    with pytest.raises(RuntimeError, match="too long"):
        tok.tokenize([long], context_length=22, truncate=False)


def test_context_22_padded_to_77_has_the_same_argmax():
    tok = ct.SimpleTokenizer(MERGES)
    enc = ct.ClipTextEncoder.__new__(ct.ClipTextEncoder)          # the tokenize rule alone: no device
    enc.tokenizer = tok
    for dataset, strings in (("humanml", cf.TOY_STRINGS), ("kit", cf.TOY_STRINGS[:3])):
        enc.dataset = dataset
        padded = enc.tokenize(strings)
        short = tok.tokenize(strings, context_length=22)
        assert tuple(padded.shape) == (len(strings), 77) and torch.equal(padded[:, :22], short) and not padded[:, 22:].any()
        assert torch.equal(padded.argmax(dim=1), short.argmax(dim=1))
    enc.dataset = "stylexia_posrot"
    assert torch.equal(enc.tokenize(cf.TOY_STRINGS), tok.tokenize(cf.TOY_STRINGS, context_length=77))


def test_both_state_dict_layouts_map_to_identical_tables():
    sd = cf.state_dict(2)
    a = ct.weight_table(sd)
    b = ct.weight_table({k: torch.from_numpy(v) for k, v in cf.to_hf(sd).items()})
    assert len(a["layers"]) == len(b["layers"]) == 2
    for k in ("tok_emb", "pos_emb", "lnf_g", "lnf_b", "proj"):
        assert torch.equal(a[k], b[k]) and a[k].is_contiguous() and b[k].is_contiguous(), k
    for la, lb in zip(a["layers"], b["layers"]):
        assert sorted(la) == sorted(ct.LAYER_FIELDS)
        for k in ct.LAYER_FIELDS:
            assert torch.equal(la[k], lb[k]), k
    assert torch.equal(a["proj"], torch.from_numpy(sd["text_projection"]))       # applied as x @ P
    assert tuple(a["layers"][0]["wqkv"].shape) == (1536, 512)
    half = ct.weight_table({k: torch.from_numpy(v).half() for k, v in sd.items()})    # an f16 checkpoint holds the same table
    assert torch.equal(half["layers"][1]["w2"], a["layers"][1]["w2"])


def test_python_side_refusals_name_their_reason():
    sd = cf.state_dict(1)
    with pytest.raises(ValueError, match="token id 1024 out of range"):
        ct.check_token_array(np.array([[cf.SOT, 1024, cf.EOT]]), cf.VOCAB, 77)
    with pytest.raises(ValueError, match="token id -1 out of range"):
        ct.check_token_array(np.array([[cf.SOT, -1, cf.EOT]]), cf.VOCAB, 77)
    with pytest.raises(ValueError, match="row 1 holds no end-of-text"):
        ct.check_token_array(np.array([[cf.SOT, 3, cf.EOT], [cf.SOT, 3, 4]]), cf.VOCAB, 77)
    with pytest.raises(ValueError, match="context 78 above"):
        ct.check_token_array(np.zeros((1, 78), dtype=np.int64), cf.VOCAB, 77)
    ids, lens = ct.check_token_array(np.array([[cf.SOT, cf.EOT, 5, cf.EOT], [cf.SOT, 7, 9, cf.EOT]]), cf.VOCAB, 77)
    assert lens.tolist() == [2, 4]                                               # the FIRST maximum is the end-of-text position
    wide = dict(sd)
    wide["token_embedding.weight"] = np.zeros((8, 768), dtype=np.float32)
    with pytest.raises(ValueError, match="width 768"):
        ct.weight_table(wide)
    big = dict(sd)
    big["transformer.resblocks.0.mlp.c_fc.weight"] = sd["transformer.resblocks.0.mlp.c_fc.weight"] * 0 + 70000.0
    with pytest.raises(ValueError, match=r"layers\.0\.w1 does not fit f16"):
        ct.weight_table(big)
    ffn = dict(sd)
    ffn["transformer.resblocks.0.mlp.c_fc.weight"] = np.zeros((3072, 512), dtype=np.float32)
    with pytest.raises(ValueError, match="ffn 3072"):
        ct.weight_table(ffn)
    long = dict(sd)
    long["positional_embedding"] = np.zeros((78, 512), dtype=np.float32)
    with pytest.raises(ValueError, match="context 78"):
        ct.weight_table(long)
    with pytest.raises(ValueError, match="neither"):
        ct.weight_table({"foo": np.zeros(3)})
    with pytest.raises(RuntimeError, match="GPU only"):
        ct.ClipTextEncoder(ct.weight_table(sd), "cpu")


def test_encode_text_without_an_encoder_still_raises_as_before():
    from mst_amd.model.mdm_forstyledataset import MDM
    m = MDM.__new__(MDM)
    torch.nn.Module.__init__(m)
    m.p = torch.nn.Parameter(torch.zeros(1))
    m._text_encoder, m.clip_model = None, None
    with pytest.raises(RuntimeError, match=r"CLIP is not installed: pass y\['text_embed'\] or call set_text_encoder\(fn\)"):
        m.encode_text(["a person walks"])


def test_header_signatures_and_struct_sizes_agree():
    text = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "mst_engine.h")).read()
    for name in ("mst_clip_pack_weight", "mst_clip_plan", "mst_clip_encode"):
        assert name in N.SIGNATURES and f"int {name}(" in text
    assert len(N.SIGNATURES["mst_clip_encode"][1]) == 11 and len(N.SIGNATURES["mst_clip_plan"][1]) == 6
    assert C.sizeof(N.MstClipLayer) == 12 * 8                                    # 12 pointers
    assert C.sizeof(N.MstClipWeights) == 6 * 4 + 6 * 8 and N.MstClipWeights.tok_emb.offset == 24
    import re
    body = re.search(r"typedef struct mst_clip_layer \{(.*?)\} mst_clip_layer;", text, re.S).group(1)
    assert re.findall(r"(\w+)_dev;", body) == list(ct.LAYER_FIELDS)


def test_planner_and_host_side_refusals_without_a_gpu():
    lib = N.lib()
    i32p = C.POINTER(C.c_int32)
    lens = np.array([2, 16, 77, 1], dtype=np.int32)
    offs = np.zeros(4, dtype=np.int32)
    rows, nbytes = C.c_int32(), C.c_int64()
    assert lib.mst_clip_plan(lens.ctypes.data_as(i32p), 4, 77, offs.ctypes.data_as(i32p), C.byref(rows), C.byref(nbytes)) == 0
    assert offs.tolist() == [0, 2, 18, 95] and rows.value == 96
    assert nbytes.value == 96 * (512 * 4 + 512 * 2 + 1536 * 2 + 512 * 2 + 2048 * 2)
    assert lib.mst_clip_plan(lens.ctypes.data_as(i32p), 4, 22, offs.ctypes.data_as(i32p), C.byref(rows), C.byref(nbytes)) != 0
    assert b"prompt 2 has 77 live rows" in lib.mst_last_error()
    assert lib.mst_clip_plan(lens.ctypes.data_as(i32p), 4, 78, offs.ctypes.data_as(i32p), C.byref(rows), C.byref(nbytes)) != 0
    assert b"context 78" in lib.mst_last_error()
    w = N.MstClipWeights(layers=1, vocab=8, context=77, width=768, heads=12, ffn=3072)
    one = C.c_void_p(16)                                                         # never dereferenced: the refusal comes first
    assert lib.mst_clip_encode(C.byref(w), one, 1, 2, one, one, 2, one, 1 << 20, one, None) != 0
    assert b"width 768" in lib.mst_last_error()
    assert lib.mst_clip_pack_weight(one, 0, 24, 64, one, None) != 0
    assert b"24 output rows" in lib.mst_last_error()
