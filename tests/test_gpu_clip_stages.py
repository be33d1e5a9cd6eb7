"""Every kernel of the CLIP text tower (csrc/mst_clip.h) against float64, one stage at a time, over every packed row and column.

mst_clip_encode works in a workspace the caller owns (x f32 [M][512] | h f16 [M][512] | qkv f16 [M][1536] | att f16 [M][512] | u f16
[M][2048]) that still holds every stage's output after the call.  Towers with altered weights (tests/clip_stage_fixture.py: real-1,
mid-1, emb-1, next-2, small-2, and the 12-layer tower called with `layers` = 1 .. 12) make every stage's input and output observable
as bits; each check feeds the kernel's own input buffers to a float64 numpy statement of that one stage.

  1. what licenses combining the runs: mid-1's qkv, att, h and u are real-1's bits, next-2's stream is real-1's, emb-1's and small-2's
     streams are the embedding, and every call leaves the bytes behind its workspace and behind its output rows untouched.
  2. the ten stages (embed, its LayerNorm, QKV, attention, out-proj, its LayerNorm2, FFN1, FFN2, its next LayerNorm1, final) on row set
     A (M = 350) and on M = 64, 1, 33, 16 and 81; embed is bit-equal, the others are held to the fixture's bar.
  3. the four LayerNorm sites on small-2, whose rows have a variance within a factor 10 of eps.
  4. trunc-12: the fp32 stream after layer k against a float64 statement of layer k (rounding h, qkv, att and u to f16 as the kernels
     do) fed the kernel's stream after layer k - 1, k = 1 .. 12.
  5. the pack kernel's layout, index by index.

Bars: fp32 outputs 4 d32 rowmax; f16 outputs half an f16 ulp of the float64 value + 4 d32 rowmax; d32 = the fp32 numpy restatement's
own distance, measured on the same inputs.  tests/test_clip_stages_cpu.py shows that the bars catch a wrong eps, divisor, constant,
bias column, tile, row pairing, clamp, scale, mask and pooled row.

Each check prints `clip_stage: <tower> <stage> rows <set> worst <ratio of the bar> d32 <value>`.

Measured on an MI355X, no kernel changed (worst ratio of the bar over the six row sets; d32 on row set A, over the sets in brackets):

    embed           bit-equal on every set
    embed_ln1       0.997   d32 1.8e-7 (1.1e-7 .. 1.9e-7)        small-2 embed     0.997   d32 1.7e-7
    qkv             0.991   d32 1.4e-6 (2.4e-7 .. 1.4e-6)
    attn            0.996   d32 5.5e-7 (0 at M = 1 .. 5.5e-7)
    outproj         0.406   d32 2.7e-7 (8.4e-8 .. 2.7e-7)
    ln2             0.998   d32 1.8e-7 (6.9e-8 .. 1.8e-7)        small-2 outproj   0.995   d32 1.6e-7
    ffn1            0.996   d32 1.1e-6 (1.8e-7 .. 1.1e-6)
    ffn2            0.409   d32 2.5e-7 (1.6e-7 .. 3.6e-7)
    next_ln1        0.997   d32 1.7e-7 (9.0e-8 .. 1.7e-7)        small-2 ffn2      0.998   d32 1.8e-7
    final           0.569   d32 8.2e-7 (3.2e-7 .. 8.2e-7)        small-2 final     0.335   d32 7.2e-7
    trunc-12        0.532 at layer 1, 0.158 .. 0.283 behind it; d32 8.9e-5 at layer 1 falling to 5.7e-6 at layer 12 (it carries the
                    f16 roundings of h, qkv, att and u that fall the other way in fp32 than in float64)

The f16 stages sit just under 1 by construction: the bar is half an ulp plus the small fp32 term, and over 10^5 elements some value
always lies next to a rounding tie.  The fp32 stages use 0.41 .. 0.57 of the bar with the restatement summed in numpy's own order;
no restatement had to be moved toward the kernels' order.  The file takes 6 s (73 tests)."""
import ctypes as C

import numpy as np
import pytest
import torch

import clip_stage_fixture as sf
import clip_text_fixture as cf
import mst_amd  # noqa: F401
from mst_amd import _native as N
from mst_amd.model.clip_text import ClipTextEncoder

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 4096, 0xA5
_ENC, _RUN, _W = {}, {}, {}


def dev():
    return torch.device("cuda")


def encoder(tower):
    if tower not in _ENC:
        _ENC[tower] = ClipTextEncoder.from_state_dict(sf.tower_sd(tower), dev())
    return _ENC[tower]


def stage_weights():
    if "stage" not in _W:
        _W["stage"], _W["site"] = sf.stage_weights(), sf.site_weights()
    return _W["stage"]


def run(tower, rows, layers=None):
    """mst_clip_encode of a tower on a row set, in a workspace and an output buffer with a sentinel region behind their last documented
    byte -> {x, h, qkv, att, u, out} on the host.  Cached: nothing changes a result."""
    key = (tower, rows, layers)
    if key in _RUN:
        return _RUN[key]
    enc, lib = encoder(tower), N.lib()
    ids, lens = sf.rowset_ids(rows)
    B, stride, M = len(lens), ids.shape[1], int(sum(lens))
    lens32, offs = np.asarray(lens, dtype=np.int32), np.zeros(B, dtype=np.int32)
    planned, nbytes = C.c_int32(), C.c_int64()
    i32p = C.POINTER(C.c_int32)
    N.check(lib.mst_clip_plan(lens32.ctypes.data_as(i32p), B, enc.context, offs.ctypes.data_as(i32p), C.byref(planned), C.byref(nbytes)))
    assert planned.value == M and nbytes.value == M * sf.WS_ROW_BYTES and np.array_equal(offs, sf.offsets(lens))
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev())
    ids_d, lens_d, offs_d = put(ids), put(lens32), put(offs)
    ws = torch.full((nbytes.value + GUARD,), SENTINEL, dtype=torch.uint8, device=dev())
    out = torch.full((B * sf.WIDTH * 4 + GUARD,), SENTINEL, dtype=torch.uint8, device=dev())
    w = N.MstClipWeights()
    C.memmove(C.byref(w), C.byref(enc._w), C.sizeof(w))
    if layers is not None:
        w.layers = layers
    rc = lib.mst_clip_encode(C.byref(w), N.ptr(ids_d), B, stride, N.ptr(lens_d), N.ptr(offs_d), M, N.ptr(ws), nbytes.value, N.ptr(out),
                             N.stream_ptr(dev()))
    torch.cuda.synchronize()
    assert rc == 0, lib.mst_last_error().decode()
    ws, out = ws.cpu().numpy(), out.cpu().numpy()
    assert (ws[nbytes.value:] == SENTINEL).all(), f"{tower} {rows}: bytes behind the workspace were written"
    assert (out[B * sf.WIDTH * 4:] == SENTINEL).all(), f"{tower} {rows}: bytes behind the output rows were written"
    r, at = {"out": out[:B * sf.WIDTH * 4].view(np.float32).reshape(B, sf.WIDTH).copy()}, 0
    for name, dt, cols in (("x", np.float32, 512), ("h", np.float16, 512), ("qkv", np.float16, 1536), ("att", np.float16, 512),
                           ("u", np.float16, 2048)):
        n = M * cols * np.dtype(dt).itemsize
        r[name] = ws[at:at + n].view(dt).reshape(M, cols).copy()
        at += n
    assert at == nbytes.value and all(np.isfinite(v).all() for v in r.values()), f"{tower} {rows}"
    _RUN[key] = r
    return r


def bits(a):
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def operands(rows):
    """The fixture's operand dict from the kernels' own buffers."""
    real, mid, emb, nxt = (run(t, rows) for t in ("real-1", "mid-1", "emb-1", "next-2"))
    ids, lens = sf.rowset_ids(rows)
    return {"ids": ids, "lens": lens, "x_emb": emb["x"], "ln1": emb["qkv"][:, :512], "qkv": real["qkv"], "att": real["att"], "x_mid": mid["x"],
            "h": real["h"], "u": real["u"], "x_out": real["x"], "x_next": nxt["x"], "ln1_next": nxt["qkv"][:, :512], "out": real["out"]}


@pytest.mark.parametrize("rows", sf.STAGE_SETS)
def test_the_towers_may_be_combined(rows):
    real, mid, emb, nxt = (run(t, rows) for t in ("real-1", "mid-1", "emb-1", "next-2"))
    for k in ("qkv", "att", "h", "u"):                                            # mid-1 differs from real-1 behind u only
        assert np.array_equal(bits(mid[k]), bits(real[k])), k
    assert np.array_equal(bits(nxt["x"]), bits(real["x"]))                        # next-2's layer 1 adds exact zeros
    assert np.array_equal(bits(emb["qkv"][:, 512:]), bits(real["qkv"][:, 512:]))  # emb-1's K and V are real-1's: the same LayerNorm1 bits


@pytest.mark.parametrize("rows", sf.STAGE_SETS)
def test_embedding_is_the_exact_sum(rows):
    W, B = stage_weights(), operands(rows)
    want = sf.statement("embed", B, W, np.float32)                                # f16 + f16 in fp32 is exact
    assert np.array_equal(bits(B["x_emb"]), bits(want))
    print(f"clip_stage: emb-1 embed rows {rows} worst 0.000 d32 0.000e+00")


TOWER_OF = {"embed_ln1": "emb-1", "qkv": "real-1", "attn": "real-1", "outproj": "mid-1", "ln2": "real-1", "ffn1": "real-1", "ffn2": "real-1",
            "next_ln1": "next-2", "final": "real-1"}


@pytest.mark.parametrize("rows", sf.STAGE_SETS)
@pytest.mark.parametrize("stage", sf.STAGES[1:])
def test_stage_against_float64(stage, rows):
    worst, d32 = sf.judge(stage, operands(rows), stage_weights())
    print(f"clip_stage: {TOWER_OF[stage]} {stage} rows {rows} worst {worst:.3f} d32 {d32:.3e}")
    assert worst < 1.0


@pytest.mark.parametrize("site", list(sf.SITES))
def test_layernorm_sites_at_variance_near_eps(site):
    stage_weights()
    W = _W["site"]
    one, two = run("small-2", "A", layers=1), run("small-2", "A")
    ids, lens = sf.rowset_ids("A")
    x = sf.embed(ids, lens, W["tok"], W["pos"], np.float32)
    assert np.array_equal(bits(one["x"]), bits(x)) and np.array_equal(bits(two["x"]), bits(x))   # the stream is the embedding at every site
    S = {"ids": ids, "lens": lens, "x": x, "ln1": one["qkv"][:, :512], "h": two["h"], "ln1_next": two["qkv"][:, :512], "out": two["out"]}
    worst, d32 = sf.judge_site(site, S, W)
    print(f"clip_stage: small-2 {site}_ln rows A worst {worst:.3f} d32 {d32:.3e}")
    assert worst < 1.0
    if site == "final":                                                           # the call of one layer pools the same stream
        assert np.array_equal(bits(one["out"]), bits(two["out"]))


def test_stream_after_every_layer_of_the_truncated_tower():
    sd = sf.tower_sd("trunc-12")
    ids, lens = sf.rowset_ids("T")
    w = [sf.weights(sd, k) for k in range(12)]
    x = sf.embed(ids, lens, w[0]["tok"], w[0]["pos"], np.float32)
    worst = []
    for k in range(1, 13):
        got = run("trunc-12", "T", layers=k)["x"]
        ref, _ = sf.layer(x, w[k - 1], lens, np.float64, lambda a: sf.f16(a).astype(np.float64))
        rest, _ = sf.layer(x, w[k - 1], lens, np.float32, lambda a: sf.f16(a).astype(np.float32))
        d32 = sf.d32_of(rest, ref)
        worst.append(sf.ratio(got, ref, d32, False))
        print(f"clip_stage: trunc-12 layer_{k} rows T worst {worst[-1]:.3f} d32 {d32:.3e}")
        x = got                                                                   # the next layer is fed the kernel's stream
    full = encoder("trunc-12").encode_tokens(torch.from_numpy(np.pad(ids, ((0, 0), (0, 77 - ids.shape[1])))))
    assert np.array_equal(bits(full.cpu().numpy()), bits(run("trunc-12", "T", layers=12)["out"]))
    assert max(worst) < 1.0, worst


@pytest.mark.parametrize("n,k", [(64, 64), (2048, 512)])
def test_pack_layout_index_by_index(n, k):
    """dst[((nt K/32 + ks) 64 + lane) 8 + j] == W[16 nt + (lane & 15)][32 ks + 8 (lane >> 4) + j], from f32 and from f16 sources.  The
    64 x 64 matrix holds 4096 distinct f16 values; f16 has fewer finite values than the 2048 x 512 matrix has elements, which therefore
    cycles through 63467 of them (a prime: no row, column, tile or lane step maps the matrix onto itself)."""
    lib = N.lib()
    finite = np.arange(1 << 16, dtype=np.uint16)
    finite = finite[(finite & 0x7C00) != 0x7C00]                                  # no inf, no NaN; -0 and the subnormals stay
    finite = finite[np.random.default_rng(cf.SEED).permutation(len(finite))][:63467]
    w16 = finite[np.arange(n * k) % len(finite)].reshape(n, k).view(np.float16)
    assert len(finite) == 63467 and (n * k > 4096 or len(np.unique(bits(w16))) == n * k)
    nt, ks, lane, j = np.meshgrid(np.arange(n // 16), np.arange(k // 32), np.arange(64), np.arange(8), indexing="ij")
    want = w16[16 * nt + (lane & 15), 32 * ks + 8 * (lane >> 4) + j].reshape(-1)
    for src in (torch.from_numpy(w16.astype(np.float32)), torch.from_numpy(w16)):
        src = src.to(dev())
        dst = torch.zeros(n * k + 64, dtype=torch.float16, device=dev())
        assert lib.mst_clip_pack_weight(N.ptr(src), int(src.dtype == torch.float16), n, k, N.ptr(dst), N.stream_ptr(dev())) == 0
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert np.array_equal(bits(got[:n * k]), bits(want)), src.dtype
        assert not bits(got[n * k:]).any()                                        # nothing behind the last fragment
