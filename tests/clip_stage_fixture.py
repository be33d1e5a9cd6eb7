"""Shared by tests/test_clip_stages_cpu.py and tests/test_gpu_clip_stages.py: the CLIP text tower of csrc/mst_clip.h one stage at a
time.  A stage is one kernel, or one epilogue of k_clip_gemm; `statement(stage, B, W, dt)` states it in numpy at dtype `dt` over the
stage's own input buffers, taken from the operand dict `B`, and `judge` holds an output buffer to the float64 statement.

Operands (`B`): what mst_clip_encode leaves in the caller's workspace, combined from towers with altered weights (`tower_sd`):

    x_emb    f32 [M][512]   the embedding                              x of emb-1
    ln1      f16 [M][512]   LayerNorm1 of layer 0                      qkv[:, :512] of emb-1 (identity Q)
    qkv      f16 [M][1536]                                             real-1
    att      f16 [M][512]                                              real-1
    x_mid    f32 [M][512]   the stream after out-proj                  x of mid-1 (c_proj zero)
    h        f16 [M][512]   LayerNorm2 of x_mid                        real-1
    u        f16 [M][2048]  QuickGELU(FFN1)                            real-1
    x_out    f32 [M][512]   the stream after the layer                 x of real-1
    x_next   f32 [M][512]   the same, layer 1 following                x of next-2
    ln1_next f16 [M][512]   LayerNorm1 of layer 1 from FFN2's epilogue qkv[:, :512] of next-2
    out      f32 [B][512]                                              real-1

`host_operands` makes the same dict without a GPU: the float64 statements chained, each output rounded the way its stage rounds.

The bar (per element, rowmax = the row's largest |float64 statement|):  fp32 outputs 4 d32 rowmax;  f16 outputs half an f16 ulp of the
float64 statement + 4 d32 rowmax.  d32 is measured: the largest |fp32 statement - float64 statement| / rowmax of the same stage on
the same inputs, the fp32 statement left unrounded.  The factor 4 is the project's convention for an fp32 kernel against its fp32
restatement (another summation order, the device's expf and sqrtf)."""
import numpy as np

import clip_text_fixture as cf

WIDTH, FFN, HEADS, HD, EPS = cf.WIDTH, cf.FFN, cf.HEADS, 64, 1e-5
WS_ROW_BYTES = WIDTH * 4 + WIDTH * 2 + 3 * WIDTH * 2 + WIDTH * 2 + FFN * 2        # x | h | qkv | att | u of one packed row

# live rows per prompt.  A: every wave-tail count of attention's 4-row trips, both sides of the lane + 64 key half, prompts across
# 32-row tiles, M = 350 = 10 * 32 + 30.  B<r>: M % 32 = r -- a full last tile (64), one row (1), one row in the second tile (33), a dead
# upper accumulator half (16), one live row in it (81 = 2 * 32 + 17).  T: the prompts of the truncated 12-layer tower.
ROWSETS = {"A": (1, 2, 3, 4, 5, 63, 64, 65, 66, 77), "B0": (20, 44), "B1": (1,), "B33": (16, 17), "B16": (7, 9), "B17": (77, 3, 1),
           "T": (8, 22, 77)}
STAGE_SETS = ("A", "B0", "B1", "B33", "B16", "B17")

STAGES = ("embed", "embed_ln1", "qkv", "attn", "outproj", "ln2", "ffn1", "ffn2", "next_ln1", "final")
OUTPUT = {"embed": "x_emb", "embed_ln1": "ln1", "qkv": "qkv", "attn": "att", "outproj": "x_mid", "ln2": "h", "ffn1": "u", "ffn2": "x_out",
          "next_ln1": "ln1_next", "final": "out"}
F16_OUT = {"embed": False, "embed_ln1": True, "qkv": True, "attn": True, "outproj": False, "ln2": True, "ffn1": True, "ffn2": False,
           "next_ln1": True, "final": False}
# the four LayerNorm sites of small-2: site -> (operand holding its output, f16 output?)
SITES = {"embed": ("ln1", True), "outproj": ("h", True), "ffn2": ("ln1_next", True), "final": ("out", False)}


def rowset_ids(name):
    """-> (int64 ids [B][longest prompt], zero behind a prompt's end-of-text; lens)."""
    lens = ROWSETS[name]
    ids = np.zeros((len(lens), max(lens)), dtype=np.int64)
    for k, n in enumerate(lens):
        ids[k, :n] = cf.token_row("stage/" + name, k, n - 1)[:n]
    return ids, lens


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------- towers
def _zero(sd, layer, *names):
    for n in names:
        for leaf in (".weight", ".bias"):
            k = f"transformer.resblocks.{layer}.{n}{leaf}"
            sd[k] = np.zeros_like(sd[k])


def _identity_q(sd, layer):
    p = f"transformer.resblocks.{layer}.attn."
    w, b = sd[p + "in_proj_weight"].copy(), sd[p + "in_proj_bias"].copy()
    w[:WIDTH], b[:WIDTH] = np.eye(WIDTH, dtype=w.dtype), 0.0
    sd[p + "in_proj_weight"], sd[p + "in_proj_bias"] = w, b


def small_shift():
    """The power of two s (tables scaled by 2^-s) that centres the variances of row set A's embedding rows on eps."""
    sd = cf.state_dict(1)
    ids, lens = rowset_ids("A")
    v = embed(ids, lens, sd["token_embedding.weight"], sd["positional_embedding"], np.float64).var(-1)
    return int(round(0.5 * np.log2(np.sqrt(v.min() * v.max()) / EPS)))


def tower_sd(name):
    """The OpenAI-layout state dict of a tower; every edit is exactly representable in f16."""
    if name == "trunc-12":
        return cf.state_dict(12)
    sd = dict(cf.state_dict(1 if name.endswith("-1") else 2))
    if name == "mid-1":
        _zero(sd, 0, "mlp.c_proj")
    elif name == "emb-1":
        _zero(sd, 0, "attn.out_proj", "mlp.c_proj")
        _identity_q(sd, 0)
    elif name in ("next-2", "small-2"):
        _zero(sd, 1, "attn.out_proj", "mlp.c_proj")
        _identity_q(sd, 1)
        if name == "small-2":
            # the stream is the (small) embedding at every LayerNorm site; identity Q in layer 0 too, so that a call truncated to one
            # layer shows the embed kernel's LayerNorm.  A scaled value that falls below f16's normal range is rounded to f16 again.
            _zero(sd, 0, "attn.out_proj", "mlp.c_proj")
            _identity_q(sd, 0)
            for k in ("token_embedding.weight", "positional_embedding"):
                sd[k] = cf._f16(sd[k] * 2.0 ** -small_shift())
    elif name != "real-1":
        raise KeyError(name)
    return sd


def weights(sd, layer=0):
    """float64 operands of one layer and of the tower's ends, by the names of the C ABI."""
    p = f"transformer.resblocks.{layer}."
    src = {"tok": "token_embedding.weight", "pos": "positional_embedding", "lnf_g": "ln_final.weight", "lnf_b": "ln_final.bias",
           "proj": "text_projection", "ln1_g": p + "ln_1.weight", "ln1_b": p + "ln_1.bias", "wqkv": p + "attn.in_proj_weight",
           "bqkv": p + "attn.in_proj_bias", "wo": p + "attn.out_proj.weight", "bo": p + "attn.out_proj.bias", "ln2_g": p + "ln_2.weight",
           "ln2_b": p + "ln_2.bias", "w1": p + "mlp.c_fc.weight", "b1": p + "mlp.c_fc.bias", "w2": p + "mlp.c_proj.weight",
           "b2": p + "mlp.c_proj.bias"}
    return {k: np.asarray(sd[v], dtype=np.float64) for k, v in src.items()}


def stage_weights():
    """Layer 0 and the ends of real-1, and (ln1n_g, ln1n_b) LayerNorm1 of next-2's layer 1."""
    w = weights(tower_sd("real-1"))
    nxt = weights(tower_sd("next-2"), 1)
    w["ln1n_g"], w["ln1n_b"] = nxt["ln1_g"], nxt["ln1_b"]
    return w


def site_weights():
    """small-2: LayerNorm site -> (gain, bias) of the LayerNorm the site applies, and the projection."""
    sd = tower_sd("small-2")
    l0, l1 = weights(sd, 0), weights(sd, 1)
    return {"embed": (l0["ln1_g"], l0["ln1_b"]), "outproj": (l1["ln2_g"], l1["ln2_b"]), "ffn2": (l1["ln1_g"], l1["ln1_b"]),
            "final": (l0["lnf_g"], l0["lnf_b"]), "proj": l0["proj"], "tok": l0["tok"], "pos": l0["pos"]}


# ------------------------------------------------------------------------------------------------ the stages, at any dtype
def f16(a):
    return np.asarray(a).astype(np.float16)


def embed(ids, lens, tok, pos, dt, shift=0):
    rows = [tok[ids[b, :n]].astype(dt) + pos[(np.arange(n) + shift) % len(pos)].astype(dt) for b, n in enumerate(lens)]
    return np.concatenate(rows)


def layernorm(x, g, b, dt, eps=EPS, div=WIDTH):
    x = np.asarray(x).astype(dt)
    c = x - x.mean(-1, keepdims=True, dtype=dt)
    v = (c * c).sum(-1, keepdims=True, dtype=dt) / dt(div)
    return c / np.sqrt(v + dt(eps)) * g.astype(dt) + b.astype(dt)


def linear(a, w, bias, dt):
    return np.asarray(a).astype(dt) @ w.astype(dt).T + bias.astype(dt)


def quickgelu(u, dt, c=1.702):
    return u / (dt(1) + np.exp(-dt(c) * u))


def attention(qkv, lens, dt, scale=0.125, see=0, drop=None):
    """Causal attention per prompt over packed rows.  Mutant switches: another score scale, `see` keys past the diagonal visible, key
    `drop` never visible."""
    qkv = np.asarray(qkv).astype(dt)
    out = np.zeros((len(qkv), WIDTH), dtype=dt)
    off = 0
    for n in lens:
        q, k, v = (qkv[off:off + n, j * WIDTH:(j + 1) * WIDTH].reshape(n, HEADS, HD).transpose(1, 0, 2) for j in range(3))
        i, j = np.arange(n)[:, None], np.arange(n)[None, :]
        vis = j <= np.minimum(i + see, n - 1)
        if drop is not None:
            vis = vis & (j != drop)
        s = np.where(vis, (q @ k.transpose(0, 2, 1)) * dt(scale), dt(-np.inf))
        p = np.exp(s - s.max(-1, keepdims=True))
        out[off:off + n] = ((p @ v) / p.sum(-1, keepdims=True, dtype=dt)).transpose(1, 0, 2).reshape(n, WIDTH)
        off += n
    return out


def final(x, lens, g, b, proj, dt, back=0):
    rows = np.maximum(offsets(lens) + np.asarray(lens) - 1 - back, 0)
    return layernorm(np.asarray(x)[rows], g, b, dt) @ proj.astype(dt)


def statement(stage, B, W, dt):
    """The stage over its own input buffers, at dtype dt, unrounded."""
    if stage == "embed":
        out = embed(B["ids"], B["lens"], W["tok"], W["pos"], dt)
    elif stage == "embed_ln1":
        out = layernorm(B["x_emb"], W["ln1_g"], W["ln1_b"], dt)
    elif stage == "qkv":
        out = linear(B["ln1"], W["wqkv"], W["bqkv"], dt)
    elif stage == "attn":
        out = attention(B["qkv"], B["lens"], dt)
    elif stage == "outproj":
        out = B["x_emb"].astype(dt) + linear(B["att"], W["wo"], W["bo"], dt)
    elif stage == "ln2":
        out = layernorm(B["x_mid"], W["ln2_g"], W["ln2_b"], dt)
    elif stage == "ffn1":
        out = quickgelu(linear(B["h"], W["w1"], W["b1"], dt), dt)
    elif stage == "ffn2":
        out = B["x_mid"].astype(dt) + linear(B["u"], W["w2"], W["b2"], dt)
    elif stage == "next_ln1":
        out = layernorm(B["x_next"], W["ln1n_g"], W["ln1n_b"], dt)
    elif stage == "final":
        out = final(B["x_out"], B["lens"], W["lnf_g"], W["lnf_b"], W["proj"], dt)
    else:
        raise KeyError(stage)
    assert out.dtype == dt, (stage, out.dtype)
    return out


def site_statement(site, S, W, dt, **ln):
    """small-2: the LayerNorm a site applies to the stream S["x"] (`final`: and the projection behind it)."""
    g, b = W[site]
    if site == "final":
        rows = offsets(S["lens"]) + np.asarray(S["lens"]) - 1
        return layernorm(S["x"][rows], g, b, dt, **ln) @ W["proj"].astype(dt)
    return layernorm(S["x"], g, b, dt, **ln)


def layer(x, w, lens, dt, rnd, nxt=None):
    """One whole layer from the stream x: -> (stream after it, every intermediate).  rnd rounds where the kernels store f16 (LayerNorm
    outputs, qkv, attention, QuickGELU); the identity gives the plain tower.  nxt = (gain, bias) of the LayerNorm that follows."""
    t = {"ln1": rnd(layernorm(x, w["ln1_g"], w["ln1_b"], dt))}
    t["qkv"] = rnd(linear(t["ln1"], w["wqkv"], w["bqkv"], dt))
    t["att"] = rnd(attention(t["qkv"], lens, dt))
    t["x_mid"] = np.asarray(x).astype(dt) + linear(t["att"], w["wo"], w["bo"], dt)
    t["h"] = rnd(layernorm(t["x_mid"], w["ln2_g"], w["ln2_b"], dt))
    t["u"] = rnd(quickgelu(linear(t["h"], w["w1"], w["b1"], dt), dt))
    t["x_out"] = t["x_mid"] + linear(t["u"], w["w2"], w["b2"], dt)
    if nxt is not None:
        t["ln1_next"] = rnd(layernorm(t["x_out"], nxt[0], nxt[1], dt))
    return t["x_out"], t


def host_operands(name, W=None):
    """The operand dict of a row set without a GPU: float64 statements, each output stored as its stage stores it."""
    W = W or stage_weights()
    ids, lens = rowset_ids(name)
    B = {"ids": ids, "lens": lens}
    for stage in STAGES:
        if stage == "next_ln1":
            B["x_next"] = B["x_out"]
        out = statement(stage, B, W, np.float64)
        B[OUTPUT[stage]] = f16(out) if F16_OUT[stage] else out.astype(np.float32)
    return B


def host_sites(W=None):
    """small-2's operand dict on row set A without a GPU."""
    W = W or site_weights()
    ids, lens = rowset_ids("A")
    S = {"ids": ids, "lens": lens, "x": embed(ids, lens, W["tok"], W["pos"], np.float32)}
    for site, (key, half) in SITES.items():
        out = site_statement(site, S, W, np.float64)
        S[key] = f16(out) if half else out.astype(np.float32)
    return S


# ---------------------------------------------------------------------------------------------------------------------- the bar
def half_ulp16(ref):
    """Half the spacing of f16 at |ref| (float64): 2^(e - 11) for 2^e <= |ref| < 2^(e + 1), e >= -14; 2^-25 below."""
    _, e = np.frexp(np.maximum(np.abs(ref), 2.0 ** -14))
    return np.ldexp(0.5, e - 11)


def rowmax(ref):
    return np.abs(ref).max(-1, keepdims=True)


def d32_of(rest, ref):
    return float((np.abs(rest.astype(np.float64) - ref) / rowmax(ref)).max())


def ratio(got, ref, d32, half):
    """The worst |got - ref| over the bar."""
    tol = 4.0 * d32 * rowmax(ref) + (half_ulp16(ref) if half else 0.0)
    err = np.abs(np.asarray(got).astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0.0, 0.0, err / tol).max())                   # an exact element passes a bar of zero


def judge(stage, B, W, got=None):
    """-> (worst ratio of the bar, d32) of `got` (default: the operand dict's own buffer) as the output of `stage`."""
    ref = statement(stage, B, W, np.float64)
    d32 = d32_of(statement(stage, B, W, np.float32), ref)
    return ratio(B[OUTPUT[stage]] if got is None else got, ref, d32, F16_OUT[stage]), d32


def judge_site(site, S, W, got=None):
    key, half = SITES[site]
    ref = site_statement(site, S, W, np.float64)
    d32 = d32_of(site_statement(site, S, W, np.float32), ref)
    return ratio(S[key] if got is None else got, ref, d32, half), d32


def stored(stage, out):
    """A statement's output the way the stage stores it."""
    return f16(out) if F16_OUT[stage] else np.asarray(out).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------- mutants
def _column(B, W, c):
    out = statement("qkv", B, W, np.float64)
    out[:, c] -= W["bqkv"][c]
    return out


def _largest_bias(W, part):
    return part * WIDTH + int(np.abs(W["bqkv"][part * WIDTH:(part + 1) * WIDTH]).argmax())


def _swapped(stage, B, W, tile=3, r=5):
    out = statement(stage, B, W, np.float64)
    a, b = 32 * tile + r, 32 * tile + r + 16
    out[[a, b]] = out[[b, a]]
    return out


A_OPERAND = {"qkv": "ln1", "outproj": "att", "ffn1": "h", "ffn2": "u"}


def _last_from_the_row_before(stage, B, W):
    """The GEMM's last live row read from row M - 2 of its activation operand (a clamp one too low)."""
    C = dict(B)
    a = np.array(B[A_OPERAND[stage]])
    a[-1] = a[-2]
    C[A_OPERAND[stage]] = a
    return statement(stage, C, W, np.float64)


def _zero_tile(B, W, t=37):
    out = statement("ffn1", B, W, np.float64)
    out[:, 16 * t:16 * t + 16] = 0.0
    return out


LN_STAGES = {"embed_ln1": ("x_emb", "ln1"), "ln2": ("x_mid", "ln2"), "next_ln1": ("x_next", "ln1n")}
GEMM_STAGES = ("qkv", "outproj", "ffn1", "ffn2")

# name -> (stage, float64 output of the stage with one thing wrong, unrounded), judged on row set A of the real towers
MUTANTS = {
    "gelu constant 1.7": ("ffn1", lambda B, W: quickgelu(linear(B["h"], W["w1"], W["b1"], np.float64), np.float64, c=1.7)),
    "Q bias column dropped": ("qkv", lambda B, W: _column(B, W, _largest_bias(W, 0))),
    "K bias column dropped": ("qkv", lambda B, W: _column(B, W, _largest_bias(W, 1))),
    "V bias column dropped": ("qkv", lambda B, W: _column(B, W, _largest_bias(W, 2))),
    "a 16-column tile of u zero": ("ffn1", _zero_tile),
    "score scale 1/sqrt(65)": ("attn", lambda B, W: attention(B["qkv"], B["lens"], np.float64, scale=65.0 ** -0.5)),
    "key i + 1 visible": ("attn", lambda B, W: attention(B["qkv"], B["lens"], np.float64, see=1)),
    "key 64 dropped": ("attn", lambda B, W: attention(B["qkv"], B["lens"], np.float64, drop=64)),
    "final reads row e - 1": ("final", lambda B, W: final(B["x_out"], B["lens"], W["lnf_g"], W["lnf_b"], W["proj"], np.float64, back=1)),
    "final variance over 511": ("final", lambda B, W: layernorm(B["x_out"][offsets(B["lens"]) + np.asarray(B["lens"]) - 1], W["lnf_g"],
                                                                W["lnf_b"], np.float64, div=511) @ W["proj"]),
}
for _s, (_x, _p) in LN_STAGES.items():
    MUTANTS[f"{_s} variance over 511"] = (_s, lambda B, W, x=_x, p=_p: layernorm(B[x], W[p + "_g"], W[p + "_b"], np.float64, div=511))
for _s in GEMM_STAGES + ("ln2", "next_ln1"):
    MUTANTS[f"{_s} rows r and r + 16 exchanged"] = (_s, lambda B, W, s=_s: _swapped(s, B, W))
for _s in GEMM_STAGES:
    MUTANTS[f"{_s} last row from row M - 2"] = (_s, lambda B, W, s=_s: _last_from_the_row_before(s, B, W))
