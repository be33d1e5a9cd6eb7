"""Local error profiles of the TRAINING path against a float64 reference, and the yardstick they are held to.

A pooled relative L2 per tensor cannot see one token of dL/dh, one row of a weight gradient or one block of a bias gradient: at
M = 7289 tokens one token of dL/dh wrong by 10 % adds 1.2e-3 in quadrature, one row of a 1536 x 512 gradient wrong by 5 % adds 1.3e-3.
Here the same differences are resolved per (clip, token), per clip, per output row and input column of a 2-D gradient and per
64-element block of a 1-D one, and each is held to a ROUNDING MODEL of the backward on the test's own inputs:

    kernel_err <= c * max(model_err, median model_err)                  c_tok (tokens), c_grow (rows, columns), c_vec (blocks)

The model (`stack` with dt=torch.float16) is the eight post-norm layers of tests/test_gpu_train.py's torch_stack with every
contraction -- the four GEMMs, Q K^T and P V -- behind one autograd function: the forward rounds both operands to dt and multiplies in
the carrier precision (float64); the backward rounds the incoming gradient and the saved operands the same way before the dgrad and
wgrad products (a bias gradient is the column sum of the rounded gradient, as the kernels' f16 column sums have it).  `model_backward`
multiplies the cotangent by the engine's own power of two (max |r| into [16, 32], `grad_scale`) and unscales the results, so the model
meets f16's subnormal range where the kernels meet it.  Softmax, LayerNorm, GELU and the masks stay in the carrier precision.  It is
what oracle/denoiser.py's `dt` is for the sampling path, extended to the backward: a yardstick, not a copy of the kernels' choices
(hi / lo tape slots, fp32 d hid in the fused tail, ...).

Everything here is float64 torch on the device of its inputs.

Measured on an MI355X over ALL cases of tests/test_gpu_train_profile.py (its docstring has the table); each factor is 1.5 x the worst
kernel / model ratio -- the half covers other seeds and weights -- and under its cap, which is a condition and no measurement: above
3 (tokens, pooled one-token sums, clips) and 6 (gradient rows and columns, vector blocks) a bar no longer separates a local error of a
few per cent from rounding."""
import math

import torch
import torch.nn.functional as F

L, D, H, FF = 8, 512, 4, 1024
TENSORS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
           "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")
WEIGHTS = (0, 2, 4, 6)                 # indices of the four 2-D tensors of a layer
# a layer's wgrad (tests/test_gpu_train_shapes.py: WGRADS) behind each 2-D tensor
WGRAD_OF = {0: "Win", 2: "Wout", 4: "W1", 6: "W2"}
VEC_BLOCK = 64

C_TOK_CAP, C_GROW_CAP, C_VEC_CAP, C_POOL_CAP, C_CLIP_CAP = 3.0, 6.0, 6.0, 3.0, 3.0
# measured worst ratios:
#   tokens  1.54  dL/dh under the token-0-of-every-clip cotangent at 37 x 197 (dense: 1.30, `out` at 37 x 197)
#   rows    3.71  L5.self_attn.in_proj_weight row 1092 (a V row) at 3 x 198 key-padded, large tiles; columns 2.14 (L7 out_proj, same case)
#   blocks  1.52  L1.norm1.weight block 7 at 37 x 197
#   pooled  1.27  L6.norm2.weight under the last-token cotangent at 37 x 197
#   clips   1.12  the 2^-16 clips beside eight 2^0 tokens at 4 x 77 (1.11 over the exponents 0 .. 24)
MEASURED_TOK, MEASURED_GROW, MEASURED_VEC, MEASURED_POOL, MEASURED_CLIP = 1.54, 3.71, 1.52, 1.27, 1.12
C_TOK, C_GROW, C_VEC = 1.5 * MEASURED_TOK, 1.5 * MEASURED_GROW, 1.5 * MEASURED_VEC
C_POOL, C_CLIP = 1.5 * MEASURED_POOL, 1.5 * MEASURED_CLIP
assert C_TOK <= C_TOK_CAP and C_GROW <= C_GROW_CAP and C_VEC <= C_VEC_CAP and C_POOL <= C_POOL_CAP and C_CLIP <= C_CLIP_CAP


def name_of(i):
    return f"L{i // 12}.{TENSORS[i % 12]}"


# ------------------------------------------------------------------------------ the rounding model
def _rnd(x, dt):
    return x if dt is None else x.to(dt).to(x.dtype)


class RoundedMatmul(torch.autograd.Function):
    """a @ b over equal batch dimensions with both operands rounded to dt; the backward rounds the incoming gradient and the saved
    operands before both products."""
    @staticmethod
    def forward(ctx, a, b, dt):
        ctx.save_for_backward(a, b)
        ctx.dt = dt
        return _rnd(a, dt) @ _rnd(b, dt)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = _rnd(g, ctx.dt)
        return g @ _rnd(b, ctx.dt).transpose(-1, -2), _rnd(a, ctx.dt).transpose(-1, -2) @ g, None


class RoundedLinear(torch.autograd.Function):
    """x [M, K] @ w [N, K]^T + b: the dgrad, the wgrad and the bias gradient (a column sum) all read the rounded gradient."""
    @staticmethod
    def forward(ctx, x, w, b, dt):
        ctx.save_for_backward(x, w)
        ctx.dt = dt
        return _rnd(x, dt) @ _rnd(w, dt).t() + b

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = _rnd(g, ctx.dt)
        return g @ _rnd(w, ctx.dt), g.t() @ _rnd(x, ctx.dt), g.sum(0), None


def stack(h, params, masks=None, keep=None, dt=None):
    """torch_stack of tests/test_gpu_train.py (same arguments, same arithmetic) with every contraction behind RoundedMatmul /
    RoundedLinear: dt=None is plain autograd up to the order of the sums."""
    B, S, _ = h.shape
    x = h
    bias = None
    if keep is not None:
        bias = torch.zeros(keep.shape, dtype=h.dtype, device=h.device).masked_fill(~keep.bool(), float("-inf"))[:, None, None, :]
    lin = lambda v, w, b: RoundedLinear.apply(v.reshape(B * S, -1), w, b, dt).view(B, S, -1)
    for l in range(L):
        win, bin_, wout, bout, w1, b1, w2, b2, g1, be1, g2, be2 = params[12 * l:12 * l + 12]
        m = masks[l] if masks is not None else (None,) * 4
        qkv = lin(x, win, bin_)
        q, k, v = qkv.view(B, S, 3, H, D // H).permute(2, 0, 3, 1, 4)          # [B, H, S, hd]
        s = RoundedMatmul.apply(q * (D // H) ** -0.5, k.transpose(-1, -2), dt)
        if bias is not None:
            s = s + bias
        p = torch.softmax(s, dim=-1)
        if m[0] is not None:
            p = p * m[0]
        att = RoundedMatmul.apply(p, v, dt).permute(0, 2, 1, 3).reshape(B, S, D)
        o = lin(att, wout, bout)
        if m[1] is not None:
            o = o * m[1]
        x1 = F.layer_norm(x + o, (D,), g1, be1, 1e-5)
        hid = F.gelu(lin(x1, w1, b1))
        if m[2] is not None:
            hid = hid * m[2]
        f = lin(hid, w2, b2)
        if m[3] is not None:
            f = f * m[3]
        x = F.layer_norm(x1 + f, (D,), g2, be2, 1e-5)
    return x


F16_MIN_NORMAL, F16_MIN_SUBNORMAL = 2.0 ** -14, 2.0 ** -24


def grad_scale(amax):
    """k_grad_scale's rule (csrc/mst_train.h): the power of two s = 2^floor(log2(32 / max |g|)), which brings max |g| into (16, 32];
    1 for a zero, infinite or NaN maximum."""
    amax = float(amax)
    if not (0.0 < amax < math.inf):
        return 1.0
    s = 2.0 ** math.floor(math.log2(32.0 / amax))
    return s if 0.0 < s < math.inf else 1.0


def subnormal_below(amax):
    """(below this magnitude a value of the launch is an f16 subnormal, below this it is zero) after the scale of a launch whose largest
    cotangent entry is amax: between 2^-18 and 2^-19 of amax, and 2^-10 of that."""
    s = grad_scale(amax)
    return F16_MIN_NORMAL / s, 0.5 * F16_MIN_SUBNORMAL / s


def model_backward(out, leaves, r, dt=torch.float16):
    """Gradients of sum(out * r) with respect to `leaves` through a graph built by stack(dt=...): the cotangent scaled by the engine's
    power of two first, every result unscaled, so that the model's rounded gradients live where the kernels' f16 operands live."""
    s = grad_scale(r.abs().max()) if dt is not None else 1.0
    g = torch.autograd.grad(out, leaves, grad_outputs=r.to(out.dtype) * s, retain_graph=True, allow_unused=True)
    return [None if x is None else x / s for x in g]


# ------------------------------------------------------------------------------ the profiles
def _d(a):
    return a.detach().double()


def rel(a, b):
    a, b = _d(a), _d(b)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def token_errors(out, ref):
    """[B, S]: L2 norm of out - ref at one (clip, token) over the clip's RMS token norm of ref."""
    o, r = _d(out), _d(ref)
    assert o.ndim == 3 and o.shape == r.shape, (o.shape, r.shape)
    rms = (r ** 2).sum(2).mean(1, keepdim=True).sqrt()
    return ((o - r) ** 2).sum(2).sqrt() / rms.clamp_min(1e-300)


def clip_errors(out, ref):
    """[B]: relative L2 per clip."""
    o, r = _d(out), _d(ref)
    return ((o - r) ** 2).sum((1, 2)).sqrt() / (r ** 2).sum((1, 2)).sqrt().clamp_min(1e-300)


def row_errors(g, ref):
    """[rows]: relative L2 of each output row of a 2-D gradient over that row's own norm in ref."""
    g, r = _d(g), _d(ref)
    assert g.ndim == 2 and g.shape == r.shape
    return ((g - r) ** 2).sum(1).sqrt() / (r ** 2).sum(1).sqrt().clamp_min(1e-300)


def col_errors(g, ref):
    """[columns]: the same per input column."""
    return row_errors(_d(g).t(), _d(ref).t())


def block_errors(g, ref):
    """[n / 64]: RMS of g - ref over one 64-element block over the RMS of the whole of ref (1-D gradients)."""
    g, r = _d(g), _d(ref)
    assert g.ndim == 1 and g.numel() % VEC_BLOCK == 0
    return ((g - r) ** 2).view(-1, VEC_BLOCK).mean(1).sqrt() / (r ** 2).mean().sqrt().clamp_min(1e-300)


# Where no contraction lies between the cotangent and a result (the last layer's norm2 gradients: sums of g and of g xhat) the float64
# model has no error at all, while the kernels sum in fp32 and read LayerNorm's input as an f16 hi + lo pair (2^-22 relative) through
# 512-term fp32 reductions (sqrt(512) x 2^-24 = 1.3e-6).  No bar lies below 2^-19 = 1.9e-6, 32 fp32 ulps.
FLOOR = 2.0 ** -19


def _over_bar(k, m, median):
    return k / torch.maximum(torch.maximum(m, median), torch.full_like(m, FLOOR))


def token_ratios(out, ref, model, valid=None):
    """[B, S]: kernel token error over its bar at c_tok = 1; the floor is the median model error of the clip's tokens (of its
    `valid` ones: padded positions are scored nowhere and take no part in the median; their ratio is 0)."""
    k, m = token_errors(out, ref), token_errors(model, ref)
    if valid is None:
        return _over_bar(k, m, m.median(1, keepdim=True).values)
    v = valid.bool()
    med = torch.nanmedian(torch.where(v, m, torch.full_like(m, float("nan"))), 1, keepdim=True).values
    return torch.where(v, _over_bar(k, m, med), torch.zeros_like(k))


def vector_ratios(kind, g, ref, model):
    """kind: "row" | "col" (2-D gradients) | "block" (1-D): kernel error over its bar at c = 1, floor = the median over the profile."""
    fn = {"row": row_errors, "col": col_errors, "block": block_errors}[kind]
    k, m = fn(g, ref), fn(model, ref)
    return _over_bar(k, m, m.median())


def where_token(b, t, S):
    """Where (clip b, token t) sits in the training kernels' tiles: token rows b S + t are walked in 64-token tiles (GEMMs, the fused
    tails) and 32-token wgrad slabs; attention walks a clip's keys in 32-key tiles."""
    row = b * S + t
    return f"clip {b}, token {t} (% 32 = {t % 32}): token row {row} (% 64 = {row % 64}, % 32 = {row % 32})"


def wgrad_split_of(row, M, plan):
    """plan = (grid, nsplit, tokens in the last split) of tests/test_gpu_train_shapes.py's wgrad_plan: the split that holds a token row."""
    _, nsplit, last = plan
    if nsplit == 1:
        return 0
    kchunk = (M - last) // (nsplit - 1)
    return row // kchunk


def assert_tokens(out, ref, model, c_tok, valid=None, what=""):
    """Every token within c_tok of the model's own token profile.  Returns the worst ratio."""
    ratio = token_ratios(out, ref, model, valid)
    S = ratio.shape[1]
    i = int(ratio.argmax())
    b, t = divmod(i, S)
    worst = float(ratio[b, t])
    assert worst <= c_tok, (f"{what}: token error {float(token_errors(out, ref)[b, t]):.3e} is {worst:.2f} x the model's bar "
                            f"(c_tok = {c_tok:.2f}) at {where_token(b, t, S)}")
    return worst


def assert_clips(out, ref, bar, what=""):
    e = clip_errors(out, ref)
    b = int(e.argmax())
    assert float(e[b]) <= bar, f"{what}: clip {b} reads {float(e[b]):.3e} against {bar:.1e}"
    return float(e[b])


def assert_gradient(i, g, ref, model, c_grow, c_vec, plans=None, M=None, what=""):
    """Tensor i (0 .. 95) of the 96: rows and columns of a 2-D gradient, 64-element blocks of a 1-D one.  Returns {kind: worst ratio}.
    plans / M (wgrad_plan(M)): the message says how many splits the tensor's wgrad ran in."""
    worst = {}
    kinds = ("row", "col") if g.ndim == 2 else ("block",)
    for kind in kinds:
        ratio = vector_ratios(kind, g, ref, model)
        j = int(ratio.argmax())
        c = c_grow if g.ndim == 2 else c_vec
        plan = ""
        if plans is not None and i % 12 in WGRAD_OF:
            grid, nsplit, last = plans[WGRAD_OF[i % 12]]
            plan = f", wgrad {WGRAD_OF[i % 12]} in {nsplit} split(s) ({grid}), last of {last} tokens"
        at = f"{kind} {j}" if kind != "block" else f"block {j} (elements {j * VEC_BLOCK} .. {j * VEC_BLOCK + VEC_BLOCK - 1})"
        assert float(ratio[j]) <= c, (f"{what}: {name_of(i)} {at}: {float(ratio[j]):.2f} x the model's bar "
                                      f"(c = {c:.2f}; {kind} % 16 = {j % 16}, % 128 = {j % 128}{plan})")
        worst[kind] = float(ratio[j])
    return worst
