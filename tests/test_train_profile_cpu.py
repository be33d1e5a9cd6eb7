"""tests/train_profile.py on the CPU (torch float64, 2 x 33 and 3 x 77 tokens): the rounding model without rounding is plain autograd,
its pooled error sits in the band the GPU measures for the kernels, a coarser rounding reads above the caps, planted local errors are
caught by the profiles, and the scale rule's arithmetic."""
import math

import pytest
import torch

import mst_amd  # noqa: F401
from mst_amd import synthetic as syn
from conftest import SEED

import train_profile as trp
from train_profile import C_GROW_CAP, C_POOL_CAP, C_TOK_CAP, C_VEC_CAP, D, FF, H, L

TOL_GRAD = 1.5e-3                # tests/test_gpu_train.py
FE = 263
_CACHE = {}


def params64():
    if "w" not in _CACHE:
        w = syn.denoiser_state(SEED, FE, layer_prefix="seqTransEncoder.layers.")
        _CACHE["w"] = [torch.from_numpy(w[f"seqTransEncoder.layers.{l}.{k}"]).double() for l in range(L) for k in trp.TENSORS]
    return [q.clone().requires_grad_(True) for q in _CACHE["w"]]


def inputs(rows, S, p=0.1):
    h = torch.from_numpy(syn.normal(SEED, f"cpuprofile/h/{rows}/{S}", (rows, S, D))).double()
    r = torch.from_numpy(syn.normal(SEED, f"cpuprofile/r/{rows}/{S}", (rows, S, D))).double()
    gen = torch.Generator().manual_seed(rows * 1000 + S)
    keepm = lambda *shape: (torch.rand(*shape, generator=gen) >= p).double() / (1 - p)
    masks = [(keepm(rows, H, S, S), keepm(rows, S, D), keepm(rows, S, FF), keepm(rows, S, D)) for _ in range(L)]
    return h, r, masks


def run(rows, S, dt, r=None, fn=trp.stack, **kw):
    """(out, dL/dh, the 96 gradients) of sum(out * r) through fn on the CPU inputs of (rows, S)."""
    h, r0, masks = inputs(rows, S)
    r = r0 if r is None else r
    leaves = [h.clone().requires_grad_(True)] + params64()
    out = fn(leaves[0], leaves[1:], masks, None, **kw) if dt == "plain" else fn(leaves[0], leaves[1:], masks, None, dt=dt, **kw)
    g = trp.model_backward(out, leaves, r, dt=None if dt == "plain" else dt)
    return out.detach(), g[0], list(g[1:])


def cached(rows, S, dt):
    key = (rows, S, str(dt))
    if key not in _CACHE:
        _CACHE[key] = run(rows, S, dt)
    return _CACHE[key]


def test_the_model_without_rounding_is_plain_autograd():
    from test_gpu_train import torch_stack
    for rows, S in ((2, 33), (3, 77)):
        out, d_in, grads = cached(rows, S, None)
        p_out, p_din, p_grads = run(rows, S, "plain", fn=torch_stack)
        assert trp.rel(out, p_out) < 1e-12 and trp.rel(d_in, p_din) < 1e-12
        worst = max(trp.rel(a, b) for a, b in zip(grads, p_grads))
        assert worst < 1e-12, worst
    # ... and with a key-padding mask
    h, r, _ = inputs(2, 33)
    keep = torch.ones(2, 33, dtype=torch.bool)
    keep[1, 20:] = False
    a, b = [h.clone().requires_grad_(True)] + params64(), [h.clone().requires_grad_(True)] + params64()
    ga = torch.autograd.grad(trp.stack(a[0], a[1:], None, keep), a, grad_outputs=r * keep[:, :, None])
    gb = torch.autograd.grad(torch_stack(b[0], b[1:], None, keep), b, grad_outputs=r * keep[:, :, None])
    assert max(trp.rel(x, y) for x, y in zip(ga, gb)) < 1e-12
    assert float(ga[0][~keep].abs().max()) == 0.0


# measured on the CPU (pooled relative L2 of the f16 model against float64) at 2 x 33 / 3 x 77: forward 3.08e-4 / 2.87e-4, dL/dh
# 3.63e-4 / 3.26e-4, the worst of the 96 gradients 6.71e-4 / 6.64e-4 (L0.self_attn.in_proj_weight, the kernels' worst tensor too); the
# kernels measure 2.8e-4 .. 3.6e-4, 3.0e-4 .. 4.0e-4 and 6.4e-4 .. 7.4e-4 on the GPU (tests/test_gpu_train_shapes.py)
BAND = (2e-4, 1e-3)


def test_the_model_sits_where_the_kernels_measure():
    for rows, S in ((2, 33), (3, 77)):
        ref, model = cached(rows, S, None), cached(rows, S, torch.float16)
        e_out, e_din = trp.rel(model[0], ref[0]), trp.rel(model[1], ref[1])
        errs = {trp.name_of(i): trp.rel(a, b) for i, (a, b) in enumerate(zip(model[2], ref[2]))}
        lo, hi = min(errs, key=errs.get), max(errs, key=errs.get)
        print(f"f16 model at {rows} x {S}: out {e_out:.2e}, d_in {e_din:.2e}, gradients {errs[lo]:.2e} ({lo}) .. {errs[hi]:.2e} ({hi})")
        assert BAND[0] < e_out < BAND[1] and BAND[0] < e_din < BAND[1], (e_out, e_din)
        # every tensor behind at least one contraction rounds; the last layer's norm2 vectors have none behind them
        assert errs[hi] < BAND[1], (hi, errs[hi])
        assert all(e > 1e-5 for n, e in errs.items() if not n.startswith("L7.norm2")), (lo, errs[lo])
        assert errs["L7.norm2.bias"] < 1e-12


def test_a_coarser_rounding_reads_above_the_caps():
    """bfloat16 operands (eight times f16's rounding error) as the "kernel" against the f16 model: above every cap."""
    rows, S = 3, 77
    ref, model, coarse = cached(rows, S, None), cached(rows, S, torch.float16), cached(rows, S, torch.bfloat16)
    tok_out = float(trp.token_ratios(coarse[0], ref[0], model[0]).max())
    tok_din = float(trp.token_ratios(coarse[1], ref[1], model[1]).max())
    worst = {"row": 0.0, "col": 0.0, "block": 0.0}
    for i in range(96):
        if trp.name_of(i).startswith("L7.norm2"):
            continue
        for kind in (("row", "col") if ref[2][i].ndim == 2 else ("block",)):
            worst[kind] = max(worst[kind], float(trp.vector_ratios(kind, coarse[2][i], ref[2][i], model[2][i]).max()))
    print(f"bf16 operands against the f16 model: tokens {tok_out:.1f} / {tok_din:.1f}, {worst}")
    assert tok_out > C_TOK_CAP and tok_din > C_TOK_CAP
    assert worst["row"] > C_GROW_CAP and worst["col"] > C_GROW_CAP and worst["block"] > C_VEC_CAP
    with pytest.raises(AssertionError, match=r"clip \d, token \d+ \(% 32 = \d+\): token row \d+ \(% 64 = \d+, % 32 = \d+\)"):
        trp.assert_tokens(coarse[1], ref[1], model[1], C_TOK_CAP, what="bf16")
    # the model itself passes at ratio <= 1 everywhere: no zero median, no empty row
    assert 0 < trp.assert_tokens(model[1], ref[1], model[1], 1.0) <= 1
    for i in range(96):
        assert all(0 <= v <= 1 for v in trp.assert_gradient(i, model[2][i], ref[2][i], model[2][i], 1.0, 1.0).values())


def second(rows, S):
    """A second realisation of f16 rounding to plant errors into: the model with every operand nudged by 1 + 2^-13 before it is rounded."""
    key = (rows, S, "second")
    if key not in _CACHE:
        orig = trp._rnd
        trp._rnd = lambda x, dt: orig(x * (1 + 2.0 ** -13), dt) if dt is not None else x
        try:
            _CACHE[key] = run(rows, S, torch.float16)
        finally:
            trp._rnd = orig
    return _CACHE[key]


def test_planted_local_errors_are_caught_by_the_profiles():
    """Each mutant with its pooled figure beside the profile's.  What the pooled bar (1.5e-3) makes of each depends on the share of the
    tensor it touches: at M = 231 one token is 1 / 231 of dL/dh and a 5 % error reads 0.05 / sqrt(231) = 3.3e-3 pooled -- the pooled bar
    sees it at this size and no longer at the suite's large cases (7289 tokens: 5.9e-4 in quadrature), which the synthetic tensor of that
    size shows; the profile's reading does not depend on the size."""
    rows, S = 3, 77
    ref, model, other = cached(rows, S, None), cached(rows, S, torch.float16), second(rows, S)
    assert float(trp.token_ratios(other[1], ref[1], model[1]).max()) < C_TOK_CAP            # the second realisation itself passes
    # (1) one token of dL/dh x 1.05 at M = 231
    d = other[1].clone()
    d[2, 50] *= 1.05                                   # token row 204: % 64 = 12
    ratio = float(trp.token_ratios(d, ref[1], model[1]).max())
    print(f"one token of dL/dh x 1.05 at M = 231: pooled {trp.rel(d, ref[1]):.2e}, token ratio {ratio:.0f}")
    assert ratio > 10 * C_TOK_CAP
    with pytest.raises(AssertionError, match=r"clip 2, token 50 \(% 32 = 18\): token row 204 \(% 64 = 12, % 32 = 12\)"):
        trp.assert_tokens(d, ref[1], model[1], C_TOK_CAP, what="one token")
    # ... and at 37 x 197 = 7289 tokens, where the pooled bar lets it pass
    gen = torch.Generator().manual_seed(7)
    big = torch.randn(37, 197, D, generator=gen, dtype=torch.float64)
    noise = lambda: big + 5e-4 * torch.randn(big.shape, generator=gen, dtype=torch.float64)
    big_model, big_kernel = noise(), noise()
    big_kernel[36, 190] = big[36, 190] * 1.05
    assert trp.rel(big_kernel, big) < 8e-4 < TOL_GRAD
    assert float(trp.token_ratios(big_kernel, big, big_model).max()) > 10 * C_TOK_CAP
    # (2) one row of L3.linear1.weight's gradient x 1.05: 1 / 1024 of the tensor
    i = 3 * 12 + 4
    g = other[2][i].clone()
    g[517] *= 1.05
    pooled, clean = trp.rel(g, ref[2][i]), trp.rel(other[2][i], ref[2][i])
    rr = trp.vector_ratios("row", g, ref[2][i], model[2][i])
    print(f"row 517 of {trp.name_of(i)} x 1.05: pooled {clean:.2e} -> {pooled:.2e}, row ratio {float(rr[517]):.0f}")
    assert int(rr.argmax()) == 517 and float(rr[517]) > 5 * C_GROW_CAP
    assert pooled < 2 * 0.05 / math.sqrt(1024) + clean                      # the row's share: about 1.6e-3, at the pooled bar
    with pytest.raises(AssertionError, match=r"L3.linear1.weight row 517"):
        trp.assert_gradient(i, g, ref[2][i], model[2][i], C_GROW_CAP, C_VEC_CAP)
    # (3) one 64-block of L0.norm1.bias's gradient x 1.1: 1 / 8 of the tensor, which the pooled figure sees as well
    i = 9
    g = other[2][i].clone()
    g[128:192] *= 1.1
    br = trp.vector_ratios("block", g, ref[2][i], model[2][i])
    print(f"block 2 of {trp.name_of(i)} x 1.1: pooled {trp.rel(g, ref[2][i]):.2e}, block ratio {float(br[2]):.0f}")
    assert int(br.argmax()) == 2 and float(br[2]) > 5 * C_VEC_CAP
    with pytest.raises(AssertionError, match=r"L0.norm1.bias block 2 \(elements 128 .. 191\)"):
        trp.assert_gradient(i, g, ref[2][i], model[2][i], C_GROW_CAP, C_VEC_CAP)


def test_a_dropped_token_shows_undiluted_under_a_localized_cotangent():
    """The last layer's W2 gradient without the last token's contribution: under the dense cotangent the loss is one token's share of a sum
    over 231 (and 1 / sqrt(7289) = 1.2e-2 at the suite's largest case); under the "last token of the launch" cotangent it is the whole
    gradient."""
    rows, S = 3, 77
    h, r, masks = inputs(rows, S)
    i = 7 * 12 + 6
    r_last = torch.zeros_like(r)
    r_last[-1, -1] = r[-1, -1]
    r_without = r.clone()
    r_without[-1, -1] = 0                               # the dense gradient of L7.linear2.weight without that token: it enters only through r
    dense, local = cached(rows, S, None), run(rows, S, None, r=r_last)
    dropped = run(rows, S, None, r=r_without)[2][i]
    e_dense = trp.rel(dropped, dense[2][i])
    e_local = trp.rel(torch.zeros_like(local[2][i]), local[2][i])
    model_local = run(rows, S, torch.float16, r=r_last)
    m_local = trp.rel(model_local[2][i], local[2][i])
    print(f"{trp.name_of(i)} without the last token: dense {e_dense:.2e}, localized {e_local:.2e} against a model error of {m_local:.2e}")
    assert e_local == 1.0 and e_local > 10 * e_dense
    assert e_local > 100 * C_POOL_CAP * max(m_local, trp.FLOOR)
    assert 1e-5 < m_local < 1e-3                       # the pooled model error is a usable bar for a one-token sum


def test_localized_sets_leave_the_reference_a_gradient_everywhere():
    """The share of (set, tensor) pairs whose float64 gradient is below 1e-12 of the dense one -- skipped on the GPU -- at 3 x 77."""
    from test_gpu_train_profile import MAX_SKIPPED_SHARE, NEGLIGIBLE, local_cotangent, token_sets
    rows, S = 3, 77
    _, r, _ = inputs(rows, S)
    dense = cached(rows, S, None)
    norms = [float(dense[1].norm())] + [float(x.norm()) for x in dense[2]]
    sets = token_sets(rows, S)
    assert sets["last-token"] == [(2, 76)] and sets["tile-edges"] == [(1, 50), (1, 51)] and sets["split-edges"] == [(0, 0), (2, 76)]
    skipped = 0
    for name, tokens in sets.items():
        _, d_in, grads = run(rows, S, None, r=local_cotangent(r, tokens))
        small = [n for n, x, dn in zip(["d_in"] + [trp.name_of(i) for i in range(96)], [d_in] + grads, norms) if float(x.norm()) < NEGLIGIBLE * dn]
        print(f"{name} {tokens}: {len(small)} of 97 tensors without a gradient {small}")
        skipped += len(small)
    assert skipped <= MAX_SKIPPED_SHARE * 97 * len(sets)


def test_the_scale_rule():
    for amax, want in ((1.0, 32.0), (16.0, 2.0), (17.0, 1.0), (31.9, 1.0), (32.0, 1.0), (33.0, 0.5), (2.0 ** -30, 2.0 ** 35), (3e-9, 2.0 ** 33)):
        s = trp.grad_scale(amax)
        assert s == want and math.log2(s) == round(math.log2(s)) and 16.0 < amax * s <= 32.0, (amax, s)
    assert trp.grad_scale(0.0) == 1.0 and trp.grad_scale(float("inf")) == 1.0 and trp.grad_scale(float("nan")) == 1.0
    # f16 after the scale: normal down to 2^-14, so an entry 2^-18 .. 2^-19 below the launch's largest is the first subnormal one, and
    # 2^-10 of that rounds to zero
    for amax in (1.0, 17.0, 31.9, 3e-9):
        sub, zero = trp.subnormal_below(amax)
        assert 2.0 ** -19 <= sub / amax < 2.0 ** -18 and zero == sub * 2.0 ** -11
        x = torch.tensor([sub, sub * (1 - 2.0 ** -12), zero * 1.01, zero * 0.99], dtype=torch.float64) * trp.grad_scale(amax)
        y = x.to(torch.float16).double()
        assert y[0] == x[0] and y[1] != x[1] and y[2] == 2.0 ** -24 and y[3] == 0.0
    # the model applies it: a cotangent scaled by 2^-30 gives the same relative error, bit for bit after unscaling
    a = run(2, 33, torch.float16)
    _, r, _ = inputs(2, 33)
    b = run(2, 33, torch.float16, r=r * 2.0 ** -30)
    assert torch.equal(b[1] * 2.0 ** 30, a[1])
