"""The training path per token, per clip, per gradient row / column / block, under localized cotangents and over the cotangent's
dynamic range -- through eng.train_forward / eng.train_backward against float64 autograd on the GPU, held to the rounding model of
tests/train_profile.py (`kernel_err <= c * max(model_err, median model_err, 2^-19)`).

tests/test_gpu_train*.py judge `out`, dL/dh and each of the 96 gradient tensors by one relative L2 each (bars 1e-3 / 1.5e-3, measured
worst about 7e-4) under a dense unit-variance cotangent.  Inside that slack fit one token of dL/dh wrong by 10 % at M = 7289, one row of
a 1536 x 512 gradient wrong by 5 %, a token dropped at a split boundary, and any loss of small gradients beside large ones in one launch.

A. dense cotangent, resolved (test_dense_cotangent_resolved): the pooled bars unchanged, then every token and clip of `out` and dL/dh,
   every row and column of the four weight gradients and every 64-element block of the eight vectors of every layer.
B. localized cotangents (test_localized_cotangent): r is nonzero on a chosen token set only -- the last token of the launch, both sides
   of every 64-token tile boundary inside one clip, the first and last token of the last wgrad split of each plan, token 0 of every clip,
   the last real key of each padded clip.  Every tensor pooled against the model's own pooled error (a one-token sum averages nothing),
   the token profile of dL/dh on the clips that hold the tokens, exact zeros on every other clip and on padded keys.
C. dynamic range (test_cotangent_dynamic_range, test_cotangent_range_inside_one_clip): r[b] = 2^-k_b n[b].  ONE power of two per launch
   (k_grad_scale: max |r| into [16, 32)) scales every f16 operand of the backward, so a clip 2^-k below the launch's largest meets f16's
   subnormals from k = 18 on.  Per clip: the kernel against the model wherever the model is below 1e-2; TOL_GRAD against float64 for every
   k <= R_SUPPORTED; the gradients of the mixed launch equal the sum of per-exponent launches within 2e-5.

MEASURED on an MI355X, 29 cases, 7.2 s in all (tests/test_gpu_train_shapes.py: 8 s).  Worst kernel / model ratio per group; the factors of
tests/train_profile.py are 1.5 x the worst of each column: c_tok 2.31 (cap 3), c_grow 5.57 (cap 6), c_vec 2.28 (cap 6), c_pool 1.91
(cap 3), c_clip 1.68 (cap 3).

    A. dense                     tokens out | dL/dh   rows | columns                      blocks   pooled out | dL/dh | worst gradient
       3 x 77 small              1.23 | 1.20          2.82 (L7 in_proj row 1279) | 1.82   1.43     3.3e-4 | 3.6e-4 | 7.3e-4
       3 x 198 key-padded small  1.27 | 1.25          3.58 (L7 in_proj row 1335) | 1.84   1.43     3.1e-4 | 3.4e-4 | 7.1e-4
       3 x 198 key-padded large  1.29 | 1.26          3.71 (L5 in_proj row 1092) | 2.14   1.36     3.1e-4 | 3.4e-4 | 6.9e-4
       27 x 77                   1.27 | 1.24          1.93 | 1.35                         1.37     3.3e-4 | 3.6e-4 | 6.9e-4
       21 x 197, p 0             1.28 | 1.26          3.08 (L4 in_proj row 1362) | 1.33   1.39     2.8e-4 | 3.0e-4 | 6.6e-4
       37 x 197                  1.30 | 1.29          3.17 (L3 in_proj row 1272) | 1.31   1.52     3.1e-4 | 3.4e-4 | 6.9e-4
       21 x 197 frozen           1.28 | 1.17                                                       2.8e-4 | 2.8e-4
       3 x 198 key-padded frozen 1.29 | 1.14                                                       3.1e-4 | 3.2e-4
       27 x 77, fused tail = 2   1.27 | 1.16          2.14 (L4 out_proj row 380) | 1.34   1.31     3.3e-4 | 3.3e-4 | 6.7e-4
    B. localized (pooled per tensor | tokens of the clips that hold the set)
       3 x 77 small              last token 1.21 | 1.20, tile edges 1.21 | 1.13, split edges 1.20 | 1.25, token 0 of every clip 1.21 | 1.26
       27 x 77                   1.18 | 1.14, 1.19 | 1.13, 1.15 | 1.15, 1.16 | 1.28
       37 x 197                  1.27 | 1.15, 1.19 | 1.15, 1.21 | 1.29, 1.20 | 1.54
       3 x 198 last real keys    small 1.19 | 1.33, large 1.22 | 1.22;  no (set, tensor) pair of the 14 x 97 is skipped
    C. per-clip dL/dh error by exponent, kernel | model (27 x 77 trainable; 4 x 77 and the frozen passes within 3 % of it):
       2^0 3.61e-4 | 3.29e-4, 2^-6 3.59e-4 | 3.29e-4, 2^-12 3.66e-4 | 3.33e-4, 2^-16 1.37e-3 | 1.30e-3, 2^-20 2.15e-2 | 2.04e-2,
       2^-24 2.57e-1 | 2.42e-1: worst ratio 1.11, R = 16 on all four cases; every gradient of the mixed launch <= 6.7e-4 of float64 and
       within 7.5e-6 of the sum of its per-exponent launches; eight 2^0 tokens inside a 2^-16 clip: 1.12 (4 x 77), 1.05 (27 x 77).

The worst rows are V rows of in_proj_weight (rows 1024 .. 1535) on every path and at every plan, one split included: about three times
the model's median row, a property of the attention backward's dV and no tile edge.  The kernels follow f16's GRADUAL underflow: the
matrix pipe of gfx950 does not flush subnormal f16 operands (at 2^-20, where every operand of those clips is subnormal, a flush would
read 1.0, not 2e-2).  Before k_attention_bwd rounded dS without the softmax scale, part C read 4.79e-4, 5.22e-3, 7.15e-2 at 2^-12,
2^-16, 2^-20: four times the model (R = 12); the model with dS rounded behind the scale reproduces those figures on the CPU.
"""
import pytest
import torch

import mst_amd  # noqa: F401
from mst_amd import synthetic as syn

import train_profile as trp
from test_gpu_train import TOL_FWD, TOL_GRAD, engine_masks, layer_params, torch_stack
from test_gpu_train_shapes import FE, MAX_FRAMES, MAX_ROWS, _dev, check, engine, label, pad_keep, plan_str, stream, weights, wgrad_plan
from train_profile import C_CLIP, C_GROW, C_POOL, C_TOK, C_VEC

pytestmark = pytest.mark.gpu

# The supported cotangent range: a clip (or token) whose cotangent lies 2^-R_SUPPORTED below the launch's largest still meets TOL_GRAD
# on its dL/dh.  Measured over EXPONENTS on both tile paths, trainable and frozen: 16 on all four (1.30e-3 .. 1.37e-3 at 2^-16, the edge;
# 2.1e-2 at 2^-20).  OBJECTIVE_RATIO is the largest ratio of per-clip max |g| that the fine-tune objective produces in one backward pass
# (tools/train_grad_range.py on the three fine-tune gradient cases of tests/test_gpu_boundary.py, torch-ops path, a hook on every stack's
# output gradient): 7.9 / 6.6 / 10.4 over ALL clips that enter the trainable stack during the pass (six chained steps and the
# text-to-motion batch, which the native path differentiates in two launches with a scale each: the native calls see 1.12 / 1.11 /
# 1.08 inside one launch), 1.05 / 1.05 / 1.06 at the motion encoder.  Required: 2^R >= 16 x that ratio; 2^16 is 394 x.
EXPONENTS = (0, 6, 12, 16, 20, 24)
R_SUPPORTED = 16
OBJECTIVE_RATIO = 10.4

_CACHE = {}


def fused_engine():
    """engine("large") built with MST_TRAIN_FUSE_BWD_TAIL=2: k_layer_tail_bwd<..., true> with parameter gradients."""
    from mst_amd.engine import DenoiserEngine
    if "fuse2" not in _CACHE:
        w = weights()
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("MST_SMALL_M", "0")
            mp.setenv("MST_TRAIN_FUSE_BWD_TAIL", "2")
            eng = DenoiserEngine(FE, MAX_FRAMES, MAX_ROWS, device=_dev())
        eng.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, layer_prefix="seqTransEncoder.layers.",
                            pe=torch.from_numpy(syn.positional_table(5000, 512)))
        _CACHE["fuse2"] = eng
    return _CACHE["fuse2"]


def get_engine(path):
    return fused_engine() if path == "fuse2" else engine(path)


class Graphs:
    """The float64 reference (torch_stack) and the rounding model (train_profile.stack, f16 operands) of one forward pass, kept as
    autograd graphs: any number of cotangents are differentiated through them.  Computed once per (rows, S, p, padding)."""
    def __init__(self, rows, S, p, padded, tag):
        self.rows, self.S, self.p, self.M = rows, S, p, rows * S
        self.seed = 5150 + 7 * rows + S
        self.keep = pad_keep(S) if padded else None
        self.valid = None if self.keep is None else self.keep[:, :, None].float()
        self.h, r = stream(rows, S, "profile/" + tag)
        self.r = r if self.valid is None else r * self.valid     # outputs at padded positions are unconstrained: score the real ones
        masks = engine_masks(engine("large"), self.seed, p, rows, S) if p > 0 else None
        leaves = lambda: [self.h.double().requires_grad_(True)] + [q.double().requires_grad_(True) for q in layer_params(weights(), False)]
        self.ref_leaves, self.model_leaves = leaves(), leaves()
        self.ref_out = torch_stack(self.ref_leaves[0], self.ref_leaves[1:], masks, self.keep)
        self.model_out = trp.stack(self.model_leaves[0], self.model_leaves[1:], masks, self.keep, dt=torch.float16)
        self._dense = None

    def reference(self, r):
        g = torch.autograd.grad(self.ref_out, self.ref_leaves, grad_outputs=r.double(), retain_graph=True)
        return g[0], list(g[1:])

    def model(self, r):
        g = trp.model_backward(self.model_out, self.model_leaves, r)
        return g[0], list(g[1:])

    def dense_norms(self):
        if self._dense is None:
            d, g = self.reference(self.r)
            self._dense = [float(d.norm())] + [float(x.norm()) for x in g]
        return self._dense


def graphs(rows, S, p, padded=False):
    key = ("graphs", rows, S, p, padded)
    if key not in _CACHE:
        _CACHE[key] = Graphs(rows, S, p, padded, f"{rows}x{S}")
    return _CACHE[key]


def forward(path, g):
    """The engine's forward of the graphs' inputs on one tile path: (out, tape), once per (path, graphs)."""
    key = ("tape", path, id(g))
    if key not in _CACHE:
        _CACHE[key] = get_engine(path).train_forward(g.h, g.p, g.seed, key_keep=g.keep)
    return _CACHE[key]


def backward(path, g, r, frozen=False):
    _, tape = forward(path, g)
    grads = None if frozen else [torch.zeros_like(q) for q in layer_params(weights(), False)]
    d_in = get_engine(path).train_backward(tape, r, g.p, g.seed, grads, key_keep=g.keep)
    return d_in, grads


def gradient_profiles(grads, r_grads, m_grads, M):
    """Worst row / column / block ratio over the 96 tensors, each with where it sits: {kind: (ratio, tensor name, index)}."""
    worst = {"row": (0.0, "", 0), "col": (0.0, "", 0), "block": (0.0, "", 0)}
    for i, (a, b, c) in enumerate(zip(grads, r_grads, m_grads)):
        for kind in (("row", "col") if a.ndim == 2 else ("block",)):
            ratio = trp.vector_ratios(kind, a, b, c)
            j = int(ratio.argmax())
            if float(ratio[j]) > worst[kind][0]:
                worst[kind] = (float(ratio[j]), trp.name_of(i), j)
    return worst


# ------------------------------------------------------------------------------ A. dense cotangent, resolved
#         path     rows  S    p    padded frozen   what it reaches
DENSE = (("small", 3, 77, 0.1, False, False),    # small path, LayerNorms inside the GEMMs, one split
         ("small", 3, 198, 0.1, True, False),    # NKT 7, key padding from a tile boundary and 5 before one
         ("large", 3, 198, 0.1, True, False),
         ("large", 27, 77, 0.1, False, False),   # partial 64-tile of 31 tokens, first multi-split wgrad plan, k_ln_bwd<4>
         ("large", 21, 197, 0.0, False, False),  # k_ln_bwd<16> just above its 4096 threshold, 3-D split grid
         ("large", 37, 197, 0.1, False, False),  # XCD split grid, partial tile of 57, short last splits
         ("large", 21, 197, 0.0, False, True),   # k_layer_tail_bwd with LayerNorm2 fused (grads=None)
         ("large", 3, 198, 0.1, True, True),
         ("fuse2", 27, 77, 0.1, False, False))   # k_layer_tail_bwd<..., true> with parameter gradients


def case_id(path, rows, S, padded=False, frozen=False):
    return f"{path}-{rows}x{S}-M{rows * S}" + ("-keypad" if padded else "") + ("-frozen" if frozen else "") + "-" + plan_str(rows * S)


@pytest.mark.parametrize("path,rows,S,p,padded,frozen", DENSE, ids=[case_id(c[0], c[1], c[2], c[4], c[5]) for c in DENSE])
def test_dense_cotangent_resolved(path, rows, S, p, padded, frozen):
    g = graphs(rows, S, p, padded)
    out, _ = forward(path, g)
    d_in, grads = backward(path, g, g.r, frozen)
    r_din, r_grads = g.reference(g.r)
    m_din, m_grads = g.model(g.r)
    what = label(rows, S, path, p, (" key-padded" if padded else "") + (" frozen" if frozen else ""))
    v = g.valid if g.valid is not None else 1.0
    outs = (out * v, g.ref_out.detach() * v, g.model_out.detach() * v)
    dins = (d_in, r_din, m_din)
    # the figures first
    tok_out, tok_din = float(trp.token_ratios(*outs, g.keep).max()), float(trp.token_ratios(*dins, g.keep).max())
    clip_out, clip_din = float(trp.clip_errors(*outs[:2]).max()), float(trp.clip_errors(*dins[:2]).max())
    print(f"TRAINPROFILE dense {what}: out {trp.rel(*outs[:2]):.2e} (model {trp.rel(outs[2], outs[1]):.2e}), d_in {trp.rel(*dins[:2]):.2e} "
          f"(model {trp.rel(m_din, r_din):.2e}); worst clip out {clip_out:.2e}, d_in {clip_din:.2e}; token ratio out {tok_out:.2f}, d_in {tok_din:.2f}")
    if not frozen:
        worst = gradient_profiles(grads, r_grads, m_grads, g.M)
        print(f"TRAINPROFILE dense {what}: " + ", ".join(f"{k} ratio {w[0]:.2f} ({w[1]} {k} {w[2]})" for k, w in worst.items()))
    # the existing pooled bars, unchanged
    if frozen:
        assert trp.rel(*outs[:2]) <= TOL_FWD and trp.rel(*dins[:2]) <= TOL_GRAD, what
    else:
        check(what, (out, d_in, grads), (g.ref_out.detach(), r_din, r_grads), g.valid)
    # tokens and clips
    trp.assert_clips(*outs[:2], TOL_FWD, what + " out")
    trp.assert_clips(*dins[:2], TOL_GRAD, what + " d_in")
    trp.assert_tokens(*outs, C_TOK, g.keep, what + " out")
    trp.assert_tokens(*dins, C_TOK, g.keep, what + " d_in")
    if padded:
        assert float(r_din[~g.keep].abs().max()) == 0.0
        assert float(d_in[~g.keep].abs().max()) == 0.0, "padded keys received a K/V gradient"
    if not frozen:
        plans = wgrad_plan(g.M)
        for i, (a, b, c) in enumerate(zip(grads, r_grads, m_grads)):
            trp.assert_gradient(i, a, b, c, C_GROW, C_VEC, plans, g.M, what)


# ------------------------------------------------------------------------------ B. localized cotangents
def token_sets(rows, S, keep=None):
    """name -> sorted list of (clip, token)."""
    M = rows * S
    at = lambda row: divmod(row, S)
    sets = {"last-token": [at(M - 1)]}
    c = rows // 2                                                    # a clip in the middle of the launch
    sets["tile-edges"] = [at(m + d) for m in range(64, M, 64) for d in (-1, 0) if c * S <= m - 1 and m <= (c + 1) * S - 1]
    sets["split-edges"] = sorted({at(row) for _, _, last in wgrad_plan(M).values() for row in (M - last, M - 1)})
    sets["clip-token0"] = [(b, 0) for b in range(rows)]
    if keep is not None:
        sets = {"last-real-key": [(b, int(keep[b].sum()) - 1) for b in range(rows) if int(keep[b].sum()) < S]}
    assert all(v for v in sets.values()), sets
    return sets


def local_cotangent(r, tokens):
    out = torch.zeros_like(r)
    for b, t in tokens:
        out[b, t] = r[b, t]
    return out


LOCAL = ([(path, rows, S, False, name) for path, rows, S in (("small", 3, 77), ("large", 27, 77), ("large", 37, 197))
          for name in ("last-token", "tile-edges", "split-edges", "clip-token0")]
         + [(path, 3, 198, True, "last-real-key") for path in ("small", "large")])
MAX_SKIPPED_SHARE = 0.10
NEGLIGIBLE = 1e-12               # of the tensor's dense-case norm: the reference itself has no gradient there


@pytest.mark.parametrize("path,rows,S,padded,name", LOCAL, ids=[f"{c[4]}-" + case_id(c[0], c[1], c[2], c[3]) for c in LOCAL])
def test_localized_cotangent(path, rows, S, padded, name):
    g = graphs(rows, S, 0.1, padded)
    tokens = token_sets(rows, S, g.keep)[name]
    clips = sorted({b for b, _ in tokens})
    r = local_cotangent(g.r, tokens)
    d_in, grads = backward(path, g, r)
    r_din, r_grads = g.reference(r)
    m_din, m_grads = g.model(r)
    what = f"{name} {tokens if len(tokens) <= 8 else str(tokens[:8]) + ' ...'} of {label(rows, S, path, 0.1)}"
    dense = g.dense_norms()
    ratios, skipped = {}, []
    for nm, a, b, c, dn in [("d_in", d_in, r_din, m_din, dense[0])] + [(trp.name_of(i), grads[i], r_grads[i], m_grads[i], dense[1 + i]) for i in range(96)]:
        if float(b.norm()) < NEGLIGIBLE * dn:
            skipped.append(nm)
            continue
        ratios[nm] = (trp.rel(a, b) / max(trp.rel(c, b), trp.FLOOR), trp.rel(a, b), trp.rel(c, b))
    worst = max(ratios, key=lambda k: ratios[k][0])
    sel = torch.tensor(clips, device=d_in.device)
    keep = None if g.keep is None else g.keep[sel]
    tok = float(trp.token_ratios(d_in[sel], r_din[sel], m_din[sel], keep).max())
    print(f"TRAINPROFILE local {what}: worst pooled ratio {ratios[worst][0]:.2f} at {worst} (kernel {ratios[worst][1]:.2e}, model {ratios[worst][2]:.2e}), "
          f"d_in {ratios['d_in'][1]:.2e} (model {ratios['d_in'][2]:.2e}), token ratio on clips {clips if len(clips) <= 8 else len(clips)} {tok:.2f}, skipped {skipped}")
    assert len(skipped) <= MAX_SKIPPED_SHARE * 97, skipped
    assert ratios[worst][0] <= C_POOL, (what, worst, ratios[worst])
    trp.assert_tokens(d_in[sel], r_din[sel], m_din[sel], C_TOK, keep, what + " d_in")
    others = torch.ones(rows, dtype=torch.bool, device=d_in.device)
    others[sel] = False
    if bool(others.any()):
        assert float(r_din[others].abs().max()) == 0.0
        assert float(d_in[others].abs().max()) == 0.0, f"{what}: a clip without a cotangent received a gradient"
    if padded:
        assert float(r_din[~g.keep].abs().max()) == 0.0 and float(d_in[~g.keep].abs().max()) == 0.0, "padded keys received a K/V gradient"


# ------------------------------------------------------------------------------ C. cotangent dynamic range
RANGE = (("small", 4, 77), ("large", 27, 77))


def exponent_launches(rows):
    """Per launch the exponent of every clip, cycling: all six where the clips suffice, else two launches that cover them."""
    if rows >= len(EXPONENTS):
        return [[EXPONENTS[b % len(EXPONENTS)] for b in range(rows)]]
    return [[(0, 6, 12, 16)[b % 4] for b in range(rows)], [(0, 16, 20, 24)[b % 4] for b in range(rows)]]


def scaled(r, ks):
    return r * torch.tensor([2.0 ** -k for k in ks], device=r.device, dtype=r.dtype).view(-1, 1, 1)


def supported(table):
    """The largest exponent up to which every clip met TOL_GRAD: table = {k: (worst kernel error, worst model error)}."""
    ok = -1
    for k in sorted(table):
        if table[k][0] > TOL_GRAD:
            break
        ok = k
    return ok


@pytest.mark.parametrize("frozen", (False, True), ids=("trainable", "frozen"))
@pytest.mark.parametrize("path,rows,S", RANGE, ids=[case_id(*c) for c in RANGE])
def test_cotangent_dynamic_range(path, rows, S, frozen):
    g = graphs(rows, S, 0.1)
    what = label(rows, S, path, 0.1, " frozen" if frozen else "")
    table, worst_ratio, fails = {}, 0.0, []
    for ks in exponent_launches(rows):
        r = scaled(g.r, ks)
        d_in, grads = backward(path, g, r, frozen)
        r_din, r_grads = g.reference(r)
        m_din, _ = g.model(r)
        ek, em = trp.clip_errors(d_in, r_din).tolist(), trp.clip_errors(m_din, r_din).tolist()
        for b, k in enumerate(ks):
            table[k] = (max(table.get(k, (0, 0))[0], ek[b]), max(table.get(k, (0, 0))[1], em[b]))
            if em[b] < 1e-2:                                                   # (a) the kernel against gradual f16 underflow
                worst_ratio = max(worst_ratio, ek[b] / max(em[b], trp.FLOOR))
                if ek[b] > C_CLIP * max(em[b], trp.FLOOR):
                    fails.append((b, k, ek[b], em[b]))
        if not frozen:
            gerr = {trp.name_of(i): trp.rel(a, b) for i, (a, b) in enumerate(zip(grads, r_grads))}
            w = max(gerr, key=gerr.get)
            print(f"TRAINPROFILE range {what} exponents {sorted(set(ks))}: worst gradient vs fp64 {w} {gerr[w]:.2e}")
            assert gerr[w] <= TOL_GRAD, (what, w, gerr[w])
    print(f"TRAINPROFILE range {what}: per-clip d_in error, kernel | model: " + ", ".join(f"2^-{k}: {table[k][0]:.2e} | {table[k][1]:.2e}" for k in sorted(table))
          + f"; worst kernel / model ratio {worst_ratio:.2f}; R = {supported(table)}")
    assert not fails, (what, "clip, exponent, kernel, model", fails)
    assert R_SUPPORTED is not None and OBJECTIVE_RATIO is not None, "the supported range has not been measured"
    assert supported(table) >= R_SUPPORTED, (what, table)
    assert 2.0 ** R_SUPPORTED >= 16 * OBJECTIVE_RATIO
    if frozen:
        return
    # the gradients of a launch whose smallest clip sits at 2^-k: the mixed launch equals the sum of its per-exponent launches
    for kmax in [k for k in EXPONENTS if 0 < k <= R_SUPPORTED]:
        exps = [k for k in EXPONENTS if k <= kmax]
        ks = [exps[b % len(exps)] for b in range(rows)]
        _, g_all = backward(path, g, scaled(g.r, ks))
        g_sum = [torch.zeros_like(x) for x in g_all]
        for k in sorted(set(ks)):
            part = scaled(g.r, ks) * torch.tensor([float(kb == k) for kb in ks], device=g.r.device).view(-1, 1, 1)
            _, gk = backward(path, g, part)
            g_sum = [a + b for a, b in zip(g_sum, gk)]
        errs = {trp.name_of(i): trp.rel(a, b) for i, (a, b) in enumerate(zip(g_sum, g_all))}
        w = max(errs, key=errs.get)
        print(f"TRAINPROFILE range {what}: exponents up to {kmax} vs the sum of per-exponent launches: worst gradient {w} {errs[w]:.2e}")
        assert errs[w] < 2e-5, (what, kmax, w, errs[w])


@pytest.mark.parametrize("path,rows,S", RANGE, ids=[case_id(*c) for c in RANGE])
def test_cotangent_range_inside_one_clip(path, rows, S):
    """Clip 1: eight tokens at 2^0, the others at 2^-16; every other clip at 2^-16.  dL/dh per token group of clip 1 and per clip."""
    g = graphs(rows, S, 0.1)
    what = label(rows, S, path, 0.1)
    loud = torch.zeros(rows, S, dtype=torch.bool, device=_dev())
    loud[1, torch.arange(8, device=_dev()) * (S // 8) + 3] = True
    r = g.r * torch.where(loud, 1.0, 2.0 ** -16)[:, :, None]
    d_in, _ = backward(path, g, r, frozen=True)
    r_din, _ = g.reference(r)
    m_din, _ = g.model(r)
    groups = {"clip 1, the 8 tokens": loud, "clip 1, the other tokens": ~loud & (torch.arange(rows, device=_dev()) == 1)[:, None]}
    groups.update({f"clip {b}": (torch.arange(rows, device=_dev()) == b)[:, None].expand(rows, S) for b in range(rows) if b != 1})
    fails, lines, worst_ratio = [], [], 0.0
    for name, sel in groups.items():
        ek, em = trp.rel(d_in[sel], r_din[sel]), trp.rel(m_din[sel], r_din[sel])
        if em < 1e-2:
            worst_ratio = max(worst_ratio, ek / max(em, trp.FLOOR))
            if ek > C_CLIP * max(em, trp.FLOOR):
                fails.append((name, ek, em))
        if name.startswith("clip 1,") or name in ("clip 0", f"clip {rows - 1}"):
            lines.append(f"{name}: {ek:.2e} | {em:.2e}")
    print(f"TRAINPROFILE range inside one clip {what}: d_in error, kernel | model: " + ", ".join(lines) + f"; worst kernel / model ratio {worst_ratio:.2f}")
    assert not fails, (what, fails)
