"""numpy restatement of the fused AdamW step and its norms (`FusedAdamW` in optim.py, `mst_adamw_step`, `k_adamw_multi` and
`k_adamw_norms` at the end of csrc/mst_train.h), the tensor layouts, value classes and hyperparameter sets the optimizer tests run
on, and the judge that compares one step with both forms.  No GPU import: tests/test_optim_cpu.py holds everything here to
torch.optim.AdamW on the CPU, tests/test_gpu_optim.py feeds the judge the kernel's own buffers.

Every function takes a dtype.  float64 is the oracle: the five scalars rounded to float32 (what the C ABI receives) and widened
again, the bias corrections in double, torch's formula.  float32 is the restatement: the kernel's expression order, operation by
operation and without contraction, with the two bias terms rounded to float32 where `mst_adamw_step` rounds them.

The rule is the suite's (tests/track_fixture.py): `distance` = max |a - b| over the largest |b|, and the kernel may be
`bar` = max(4 x the restatement's own distance, 1e-6) away from float64.  One widening, for the update p' - p alone: any float32
evaluation rounds three values of p's magnitude (the factor 1 - lr wd, p times it, and p' itself), so a tensor on which the
restatement's own roundings happen to fall small (a tensor of one to seven elements) still admits 3 x 2^-24 max |p| over the largest
update; on tensors of hundreds of elements 4 x the restatement's distance is the larger of the two."""
import numpy as np

CHUNK, LANES = 65536, 256                   # kAdamChunk, the block size of both kernels
FLOOR = 1e-6
V_ELEM_BAR, V_ELEM_MIN = 4.0 * 2.0 ** -24, 2.0 ** -100
SEED = 20261021

HYPERS = {
    "torch": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2),      # torch's defaults
    "loop": dict(lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),        # TrainInpaintingLoop's
    "old": dict(lr=3e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.05),         # test_fused_adamw_step_equals_torch_adamw's
    "far": dict(lr=0.1, betas=(0.5, 0.9), eps=1e-3, weight_decay=0.3),            # far from every default
}

EDGES = [1, 255, 256, 257, 65535, 65536, 65537, 131072, 131073]
MIXED = [3, 3 * 65536 + 5, 1, 65536, 2, 2 * 65536, 70001]
# one seqTransEncoder layer in named_parameters() order: in_proj weight and bias, out_proj, linear1, linear2, norm1, norm2
LAYER_SHAPES = [(1536, 512), (1536,), (512, 512), (512,), (1024, 512), (1024,), (512, 1024), (512,), (512,), (512,), (512,), (512,)]
LAYER = [int(np.prod(s)) for s in LAYER_SHAPES]
P_SCALES = (0.0, 1e-3, 1.0, 30.0)
P_NAMES = ("p=0", "p=1e-3", "p=1", "p=30")


def MANY(k):
    return [(i % 7) + 1 for i in range(k)]


def nchunks(layout):
    return sum(-(-n // CHUNK) for n in layout)


def distance(a, b):
    """max |a - b| over the largest magnitude of b."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)) if b.size else 0.0


def bar(own):
    """4 x the float32 restatement's own distance from float64, floor 1e-6."""
    return max(4.0 * float(own), FLOOR)


# ------------------------------------------------------------------------------------------ one step
def scalars(hyper):
    """-> (lr, beta1, beta2, eps, weight_decay) as float32: what the ABI's `float` arguments hold."""
    b1, b2 = hyper["betas"]
    return tuple(np.float32(x) for x in (hyper["lr"], b1, b2, hyper["eps"], hyper["weight_decay"]))


def widened(hyper):
    """The same five, rounded to float32 and widened again, as keyword arguments of torch.optim.AdamW."""
    lr, b1, b2, eps, wd = (float(x) for x in scalars(hyper))
    return dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)


def decays(hyper):
    """The float32 factor 1 - lr wd as its two float32 evaluations: the product rounded and then the difference (the restatement),
    or both in one rounding (a fused multiply-add; also what torch forms, in double, before it rounds)."""
    lr, _, _, _, wd = scalars(hyper)
    return np.float32(1.0) - lr * wd, np.float32(1.0 - float(lr) * float(wd))


def adamw_step(p, g, m, v, hyper, step, dtype, mutate=()):
    """-> (p', m', v') in `dtype`.  mutate (float32 only, for tests/test_optim_cpu.py): 'no_eps' drops `+ eps`, 'beta1_for_beta2'
    puts beta1 where beta2 belongs in the second moment."""
    lr, b1, b2, eps, wd = scalars(hyper)
    t = float(int(step))
    if np.dtype(dtype) == np.float64:
        assert not mutate
        lr, b1, b2, eps, wd = (float(x) for x in (lr, b1, b2, eps, wd))
        p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
        bias1, bias2_sqrt = 1.0 - b1 ** t, np.sqrt(1.0 - b2 ** t)
        p = p * (1.0 - lr * wd)
        m = m + (1.0 - b1) * (g - m)
        v = b2 * v + (1.0 - b2) * g * g
        denom = np.sqrt(v) / bias2_sqrt + eps
        return p - (lr / bias1) * (m / denom), m, v
    assert np.dtype(dtype) == np.float32
    f, one = np.float32, np.float32(1.0)
    p, g, m, v = (np.asarray(a, np.float32) for a in (p, g, m, v))
    bias1 = one - f(float(b1) ** t)                               # mst_adamw_step: 1.0f - (float)pow((double)beta1, step)
    bias2_sqrt = f(np.sqrt(1.0 - float(b2) ** t))                 # (float)sqrt(1.0 - pow((double)beta2, step))
    step_size, decay = lr / bias1, one - lr * wd
    c2 = b1 if "beta1_for_beta2" in mutate else b2
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        p = p * decay
        m = m + (one - b1) * (g - m)
        v = c2 * v + ((one - c2) * g) * g
        denom = np.sqrt(v) / bias2_sqrt
        if "no_eps" not in mutate:
            denom = denom + eps
        p = p - step_size * (m / denom)
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


def torch_adamw(before, hyper, step0, dtype, n=1, lrs=None, grads=None):
    """torch.optim.AdamW (single-tensor form) on CPU tensors of `dtype`, the scalars rounded to float32 and widened ->
    after n steps, dict p, m, v of lists of numpy arrays."""
    import torch
    ps = [torch.from_numpy(np.array(p)).to(dtype).requires_grad_(True) for p in before["p"]]
    opt = torch.optim.AdamW(ps, foreach=False, **widened(hyper))
    for p, m, v in zip(ps, before["m"], before["v"]):
        opt.state[p] = {"step": torch.tensor(float(step0)), "exp_avg": torch.from_numpy(np.array(m)).to(dtype),
                        "exp_avg_sq": torch.from_numpy(np.array(v)).to(dtype)}
    for k in range(n):
        for p, g in zip(ps, (grads[k] if grads is not None else before["g"])):
            p.grad = torch.from_numpy(np.array(g)).to(dtype)
        if lrs is not None:
            opt.param_groups[0]["lr"] = float(np.float32(lrs[k]))
        opt.step()
    assert all(int(opt.state[p]["step"]) == step0 + n for p in ps)
    return {"p": [p.detach().numpy() for p in ps], "m": [opt.state[p]["exp_avg"].numpy() for p in ps],
            "v": [opt.state[p]["exp_avg_sq"].numpy() for p in ps]}


# ------------------------------------------------------------------------------------------ the two norms
def _partials32(chunks):
    """Per chunk, the float32 sum of squares as one k_adamw_multi block forms it: each of 256 threads adds its strided elements
    serially, six xor steps inside each wave of 64, the four wave sums added 0..3."""
    if not chunks:
        return np.zeros(0, np.float32)
    iters = max(-(-len(c) // LANES) for c in chunks)
    buf = np.zeros((len(chunks), iters * LANES), np.float32)      # a missing element adds +0.0, which changes no partial sum
    for i, c in enumerate(chunks):
        buf[i, :len(c)] = c
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        sq = buf * buf
        acc = np.zeros((len(chunks), LANES), np.float32)
        for k in range(iters):
            acc = acc + sq[:, k * LANES:(k + 1) * LANES]
        acc = acc.reshape(len(chunks), 4, 64)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, :, lane ^ o]
        w = acc[:, :, 0]
        return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def _reduce32(partials, stride=LANES):
    """k_adamw_norms: thread t adds partials t, t + stride, ... serially, then the 256 thread sums are added serially."""
    part = np.asarray(partials, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.float32(0.0)
        for t in range(LANES):
            a = np.float32(0.0)
            for x in part[t::stride]:
                a = a + x
            s = s + a
    return np.float32(0.0) + s                                    # norms[k] += s on the zeroed pair


def chunks_of(xs):
    return [x[s:s + CHUNK] for x in (np.asarray(x).reshape(-1) for x in xs) for s in range(0, x.size, CHUNK)]


def sq_norms(gs, ps, dtype, stride=LANES):
    """-> (sum g^2, sum p^2) over the tensors of a group.  float64: plain sums.  float32: the kernels' order."""
    if np.dtype(dtype) == np.float64:
        return tuple(float(sum((np.asarray(x, np.float64) ** 2).sum() for x in xs)) for xs in (gs, ps))
    return tuple(_reduce32(_partials32(chunks_of([np.asarray(x, np.float32) for x in xs])), stride) for xs in (gs, ps))


# ------------------------------------------------------------------------------------------ layouts in memory
def carve(layout, gap=3, fill=0.0):
    """-> (flat float32 buffer, slices): the tensors of a layout in one buffer, `gap` floats holding `fill` in front of, between and
    behind them, so that most tensors start off a 16-byte boundary as the views of a gradient bucket do."""
    offs, off = [], gap
    for n in layout:
        offs.append(off)
        off += n + gap
    flat = np.full(off, fill, np.float32)
    return flat, [slice(o, o + n) for o, n in zip(offs, layout)]


def gap_mask(size, slices):
    m = np.ones(size, bool)
    for s in slices:
        m[s] = False
    return m


GAP_BITS = 0x4B3C614E                                             # 12345678.0f: what the p, m and v gaps hold
GAP_FILL = np.array([GAP_BITS], np.int32).view(np.float32)[0]


# ------------------------------------------------------------------------------------------ value classes
def p_class(i):
    return i % 4


def g_class(i):
    return (i + i // 4) % 4


def _log_uniform(g, n, lo, hi):
    return 10.0 ** g.uniform(lo, hi, n)


def params(layout, seed=SEED):
    """Per tensor i, class i % 4: exactly 0, or normal x 1e-3, 1, 30."""
    g = np.random.default_rng([seed, 1, len(layout)])
    return [(g.standard_normal(n) * P_SCALES[p_class(i)]).astype(np.float32) for i, n in enumerate(layout)]


def grads(layout, it=0, scale=1.0, seed=SEED):
    """Per tensor i, class (i + i // 4) % 4: normal; random sign x log-uniform in [1e-12, 1e-2]; either with every third entry 0."""
    g = np.random.default_rng([seed, 2, len(layout), it])
    out = []
    for i, n in enumerate(layout):
        c = g_class(i)
        x = g.standard_normal(n) if c % 2 == 0 else np.where(g.integers(0, 2, n) == 0, -1.0, 1.0) * _log_uniform(g, n, -12, -2)
        if c >= 2:
            x[::3] = 0.0
        out.append((x * scale).astype(np.float32))
    return out


def moments(layout, resumed, seed=SEED):
    """-> (m, v): zeros for a first step, or m normal x 1e-3 and v log-uniform in [1e-22, 1e-2]."""
    if not resumed:
        return [np.zeros(n, np.float32) for n in layout], [np.zeros(n, np.float32) for n in layout]
    g = np.random.default_rng([seed, 3, len(layout)])
    return ([(g.standard_normal(n) * 1e-3).astype(np.float32) for n in layout],
            [_log_uniform(g, n, -22, -2).astype(np.float32) for n in layout])


# ------------------------------------------------------------------------------------------ a whole group on the host
def emulate(flats, slices, hyper, step, mutate=()):
    """The launch restated in float32 on carved host buffers, chunk by chunk in table order, in place -> (sum g^2, sum p^2).
    flats: dict p, g, m, v of flat float32 arrays sharing `slices`.  mutate: adamw_step's, and 'unclamped' (a chunk runs to
    start + 65536 whatever the tensor's size; it stops at the end of the buffer here, where a kernel would not) and 'stride255'
    (the norm kernel's thread stride)."""
    size = flats["p"].size
    part_g, part_p = [], []
    for s in slices:
        for s0 in range(s.start, s.stop, CHUNK):
            s1 = min(s0 + CHUNK, size) if "unclamped" in mutate else min(s0 + CHUNK, s.stop)
            c = slice(s0, s1)
            part_g.append(flats["g"][c].copy())
            part_p.append(flats["p"][c].copy())
            flats["p"][c], flats["m"][c], flats["v"][c] = adamw_step(flats["p"][c], flats["g"][c], flats["m"][c], flats["v"][c],
                                                                     hyper, step, np.float32, mutate)
    stride = 255 if "stride255" in mutate else LANES
    return _reduce32(_partials32(part_g), stride), _reduce32(_partials32(part_p), stride)


# ------------------------------------------------------------------------------------------ the judge
class Tally:
    """What the comparisons of a file measured: per class the worst ratio to the bar, with the distances of that comparison."""

    def __init__(self):
        self.worst = {}
        self.updates = self.widened = 0     # update comparisons, and those that passed by `update_floor` alone
        self.widened_numel = 0              # the largest tensor among the latter

    def add(self, cls, case, d32, d, b):
        r = d / b
        if cls not in self.worst or r > self.worst[cls][0]:
            self.worst[cls] = (r, case, d32, d, b)
        return r

    def lines(self):
        return [f"optim: worst {cls}: {case} restatement {d32:.3e} kernel {d:.3e} bar {b:.3e} ratio {r:.3f}"
                for cls, (r, case, d32, d, b) in sorted(self.worst.items())]

    def worst_ratio(self):
        return max((w[0] for w in self.worst.values()), default=0.0)


def _line(case, d32, d, b):
    return f"optim: {case} restatement {d32:.3e} kernel {d:.3e} bar {b:.3e} ratio {d / b:.3f}"


def update_floor(p64_after, upd64):
    """Three float32 roundings at p's magnitude, in the unit of `distance` on the update."""
    return 3.0 * 2.0 ** -24 * float(np.abs(p64_after).max()) / max(float(np.abs(upd64).max()), 1e-30)


def judge_step(case, before, after, hyper, step, tally=None, out=print):
    """One step of a group against both forms.  before: dict p, g, m, v of lists of float32 host arrays, the values the step
    read; after: dict p, m, v, what it left.  Per tensor: the update p' - p (formed in float64 from the float32 values), m', v',
    v' per element, and the exact cases.  Asserts; prints one line per quantity and parameter class, that of the tensor closest
    to its bar."""
    tally = tally if tally is not None else Tally()
    worst = {}
    for i, (p, g, m, v) in enumerate(zip(before["p"], before["g"], before["m"], before["v"])):
        got = {k: np.asarray(after[k][i]) for k in ("p", "m", "v")}
        assert all(a.dtype == np.float32 and a.shape == p.shape for a in got.values())
        assert all(np.isfinite(a).all() for a in got.values()), (case, i, "a value is not finite")
        p64, m64, v64 = adamw_step(p, g, m, v, hyper, step, np.float64)
        p32, m32, v32 = adamw_step(p, g, m, v, hyper, step, np.float32)
        pw = p.astype(np.float64)
        upd64 = p64 - pw
        rows = [("update/" + P_NAMES[p_class(i)], distance(p32.astype(np.float64) - pw, upd64),
                 distance(got["p"].astype(np.float64) - pw, upd64), update_floor(p64, upd64)),
                ("m", distance(m32, m64), distance(got["m"], m64), 0.0), ("v", distance(v32, v64), distance(got["v"], v64), 0.0)]
        big = v64 >= V_ELEM_MIN
        if big.any():
            rel = lambda a: float((np.abs(a.astype(np.float64) - v64)[big] / v64[big]).max())
            rows.append(("v per element", rel(v32), rel(got["v"]), None))
        for cls, d32, d, floor in rows:
            b = V_ELEM_BAR if floor is None else max(bar(d32), floor)
            if cls.startswith("update"):
                tally.updates += 1
                if bar(d32) < d <= b:
                    tally.widened, tally.widened_numel = tally.widened + 1, max(tally.widened_numel, p.size)
            r = tally.add(cls, f"{case} tensor {i} ({p.size})", d32, d, b)
            if cls not in worst or r > worst[cls][0]:
                worst[cls] = (r, f"{case} {cls} tensor {i} ({p.size})", d32, d, b)
            assert d <= b, _line(f"{case} {cls} tensor {i} ({p.size})", d32, d, b)
        still = (g == 0) & (m == 0) & (v == 0)                    # nothing to move: both moments stay 0, p only decays
        if still.any():
            assert not got["m"][still].any() and not got["v"][still].any(), (case, i, "moments of an all-zero element")
            assert any(np.array_equal(got["p"][still], (p * d)[still]) for d in decays(hyper)), (case, i, "p of an all-zero element")
    for cls in sorted(worst):
        out(_line(*worst[cls][1:]))
    return tally


def judge_norms(case, gs, ps, got, tally=None, out=print, extra64=(0.0, 0.0), extra32=(0.0, 0.0)):
    """last_sq_norms against the float64 sums of g^2 and of p^2 (the parameters before the update)."""
    tally = tally if tally is not None else Tally()
    n64, n32 = sq_norms(gs, ps, np.float64), sq_norms(gs, ps, np.float32)
    for k, name in enumerate(("sum g^2", "sum p^2")):
        ref = n64[k] + extra64[k]
        assert np.isfinite(got[k]), (case, name, got[k])
        d32, d = distance(float(n32[k]) + extra32[k], ref), distance(float(got[k]), ref)
        b = bar(d32)
        tally.add("norms", f"{case} {name}", d32, d, b)
        out(_line(f"{case} {name}", d32, d, b))
        assert d <= b, _line(f"{case} {name}", d32, d, b)
    return tally
