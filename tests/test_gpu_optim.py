"""`FusedAdamW.step()` -- optim.py's table tracking, `mst_adamw_step`, `k_adamw_multi` and `k_adamw_norms` -- against float64,
chunk by chunk (tests/optim_fixture.py; tests/test_optim_cpu.py holds that fixture to torch.optim.AdamW).

Every comparison is one step ahead: the kernel's own p, m and v are copied to the host before the step and fed to the float64
oracle and to the float32 restatement, so nothing accumulates and a tensor of exact zeros stays one.  Per tensor: the update
p' - p (formed in float64 from the float32 values; for parameters of size 0 and 1e-3 this is the arithmetic itself), m', v', v'
per element at 4 x 2^-24 relative, the exact cases (g = m = v = 0), and the two norms against the float64 sums of that step.
The rule: the kernel may be max(4 x the restatement's distance, 1e-6) from float64 (the fixture's head states the one
widening, for the update of a few-element tensor).

  a. three steps (gradients x 0.1, 1, 10) on EDGES, MANY(255 | 256 | 257 | 300) and MIXED, the four hyperparameter sets rotated
  b. resumed moments at t = 1000 and t = 100000
  c. the norms after every step of a, b, d, f: 255 .. 300 chunks sit on both sides of k_adamw_norms' thread stride
  d. p, g, m and v are views carved from flat buffers with gaps of 3 floats, so most start off a 16-byte boundary: NaN in g's
     gaps (a read past a tensor shows in its outputs and in the norms), a bit pattern in the others (a write past a tensor
     shows); one seqTransEncoder layer with its gradients as views of one bucket, as LayerBucketReducer builds them
  e. a tensor's bits do not depend on its company, on the stream, on the run, or on NaN in its neighbours' gradients
  f. the device-side tables follow new, swapped and reloaded tensors; parameters without a gradient are left alone
  g. twelve annealed steps against torch.optim.AdamW in float64
  h. MixedPrecisionTrainer.optimize's norms with frozen and idle parameters
  i. a refused step changes nothing, and the next step gives the bits of an optimizer that never saw it

`-s` prints `optim: <case> <quantity> tensor <i> (<numel>) restatement <d32> kernel <d> bar <b> ratio <r>` per case, step,
quantity and parameter class -- the tensor closest to its bar; every tensor is asserted -- and the last test prints the worst
per class.

Measured on an MI355X, no kernel changed (27 tests, 401 printed comparisons, the file takes 5.5 s; per class the largest
distances over the file, restatement | kernel, and the worst ratio to the bar):

    update, p = 0           5.5e-7 | 4.8e-7   0.40      m'                       2.9e-7 | 2.7e-7   0.25
    update, p of size 1e-3  4.6e-3 | 4.6e-3   0.48      v'                       3.0e-7 | 3.0e-7   0.25
    update, p of size 1     2.3e-2 | 2.3e-2   0.47      v' per element           1.7e-7 | 1.2e-7   0.50  (bar 2.4e-7)
    update, p of size 30    3.8e-1 | 3.8e-1   0.47      sum g^2                  4.2e-7 | 4.2e-7   0.25
    twelve annealed steps   4.0e-7 | 3.1e-7   0.26      sum p^2                  2.7e-7 | 2.7e-7   0.25
    trainer norms           3.4e-8 | 3.5e-8   0.04

The worst ratio over the file is 0.50 (v' per element on the 524 288-element tensor of the layer).  The update distances grow with
p because the update is measured against p's own rounding: at lr = 1e-5 the update of a parameter of size 30 is a fraction of its
last bit.  Most kernel figures equal the restatement's: the kernel follows it operation by operation, and differs where the
compiler contracted a product into a fused multiply-add.  The fixture's widening of the update's bar decided 12 of the 3927 update
comparisons, all on tensors of at most 6 elements."""
import copy

import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
import optim_fixture as of

pytestmark = pytest.mark.gpu
TALLY = of.Tally()


def dev():
    return torch.device("cuda:0")


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())


def host(ts):
    """A list of device tensors -> float32 host arrays (flattened), in one copy."""
    flat = torch.cat([t.detach().reshape(-1) for t in ts]).cpu().numpy()
    out, off = [], 0
    for t in ts:
        out.append(flat[off:off + t.numel()].copy())
        off += t.numel()
    return out


def values(layout, resumed, seed=of.SEED):
    m, v = of.moments(layout, resumed, seed)
    return {"p": of.params(layout, seed), "m": m, "v": v}


def snapshot(opt, params):
    """What the next step() will read: p, g and the moments (zeros where the state does not exist yet)."""
    zero = lambda p: torch.zeros_like(p)
    return {"p": host(params), "g": host([p.grad for p in params]),
            "m": host([opt.state[p]["exp_avg"] if p in opt.state and len(opt.state[p]) else zero(p) for p in params]),
            "v": host([opt.state[p]["exp_avg_sq"] if p in opt.state and len(opt.state[p]) else zero(p) for p in params])}


def judged_step(case, opt, params, t, hyper=None):
    """step() with a gradient on every tensor of `params`, held to the oracle; `t` is the step count the kernel must run at."""
    from mst_amd.optim import FusedAdamW
    assert isinstance(opt, FusedAdamW)
    hyper = hyper or {k: opt.param_groups[0][k] for k in ("lr", "betas", "eps", "weight_decay")}
    before = snapshot(opt, params)
    opt.step()
    norms = opt.last_sq_norms.cpu().numpy().copy()
    assert norms.dtype == np.float32 and norms.shape == (2,)
    after = {"p": host(params), "m": host([opt.state[p]["exp_avg"] for p in params]),
             "v": host([opt.state[p]["exp_avg_sq"] for p in params])}
    assert all(int(opt.state[p]["step"]) == t for p in params)
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(before["g"], host([p.grad for p in params])))
    of.judge_step(f"{case} t={t}", before, after, hyper, t, TALLY)
    of.judge_norms(f"{case} t={t}", before["g"], before["p"], norms, TALLY)
    return before, after, norms


class Carved:
    """A group whose p, g, m and v are views of four flat device buffers with 3-float gaps: NaN in g's, a bit pattern in the
    others'.  bucket: the gradients are views of one gap-free bucket instead, as LayerBucketReducer.__init__ builds them."""

    def __init__(self, layout, hyper, vals, step0=0, shapes=None, bucket=False):
        from mst_amd.optim import FusedAdamW
        self.layout, self.hyper = layout, hyper
        self.flat, self.host_g = {}, None
        for k, fill in (("p", of.GAP_FILL), ("m", of.GAP_FILL), ("v", of.GAP_FILL), ("g", np.nan)):
            h, self.slices = of.carve(layout, fill=fill)
            for s, x in zip(self.slices, vals.get(k, [])):
                h[s] = x
            self.flat[k] = torch.from_numpy(h).to(dev())
            if k == "g":
                self.host_g = h
        shapes = shapes or [(n,) for n in layout]
        view = lambda k: [self.flat[k][s].view(shape) for s, shape in zip(self.slices, shapes)]
        self.params = [p.requires_grad_(True) for p in view("p")]
        self.gaps = of.gap_mask(self.flat["p"].numel(), self.slices)
        assert self.flat["p"].data_ptr() % 16 == 0 and any(p.data_ptr() % 16 for p in self.params)
        if bucket:
            self.bucket = torch.zeros(sum(layout), dtype=torch.float32, device=dev())
            off = 0
            for p in self.params:                                  # finetune_dp.LayerBucketReducer.__init__
                p.grad = self.bucket[off:off + p.numel()].view_as(p)
                off += p.numel()
        else:
            self.bucket = None
            for p, g in zip(self.params, view("g")):
                p.grad = g
        self.opt = FusedAdamW(self.params, **hyper)
        for p, m, v in zip(self.params, view("m"), view("v")):
            self.opt.state[p] = {"step": torch.tensor(float(step0)), "exp_avg": m, "exp_avg_sq": v}

    def set_grads(self, gs):
        """In place: the gradient buffers keep their addresses, as a bucket's do."""
        if self.bucket is not None:
            self.bucket.copy_(up(np.concatenate(gs)))
            return
        for s, x in zip(self.slices, gs):
            self.host_g[s] = x
        self.flat["g"].copy_(torch.from_numpy(self.host_g))

    def gaps_intact(self):
        for k in "pmv":
            bits = self.flat[k].cpu().numpy().view(np.int32)
            assert (bits[self.gaps] == of.GAP_BITS).all(), (k, "a gap was written")
        assert np.isnan(self.flat["g"].cpu().numpy()[self.gaps]).all()

    def step(self, case, t):
        out = judged_step(case, self.opt, self.params, t, self.hyper)
        self.gaps_intact()
        return out


# ------------------------------------------------------------------------------------------ a, c, d: one step ahead, per layout
A_CASES = [("EDGES", of.EDGES, "torch"), ("MANY255", of.MANY(255), "loop"), ("MANY256", of.MANY(256), "old"),
           ("MANY257", of.MANY(257), "far"), ("MANY300", of.MANY(300), "torch"), ("MIXED", of.MIXED, "loop"),
           ("EDGES-far", of.EDGES, "far"), ("MIXED-old", of.MIXED, "old")]


def test_every_hyperparameter_set_occurs():
    assert {h for _, _, h in A_CASES} == set(of.HYPERS)
    assert [of.nchunks(l) for _, l, _ in A_CASES[1:5]] == [255, 256, 257, 300]


@pytest.mark.parametrize("name,layout,hname", A_CASES, ids=[c[0] for c in A_CASES])
def test_three_steps_one_step_ahead(name, layout, hname):
    grp = Carved(layout, of.HYPERS[hname], values(layout, False))
    seen = []
    for it in range(3):
        grp.set_grads(of.grads(layout, it, 10.0 ** (it - 1)))
        _, _, norms = grp.step(f"{name}/{hname}", it + 1)
        seen.append(norms)
    # each step's gradients are ten times the last's, and each step's sum is its own
    assert seen[1][0] > 50 * seen[0][0] and seen[2][0] > 50 * seen[1][0]


# ------------------------------------------------------------------------------------------ b: resumed
@pytest.mark.parametrize("step0,hname", [(999, "torch"), (99999, "old"), (999, "far"), (99999, "loop")])
def test_resumed_steps(step0, hname):
    grp = Carved(of.MIXED, of.HYPERS[hname], values(of.MIXED, True), step0=step0)
    for it in range(2):
        grp.set_grads(of.grads(of.MIXED, it + 5))
        grp.step(f"resumed MIXED/{hname}", step0 + it + 1)


def test_second_step_norms_are_its_own():
    """Two steps with the same gradients: a running total would double sum g^2."""
    grp = Carved(of.MANY(257), of.HYPERS["loop"], values(of.MANY(257), False))
    grp.set_grads(of.grads(of.MANY(257), 1))
    _, _, first = grp.step("norms twice MANY257", 1)
    _, _, second = grp.step("norms twice MANY257", 2)
    assert first[0] == second[0] and abs(second[1] / first[1] - 1) < 1e-3


# ------------------------------------------------------------------------------------------ d: one layer, gradients in a bucket
def test_one_layer_with_bucket_gradients():
    grp = Carved(of.LAYER, of.HYPERS["loop"], values(of.LAYER, False), shapes=of.LAYER_SHAPES, bucket=True)
    assert [tuple(p.shape) for p in grp.params] == of.LAYER_SHAPES and of.nchunks(of.LAYER) == 40
    assert all(p.grad._is_view() and p.grad.is_contiguous() for p in grp.params)
    for it in range(2):
        grp.set_grads(of.grads(of.LAYER, it))
        grp.step("LAYER/loop", it + 1)


# ------------------------------------------------------------------------------------------ e: a tensor's bits and its company
X = 65537


def _x_values():
    g = np.random.default_rng([of.SEED, 77])
    return {"p": g.standard_normal(X).astype(np.float32), "g": g.standard_normal(X).astype(np.float32),
            "m": (g.standard_normal(X) * 1e-3).astype(np.float32), "v": (10.0 ** g.uniform(-22, -2, X)).astype(np.float32)}


def _run_with_company(layout, j, stream=None, nan_others=False):
    """One step at t = 42 of a carved group whose tensor j is the fixed 65537-element one -> (its p', m', v' bits, the norms)."""
    assert layout[j] == X
    vals, gs, x = values(layout, True, seed=5), of.grads(layout, 3, seed=5), _x_values()
    for k in "pmv":
        vals[k][j] = x[k]
    gs[j] = x["g"]
    if nan_others:
        gs = [g if i == j else np.full_like(g, np.nan) for i, g in enumerate(gs)]
    grp = Carved(layout, of.HYPERS["old"], vals, step0=41)
    grp.set_grads(gs)
    if stream is None:
        grp.opt.step()
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            grp.opt.step()
        torch.cuda.current_stream().wait_stream(stream)
        stream.synchronize()
    grp.gaps_intact()
    st = grp.opt.state[grp.params[j]]
    return [t.detach().cpu().clone() for t in (grp.params[j], st["exp_avg"], st["exp_avg_sq"])], grp.opt.last_sq_norms.cpu().clone()


@pytest.fixture(scope="module")
def alone():
    return _run_with_company([X], 0)


def test_alone_is_held_to_the_oracle(alone):
    x = _x_values()
    before = {k: [x[k]] for k in "pgmv"}
    after = {k: [t.numpy()] for k, t in zip("pmv", alone[0])}
    of.judge_step("alone t=42", before, after, of.HYPERS["old"], 42, TALLY)
    of.judge_norms("alone t=42", before["g"], before["p"], alone[1].numpy(), TALLY)


@pytest.mark.parametrize("where", ["first of EDGES", "last of 300"])
def test_bits_do_not_depend_on_the_company(alone, where):
    if where == "first of EDGES":
        layout, j = [X] + [n for n in of.EDGES if n != X], 0
    else:
        layout, j = of.MANY(299) + [X], 299
    assert len(layout) in (len(of.EDGES), 300)
    got, _ = _run_with_company(layout, j)
    assert all(torch.equal(a, b) for a, b in zip(got, alone[0]))


def test_bits_do_not_depend_on_the_stream_or_the_run(alone):
    again, norms = _run_with_company([X], 0)
    assert all(torch.equal(a, b) for a, b in zip(again, alone[0])) and torch.equal(norms, alone[1])
    side, norms = _run_with_company([X], 0, stream=torch.cuda.Stream(device=dev()))
    assert all(torch.equal(a, b) for a, b in zip(side, alone[0])) and torch.equal(norms, alone[1])
    layout = of.MANY(299) + [X]
    a, na = _run_with_company(layout, 299)
    b, nb = _run_with_company(layout, 299, stream=torch.cuda.Stream(device=dev()))
    assert all(torch.equal(s, t) for s, t in zip(a, b)) and torch.equal(na, nb) and bool(torch.isfinite(na).all())


def test_nan_in_the_neighbours_stays_with_the_neighbours(alone):
    layout = [n for n in of.EDGES if n != X][:4] + [X] + [n for n in of.EDGES if n != X][4:]
    got, norms = _run_with_company(layout, 4, nan_others=True)
    assert all(torch.equal(a, b) for a, b in zip(got, alone[0]))
    assert bool(torch.isnan(norms[0])) and bool(torch.isfinite(norms[1]))


# ------------------------------------------------------------------------------------------ f: the tables follow the tensors
F_LAYOUT = [70001, 3, 70001, 257, 1, 65536, 2, 5]                 # the two largest are of one size: their buffers can be swapped


def test_tables_follow_new_swapped_and_reloaded_tensors():
    from mst_amd.optim import FusedAdamW
    hyper = of.HYPERS["torch"]
    params = [up(p).requires_grad_(True) for p in of.params(F_LAYOUT)]
    idle = [up(p).requires_grad_(True) for p in of.params([4, 300, X], seed=6)]
    idle0 = [p.detach().clone() for p in idle]
    opt = FusedAdamW(params[:4] + idle[:2] + params[4:] + idle[2:], **hyper)
    for it in range(2):                                            # new gradient tensors every step; the state is created lazily
        for p, g in zip(params, of.grads(F_LAYOUT, it)):
            p.grad = up(g)
        judged_step("tables new grads", opt, params, it + 1)
    gs = of.grads(F_LAYOUT, 2)
    old0, old2 = params[0].grad, params[2].grad                    # the two largest trade buffers: the same addresses, permuted
    old2.copy_(up(gs[0]))
    old0.copy_(up(gs[2]))
    params[0].grad, params[2].grad = old2, old0
    for i in (1, 3, 4, 5, 6, 7):
        params[i].grad.copy_(up(gs[i]))
    judged_step("tables swapped grads", opt, params, 3)
    before = [opt.state[p]["exp_avg"].data_ptr() for p in params]
    opt.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert [opt.state[p]["exp_avg"].data_ptr() for p in params] != before
    for p, g in zip(params, of.grads(F_LAYOUT, 3)):
        p.grad.copy_(up(g))
    judged_step("tables reloaded state", opt, params, 4)
    for p, p0 in zip(idle, idle0):                                 # no gradient: untouched and without state, as with torch
        assert torch.equal(p.detach(), p0) and p.grad is None
        assert p not in opt.state or len(opt.state[p]) == 0
    assert len(opt.state_dict()["state"]) == len(F_LAYOUT)


# ------------------------------------------------------------------------------------------ g: a trajectory
def test_twelve_annealed_steps_against_torch_float64():
    from mst_amd.optim import FusedAdamW
    layout, hyper, steps, anneal = of.MIXED, of.HYPERS["torch"], 12, 16
    lrs = [hyper["lr"] * (1 - k / anneal) for k in range(steps)]   # TrainInpaintingLoop._anneal_lr at step k
    gs = [of.grads(layout, k) for k in range(steps)]
    m0, v0 = of.moments(layout, False)
    start = {"p": of.params(layout), "m": m0, "v": v0}
    want = of.torch_adamw(start, hyper, 0, torch.float64, n=steps, lrs=lrs, grads=gs)
    cur = start
    for k in range(steps):
        out = [of.adamw_step(p, g, m, v, dict(hyper, lr=lrs[k]), k + 1, np.float32) for p, g, m, v in zip(cur["p"], gs[k], cur["m"], cur["v"])]
        cur = {q: [o[j] for o in out] for j, q in enumerate("pmv")}
    params = [up(p).requires_grad_(True) for p in start["p"]]
    opt = FusedAdamW(params, **hyper)
    for k in range(steps):
        for group in opt.param_groups:
            group["lr"] = lrs[k]
        for p, g in zip(params, gs[k]):
            p.grad = up(g)
        opt.step()
    got = {"p": host(params), "m": host([opt.state[p]["exp_avg"] for p in params]), "v": host([opt.state[p]["exp_avg_sq"] for p in params])}
    for q in "pmv":
        for i, n in enumerate(layout):
            d32, d = of.distance(cur[q][i], want[q][i]), of.distance(got[q][i], want[q][i])
            b = of.bar(d32)
            TALLY.add("trajectory", f"12 steps {q} tensor {i} ({n})", d32, d, b)
            print(f"optim: 12 annealed steps {q} tensor {i} ({n}) restatement {d32:.3e} kernel {d:.3e} bar {b:.3e} ratio {d / b:.3f}")
            assert d <= b, (q, i, d32, d, b)


# ------------------------------------------------------------------------------------------ h: the trainer's norms
class _Small(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = np.random.default_rng([of.SEED, 8])
        mk = lambda shape, scale, grad=True: torch.nn.Parameter(up(g.standard_normal(shape) * scale), requires_grad=grad)
        self.frozen_a, self.w = mk((300,), 2.0, False), mk((70001,), 1.0)
        self.b, self.idle = mk((257,), 1e-3), mk((129,), 3.0)
        self.frozen_b, self.c = mk((7, 5), 0.5, False), mk((33, 3), 30.0)


def test_trainer_norms_with_frozen_and_idle_parameters(tmp_path):
    from mst_amd.diffusion import logger
    from mst_amd.diffusion.fp16_util import MixedPrecisionTrainer
    from mst_amd.optim import FusedAdamW
    logger.configure(dir=str(tmp_path))
    model = _Small()
    tr = MixedPrecisionTrainer(model=model)
    opt = FusedAdamW(tr.master_params, **of.HYPERS["loop"])
    stepped, rest = [model.w, model.b, model.c], [model.frozen_a, model.idle, model.frozen_b]
    idle0 = model.idle.detach().clone()
    for it in range(2):
        for p, g in zip(stepped, of.grads([p.numel() for p in stepped], it, seed=8)):
            p.grad = up(g).view_as(p)
        gs, ps, others = host([p.grad for p in stepped]), host(stepped), host(rest)
        assert tr.optimize(opt) is True
        g64, p64 = of.sq_norms(gs, ps, np.float64)
        g32, p32 = (float(x) for x in of.sq_norms(gs, ps, np.float32))
        p64 += sum(float((o.astype(np.float64) ** 2).sum()) for o in others)
        p32 += sum(float(np.sum(o * o, dtype=np.float32)) for o in others)       # the trainer's own float32 sums of the rest
        for name, got, r32, r64 in (("grad_norm", tr.last_norms[0], g32, g64), ("param_norm", tr.last_norms[1], p32, p64)):
            d32, d = of.distance(np.sqrt(r32), np.sqrt(r64)), of.distance(got, np.sqrt(r64))
            b = of.bar(d32)
            TALLY.add("norms", f"trainer {name} step {it + 1}", d32, d, b)
            print(f"optim: trainer {name} step {it + 1} restatement {d32:.3e} kernel {d:.3e} bar {b:.3e} ratio {d / b:.3f}")
            assert d <= b, (name, d32, d, b)
    assert torch.equal(model.idle.detach(), idle0) and model.idle.grad is None
    assert all(p not in opt.state or len(opt.state[p]) == 0 for p in rest)


# ------------------------------------------------------------------------------------------ i: a refused step changes nothing
def _pair():
    from mst_amd.optim import FusedAdamW
    layout = [5, 70001, 7, 300]
    mk = lambda: [up(p).requires_grad_(True) for p in of.params(layout, seed=4)]
    ps, qs = mk(), mk()
    return layout, ps, FusedAdamW(ps, **of.HYPERS["old"]), qs, FusedAdamW(qs, **of.HYPERS["old"])


def _give(layout, ps, qs, it):
    for p, q, g in zip(ps, qs, of.grads(layout, it, seed=4)):
        p.grad, q.grad = up(g), up(g)


def _state_bits(opt, ps):
    return [(p.detach().clone(), {k: v.clone() for k, v in opt.state[p].items()} if p in opt.state and len(opt.state[p]) else None)
            for p in ps]


def _unchanged(opt, ps, snap):
    for p, (p0, st0) in zip(ps, snap):
        assert torch.equal(p.detach(), p0)
        st = opt.state[p] if p in opt.state else {}
        if st0 is None:                                            # a state may have been created: zeros at step 0
            assert len(st) == 0 or (float(st["step"]) == 0.0 and not st["exp_avg"].any() and not st["exp_avg_sq"].any())
        else:
            assert all(torch.equal(st[k], st0[k]) for k in ("step", "exp_avg", "exp_avg_sq"))


def _same_bits(opt, ps, clean, qs):
    for p, q in zip(ps, qs):
        assert torch.equal(p.detach(), q.detach())
        assert all(torch.equal(opt.state[p][k], clean.state[q][k]) for k in ("step", "exp_avg", "exp_avg_sq"))
    assert torch.equal(opt.last_sq_norms, clean.last_sq_norms)


@pytest.mark.parametrize("warm", [0, 2])
def test_a_step_refused_for_a_strided_gradient_changes_nothing(warm):
    layout, ps, opt, qs, clean = _pair()
    for it in range(warm):
        _give(layout, ps, qs, it)
        opt.step()
        clean.step()
    _give(layout, ps, qs, warm)
    good = ps[-1].grad
    ps[-1].grad = good.repeat_interleave(2)[::2]
    assert not ps[-1].grad.is_contiguous() and torch.equal(ps[-1].grad, good)
    snap = _state_bits(opt, ps)
    with pytest.raises(RuntimeError, match="contiguous"):
        opt.step()
    _unchanged(opt, ps, snap)
    ps[-1].grad = ps[-1].grad.contiguous()
    opt.step()
    clean.step()
    _same_bits(opt, ps, clean, qs)
    assert int(opt.state[ps[0]]["step"]) == warm + 1


def test_a_step_refused_for_unequal_step_counts_changes_nothing():
    layout, ps, opt, qs, clean = _pair()
    _give(layout, ps, qs, 0)
    opt.step()
    clean.step()
    _give(layout, ps, qs, 1)
    opt.state[ps[-1]]["step"] += 5
    snap = _state_bits(opt, ps)
    for _ in range(2):
        with pytest.raises(RuntimeError, match="share their step count"):
            opt.step()
        _unchanged(opt, ps, snap)
    opt.state[ps[-1]]["step"] -= 5
    opt.step()
    clean.step()
    _same_bits(opt, ps, clean, qs)
    assert int(opt.state[ps[0]]["step"]) == 2


# ------------------------------------------------------------------------------------------ the file's summary
def test_worst_ratio_over_the_file():
    for line in TALLY.lines():
        print(line)
    print(f"optim: {TALLY.widened} of {TALLY.updates} update comparisons passed by the fixture's widening alone, "
          f"on tensors of up to {TALLY.widened_numel} elements")
    print(f"optim: worst ratio to the bar over the file {TALLY.worst_ratio():.3f}")
    assert TALLY.worst_ratio() <= 1.0
