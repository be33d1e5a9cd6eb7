"""tests/optim_fixture.py without a GPU: the float64 oracle against torch.optim.AdamW in float64, the float32 restatement and
torch's own float32 AdamW against the oracle under the suite's bar, the per-element bound on v', the norm restatement, `carve`,
the refused step of `FusedAdamW` (host code, run against a stub of the library that computes), and the four kernel mutations
the GPU tests are meant to catch, carried by the restatement through the same judge.

The per-element bound on v' = beta2 v + (1 - beta2) g g: two rounded products in the gradient term, one in beta2 v, one rounded
sum of positive terms -- every rounding is relative to a value no larger than the result, so the result is within 3 unit
roundoffs (2^-24 each) to first order and fewer under a fused multiply-add; the bound is 4.  Measured here: 2.69 x 2^-24 over
400 000 log-uniform elements."""
import ctypes as C

import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
import lib_stub
import optim_fixture as of
from mst_amd import optim as O

COVER = [1, 3, 255, 257, 1000, 4099, 7, 513, 2, 65537, 31, 64, 5, 300, 129, 70001]     # every (parameter, gradient) class pairing


torch_step = of.torch_adamw


def case(layout, resumed, it=0, scale=1.0):
    m, v = of.moments(layout, resumed)
    return {"p": of.params(layout), "g": of.grads(layout, it, scale), "m": m, "v": v}


# ------------------------------------------------------------------------------------------ the oracle is torch's AdamW
@pytest.mark.parametrize("name", list(of.HYPERS))
def test_oracle_equals_torch_float64(name):
    hyper = of.HYPERS[name]
    for resumed, step0 in ((False, 0), (True, 999)):
        cur = case(COVER, resumed)
        for k in range(3 if not resumed else 1):
            cur["g"] = of.grads(COVER, k, 10.0 ** (k - 1))
            want = torch_step(cur, hyper, step0 + k, torch.float64)
            got = [of.adamw_step(p, g, m, v, hyper, step0 + k + 1, np.float64) for p, g, m, v in zip(*(cur[q] for q in "pgmv"))]
            for i in range(len(COVER)):
                for j, q in enumerate("pmv"):
                    d = of.distance(got[i][j], want[q][i])
                    assert d <= 1e-13, (name, resumed, k, i, q, d)
            cur = {"p": want["p"], "m": want["m"], "v": want["v"]}       # float64 from here on: the next step reads them as they are


@pytest.mark.parametrize("resumed", [False, True])
@pytest.mark.parametrize("name", list(of.HYPERS))
def test_restatement_and_torch_float32_are_within_the_bar(name, resumed, capsys):
    hyper, step0 = of.HYPERS[name], 999 if resumed else 0
    before = case(COVER, resumed)
    want32 = torch_step(before, hyper, step0, torch.float32)
    tally = of.judge_step(f"cpu torch-f32 {name} resumed={resumed}", before, want32, hyper, step0 + 1)
    assert set(tally.worst) == {"update/" + n for n in of.P_NAMES} | {"m", "v", "v per element"}
    own = {q: [of.adamw_step(p, g, m, v, hyper, step0 + 1, np.float32)[j] for p, g, m, v in zip(*(before[k] for k in "pgmv"))]
           for j, q in enumerate("pmv")}
    of.judge_step(f"cpu restatement {name} resumed={resumed}", before, own, hyper, step0 + 1)


def test_value_classes():
    p, g = of.params(COVER), of.grads(COVER)
    pairs = {(of.p_class(i), of.g_class(i)) for i in range(len(COVER))}
    assert len(pairs) == 16
    for i in range(len(COVER)):
        assert (not p[i].any()) == (of.p_class(i) == 0)
        if of.g_class(i) >= 2:
            assert not g[i][::3].any() and (COVER[i] < 2 or g[i][1::3].all())
        if of.g_class(i) % 2 == 1:
            mag = np.abs(g[i][g[i] != 0])
            assert mag.size == 0 or (mag.min() >= 0.99e-12 and mag.max() <= 1.01e-2)
    big = np.abs(np.concatenate([x for i, x in enumerate(g) if of.g_class(i) % 2 == 1]))
    assert (big[big > 0] < 1e-8).any() and (big > 1e-8).any()            # both sides of eps
    m, v = of.moments(COVER, True)
    assert min(x.min() for x in v) >= 0.99e-22 and max(x.max() for x in v) <= 1.01e-2
    assert not any(x.any() for pair in of.moments(COVER, False) for x in pair)


@pytest.mark.parametrize("b2", [0.9, 0.98, 0.999])
def test_second_moment_per_element_bound(b2):
    g = np.random.default_rng([of.SEED, 9])
    n = 400_000
    v = (10.0 ** g.uniform(-22, -2, n)).astype(np.float32)
    gr = (np.where(g.integers(0, 2, n) == 0, -1.0, 1.0) * 10.0 ** g.uniform(-12, -2, n)).astype(np.float32)
    hyper = dict(of.HYPERS["torch"], betas=(0.9, b2))
    z = np.zeros(n, np.float32)
    v64 = of.adamw_step(z, gr, z, v, hyper, 5, np.float64)[2]
    v32 = of.adamw_step(z, gr, z, v, hyper, 5, np.float32)[2]
    big = v64 >= of.V_ELEM_MIN
    assert big.sum() > 0.99 * n
    rel = np.abs(v32.astype(np.float64) - v64)[big] / v64[big]
    print(f"optim: v per element b2={b2} worst {rel.max() / 2.0 ** -24:.3f} x 2^-24")
    assert rel.max() <= of.V_ELEM_BAR


# ------------------------------------------------------------------------------------------ norms and layouts
LAYOUTS = {"EDGES": of.EDGES, "MIXED": of.MIXED, "LAYER": of.LAYER, **{f"MANY{k}": of.MANY(k) for k in (255, 256, 257, 300)}}


def test_layouts():
    assert of.EDGES == [1, 255, 256, 257, 65535, 65536, 65537, 131072, 131073]
    assert of.MIXED == [3, 196613, 1, 65536, 2, 131072, 70001]
    assert sum(of.LAYER) == 2_102_784 and of.nchunks(of.LAYER) == 40 and len(of.LAYER) == 12
    layer = torch.nn.TransformerEncoderLayer(d_model=512, nhead=4, dim_feedforward=1024)
    assert [tuple(p.shape) for p in layer.parameters()] == of.LAYER_SHAPES
    assert [of.nchunks(of.MANY(k)) for k in (255, 256, 257, 300)] == [255, 256, 257, 300]
    assert of.MANY(9) == [1, 2, 3, 4, 5, 6, 7, 1, 2]
    assert of.nchunks(of.EDGES) == 13 and of.nchunks(of.MIXED) == 4 + 1 + 1 + 1 + 1 + 2 + 2


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_norm_restatement_is_within_the_bar(name):
    layout = LAYOUTS[name]
    gs, ps = of.grads(layout), of.params(layout)
    n64, n32 = of.sq_norms(gs, ps, np.float64), of.sq_norms(gs, ps, np.float32)
    assert all(x.dtype == np.float32 for x in n32)
    for k in range(2):
        d = of.distance(float(n32[k]), n64[k])
        print(f"optim: norm restatement {name} [{k}] {d:.3e}")
        assert d <= of.bar(0.0)                                   # its own bar is the floor: it must not need more
    # the order is the kernels': a plain float32 running sum of the same squares is a different number on the large layouts
    if name == "LAYER":
        run = np.float32(0.0)
        for x in gs:
            run = np.float32(run + np.cumsum(x * x, dtype=np.float32)[-1])
        assert run != n32[0]


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_carve(name):
    layout = LAYOUTS[name]
    flat, slices = of.carve(layout, fill=of.GAP_FILL)
    assert flat.dtype == np.float32 and flat.size == sum(layout) + 3 * (len(layout) + 1)
    assert [s.stop - s.start for s in slices] == layout
    assert slices[0].start == 3 and flat.size - slices[-1].stop == 3
    assert all(b.start - a.stop == 3 for a, b in zip(slices, slices[1:]))            # no overlap, the gap between neighbours
    gaps = of.gap_mask(flat.size, slices)
    assert gaps.sum() == 3 * (len(layout) + 1)
    assert (flat.view(np.int32)[gaps] == of.GAP_BITS).all() and (flat.view(np.int32)[~gaps] == of.GAP_BITS).all()
    t = torch.from_numpy(flat)
    views = [t[s] for s in slices]
    assert any((s.start * 4) % 16 for s in slices)
    assert all(v.is_contiguous() and v.data_ptr() == t.data_ptr() + 4 * s.start for v, s in zip(views, slices))
    nan, _ = of.carve(layout, fill=np.nan)
    assert np.isnan(nan[gaps]).all()


# ------------------------------------------------------------------------------------------ a refused step changes nothing
class ComputingLib(lib_stub.RecordingLib):
    """The recording stub with an `mst_adamw_step` that does the float32 restatement on the host memory it is given."""

    def mst_adamw_workspace_bytes(self, n, numel):
        return 64

    def mst_adamw_step(self, n, ps, gs, ms, vs, numel, lr, b1, b2, eps, wd, step, norms, ws, ws_bytes, upload, stream):
        self.calls.append(("mst_adamw_step", (n, step, upload)))
        hyper = dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
        at = lambda a, i: np.ctypeslib.as_array((C.c_float * numel[i]).from_address(a[i]))
        for i in range(n):
            p, m, v = at(ps, i), at(ms, i), at(vs, i)
            p[:], m[:], v[:] = of.adamw_step(p.copy(), at(gs, i).copy(), m.copy(), v.copy(), hyper, step, np.float32)
        return 0


def _stub(monkeypatch):
    lib_stub.install(monkeypatch)
    lib = ComputingLib()
    monkeypatch.setattr(lib_stub.N, "lib", lambda: lib)
    monkeypatch.setattr(O, "_need_gpu", lambda dev: None)
    return lib


def _optimizer():
    layout = [5, 300, 7, 12]
    ps = [torch.from_numpy(p.copy()).requires_grad_(True) for p in of.params(layout, seed=4)]
    for p, g in zip(ps, of.grads(layout, seed=4)):
        p.grad = torch.from_numpy(g.copy())
    return ps, O.FusedAdamW(ps, **of.HYPERS["old"])


def _snapshot(opt, ps):
    return [(p.detach().clone(), {k: v.clone() for k, v in opt.state[p].items()} if p in opt.state else None) for p in ps]


def _unchanged(opt, ps, snap):
    for p, (p0, st0) in zip(ps, snap):
        assert torch.equal(p.detach(), p0)
        if st0 is None:                                            # a state may have been created: zeros at step 0
            st = opt.state.get(p)
            assert st is None or len(st) == 0 or (float(st["step"]) == 0.0 and not st["exp_avg"].any() and not st["exp_avg_sq"].any())
        else:
            assert float(opt.state[p]["step"]) == float(st0["step"])
            assert torch.equal(opt.state[p]["exp_avg"], st0["exp_avg"]) and torch.equal(opt.state[p]["exp_avg_sq"], st0["exp_avg_sq"])


def _same_bits(opt_a, ps_a, opt_b, ps_b):
    for p, q in zip(ps_a, ps_b):
        assert torch.equal(p.detach(), q.detach())
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(opt_a.state[p][k], opt_b.state[q][k])


@pytest.mark.parametrize("warm", [0, 2])
def test_a_step_refused_for_a_strided_gradient_changes_nothing(monkeypatch, warm):
    lib = _stub(monkeypatch)
    (ps, opt), (qs, clean) = _optimizer(), _optimizer()
    for _ in range(warm):
        opt.step()
        clean.step()
    good = ps[-1].grad
    ps[-1].grad = torch.from_numpy(np.repeat(good.numpy(), 2))[::2]            # the same values, stride 2
    assert not ps[-1].grad.is_contiguous() and torch.equal(ps[-1].grad, good)
    snap, calls = _snapshot(opt, ps), len(lib.calls)
    with pytest.raises(RuntimeError, match="contiguous"):
        opt.step()
    assert len(lib.calls) == calls
    _unchanged(opt, ps, snap)
    ps[-1].grad = ps[-1].grad.contiguous()
    opt.step()
    clean.step()
    assert lib.calls[-1][1][1] == warm + 1
    _same_bits(opt, ps, clean, qs)


@pytest.mark.parametrize("warm", [1, 3])
def test_a_step_refused_for_unequal_step_counts_changes_nothing(monkeypatch, warm):
    lib = _stub(monkeypatch)
    (ps, opt), (qs, clean) = _optimizer(), _optimizer()
    for _ in range(warm):
        opt.step()
        clean.step()
    opt.state[ps[-1]]["step"] += 5
    snap, calls = _snapshot(opt, ps), len(lib.calls)
    for _ in range(2):                                             # refused again for the same reason, not for a new one
        with pytest.raises(RuntimeError, match="share their step count"):
            opt.step()
        assert len(lib.calls) == calls
        _unchanged(opt, ps, snap)
    opt.state[ps[-1]]["step"] -= 5
    opt.step()
    clean.step()
    assert lib.calls[-1][1][1] == warm + 1
    _same_bits(opt, ps, clean, qs)


def test_a_step_refused_for_a_wrong_dtype_changes_nothing(monkeypatch):
    _stub(monkeypatch)
    ps, opt = _optimizer()
    opt.step()
    ps[2].data = ps[2].data.double()
    ps[2].grad = ps[2].grad.double()
    snap = _snapshot(opt, ps)
    with pytest.raises(RuntimeError, match="float32"):
        opt.step()
    _unchanged(opt, ps, snap)


# ------------------------------------------------------------------------------------------ what the GPU tests would catch
def _run_emulated(layout, hyper, step, mutate, resumed=False):
    """One emulated launch on carved buffers, judged exactly as tests/test_gpu_optim.py judges the kernel."""
    vals = case(layout, resumed)
    flats, slices = {}, None
    for k, fill in (("p", of.GAP_FILL), ("g", np.nan), ("m", of.GAP_FILL), ("v", of.GAP_FILL)):
        flats[k], slices = of.carve(layout, fill=fill)
        for s, x in zip(slices, vals[k]):
            flats[k][s] = x
    norms = of.emulate(flats, slices, hyper, step, mutate)
    gaps = of.gap_mask(flats["p"].size, slices)
    quiet = lambda s: None
    of.judge_step("emulated", vals, {k: [flats[k][s] for s in slices] for k in "pmv"}, hyper, step, out=quiet)
    of.judge_norms("emulated", vals["g"], vals["p"], norms, out=quiet)
    for k in "pmv":
        assert (flats[k].view(np.int32)[gaps] == of.GAP_BITS).all(), "a gap was written"


@pytest.mark.parametrize("layout", ["EDGES", "MIXED", "MANY256", "MANY257"])
def test_the_emulated_launch_passes_the_judge(layout):
    _run_emulated(LAYOUTS[layout], of.HYPERS["torch"], 1, ())
    _run_emulated(LAYOUTS[layout], of.HYPERS["far"], 1000, (), resumed=True)


@pytest.mark.parametrize("mutate,layout,name,resumed", [
    ("no_eps", "EDGES", "torch", False), ("no_eps", "MIXED", "loop", True),
    ("beta1_for_beta2", "EDGES", "torch", False), ("beta1_for_beta2", "MIXED", "old", True),
    ("unclamped", "EDGES", "torch", False), ("unclamped", "MANY255", "loop", False),
    ("stride255", "MANY256", "torch", False), ("stride255", "MANY257", "old", False), ("stride255", "MANY300", "far", False)])
def test_a_mutated_launch_fails_the_judge(mutate, layout, name, resumed):
    with pytest.raises(AssertionError):
        _run_emulated(LAYOUTS[layout], of.HYPERS[name], 1000 if resumed else 1, (mutate,), resumed)


def test_the_stride_mutation_is_invisible_below_256_chunks():
    """Why MANY(256) and MANY(257) are in the GPU file: at 255 chunks a thread stride of 255 sums the same partials."""
    _run_emulated(LAYOUTS["MANY255"], of.HYPERS["torch"], 1, ("stride255",))
