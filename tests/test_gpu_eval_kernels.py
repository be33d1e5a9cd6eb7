"""The `mst_eval_*` entry points (csrc/mst_eval.h: gemm in its plain and conv roles, gru, layernorm, dist_rank, cov, pair_norms) called
one by one through `_native`, each against the float64 numpy evaluation of the same operation (tests/eval_kernel_cases.py over
tests/eval_fixture.py; the cases themselves are held by tests/test_eval_kernels_cpu.py).  tests/test_gpu_evaluator.py reaches these
kernels only through the assembled networks; here they get the arguments the wrapper never passes: leading dimensions above their
minimum, a null bias, `add` with `leaky`, LayerNorm without `leaky` and at any width, the affine on the rows layout, a batch stride
above its minimum, positions > max_steps, clamped step counts, distance matrices beyond one trip of the rank count, exact ties,
`cov = None`, and NaN / inf as data.

Every case prints `eval: <case> ref <fp32 restatement's distance> got <the kernel's> bar <bar>`, distances as eval_fixture.relmax.

  * GEMM, plain and conv prologues: element-wise |got - f64| <= (K + 4) 2^-24 (|A| |W|^T + |bias| + |add|), K + 6 and
    |A| = |x scale| + |shift| with the affine -- derived, for any order of a K-term fp32 sum.  `bar` prints that bound at its largest
    in relmax units, `used` the largest fraction of it an element takes.  Every element that must not be read is NaN, every element
    that must not be written a sentinel.
  * LayerNorm, GRU, real-valued distances: eval_fixture.bar of the restatement's own distance (4 x, floor 1e-6).
  * Integer distances and pair norms: the fp32 radicand is exact, the result within 1 ulp of np.sqrt, the rank the integer count.
  * Pair norms of normals: relative error at most (d + 4) 2^-24.
  * Non-finite inputs: a NaN or inf embedding row gives non-finite distances and rank n2, never a hit; everything else keeps its bits.

Measured on an MI355X (fp32 restatement / kernel, both against float64, relmax): GEMM 2.6e-8 .. 3.2e-7 / 2.6e-8 .. 2.1e-7, at most
0.26 of the bound used; conv prologues 2.9e-8 .. 2.7e-7 / 2.9e-8 .. 2.4e-7, at most 0.26 of the bound; LayerNorm at most 1.6e-7 /
1.6e-7 but for five rows of width 2 (1.0e-6 / 1.0e-6, bar 4e-6) and the rows at mean 100 (3.6e-6 / 4.6e-6, bar 1.4e-5: 0.32 of it, the
closest approach of a 4 x bar in this file); GRU 8.4e-8 .. 2.2e-7 / 5.0e-8 .. 1.3e-7 against the 1e-6 floor; real-valued distances
1.2e-7 / 1.2e-7; integer distances and pair norms equal to np.sqrt of the exact radicand; pair norms of normals at most 1.0e-7 / 9.2e-8
against bounds from 3.0e-7.  Worst kernel / fp32 ratio (reported, not asserted): GEMM 1.98 (m130_n1_k70), conv 3.33 (t4_c12_b3_n16,
1.5e-7 against 4.6e-8, at 0.03 of its bound), LayerNorm 1.34, GRU 1.15, distances 1.00, pair norms 2.03.  With the parent's kernel
(`rad > 0 ? rad : 0`) the three non-finite distance / rank tests fail -- the row of distances is 0 and the row ranks first -- and every
other test passes.  The file takes 3 s (213 tests)."""
import numpy as np
import pytest
import torch

import eval_fixture as ef
import eval_kernel_cases as kc
import mst_amd  # noqa: F401
from mst_amd import _native as N
from mst_amd.data_loaders import evaluator_wrapper as ew
from mst_amd.utils import metrics as mt

pytestmark = pytest.mark.gpu
SENT = float(kc.SENTINEL)
WORST = {}                                                               # group -> (kernel / fp32 ratio, case), reported, not asserted


def dev():
    return torch.device("cuda")


def cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def host(t):
    return t.detach().cpu().numpy()


def stream():
    return N.stream_ptr(dev())


def name_of(case):
    return case["name"]


def note(group, tag, ref, got):
    if ref > 0 and got / ref > WORST.get(group, (0.0, ""))[0]:
        WORST[group] = (got / ref, tag)


def held(group, tag, got, f32, f64):
    """eval_fixture.bar of the restatement's own distance."""
    ref, d = ef.relmax(f32, f64), ef.relmax(got, f64)
    b = ef.bar(ref)
    print(f"eval: {tag} ref {ref:.3e} got {d:.3e} bar {b:.3e}")
    note(group, tag, ref, d)
    assert np.isfinite(got).all()
    assert d <= b, (tag, d, b)


def bounded(group, tag, got, f32, f64, bound):
    """Element-wise inside a derived bound."""
    ref, d = ef.relmax(f32, f64), ef.relmax(got, f64)
    err = np.abs(got.astype(np.float64) - f64)
    used = float((err / bound).max())
    print(f"eval: {tag} ref {ref:.3e} got {d:.3e} bar {bound.max() / np.abs(f64).max():.3e} used {used:.3f}")
    note(group, tag, ref, d)
    assert np.isfinite(got).all()
    assert (err <= bound).all(), (tag, used)


def untouched(buf, rows, cols):
    """Everything of buf [R, ld] outside [:rows, :cols] still holds the sentinel."""
    return np.array_equal(buf[:rows, cols:], np.full_like(buf[:rows, cols:], SENT)) and np.array_equal(buf[rows:], np.full_like(buf[rows:], SENT))


# ------------------------------------------------------------------------------------------ mst_eval_gemm
def gemm(a, w, bias, add, M, Nn, K, lda, ldc, ldadd, leaky, mode=0, batch=0, frames=0, channels=0, ldx=0, sb=0, scale=None, shift=None):
    """-> the whole C buffer [M + 2, ldc], sentinel-filled before the call."""
    c = torch.full((M + 2, ldc), SENT, dtype=torch.float32, device=dev())
    N.check(N.lib().mst_eval_gemm(N.ptr(a), N.ptr(w), N.ptr(bias), N.ptr(add), N.ptr(c), M, Nn, K, lda, ldc, ldadd, mode, batch, frames,
                                  channels, ldx, sb, N.ptr(scale), N.ptr(shift), int(leaky), stream()))
    return host(c)


@pytest.mark.parametrize("case", kc.gemm_cases(), ids=name_of)
def test_gemm_plain(case):
    d, M, Nn, K = kc.gemm_data(case), case["M"], case["N"], case["K"]
    out = gemm(cu(d["a"]), cu(d["w"]), cu(d["bias"]), cu(d["add"]), M, Nn, K, d["lda"], d["ldc"], d["ldadd"] if case["add"] else 0, case["leaky"])
    assert untouched(out, M, Nn)
    tag = "gemm {name} bias {bias:d} add {add:d} leaky {leaky:d} padded {padded:d}".format(**case)
    bounded("gemm", tag, out[:M, :Nn], kc.gemm_ref(case, np.float32), kc.gemm_ref(case, np.float64), kc.gemm_bound(case))


@pytest.mark.parametrize("case", kc.conv_cases(), ids=name_of)
def test_gemm_conv_prologues(case):
    """Modes 1 (rows, ldx = channels + 4) and 2 (a sample), the batch stride 11 floats above its minimum with NaN in the gap, with and
    without the affine; mode 2 gives mode 1's bits."""
    d, B, T, C, Nn = kc.conv_data(case), case["B"], case["T"], case["C"], case["N"]
    M, K = B * ef.conv_frames(T), 4 * C
    w, bias, scale, shift = cu(d["wk"]), cu(d["bias"]), cu(d["scale"]), cu(d["shift"])
    for affine in (False, True):
        got = {}
        for mode, buf in ((1, d["rows"]), (2, d["sample"])):
            out = gemm(cu(buf), w, bias, None, M, Nn, K, K, Nn + 3, 0, 1, mode=mode, batch=B, frames=T, channels=C, ldx=d["F"], sb=d["sb"],
                       scale=scale if affine else None, shift=shift if affine else None)
            assert untouched(out, M, Nn)
            got[mode] = out[:M, :Nn]
            bounded("conv", f"conv {case['name']} mode {mode} affine {affine:d}", got[mode], kc.conv_ref(case, affine, np.float32),
                    kc.conv_ref(case, affine, np.float64), kc.conv_bound(case, affine))
        assert np.array_equal(got[1], got[2])                            # the same numbers read in the same order


# ------------------------------------------------------------------------------------------ mst_eval_layernorm
@pytest.mark.parametrize("case", kc.ln_cases(), ids=name_of)
def test_layernorm(case):
    d, R, W = kc.ln_data(case), case["R"], case["W"]
    y = torch.full((R + 1, W), SENT, dtype=torch.float32, device=dev())
    x, gamma, beta = cu(d["x"]), cu(d["gamma"]), cu(d["beta"])           # held: a tensor must outlive the call that gets its pointer
    N.check(N.lib().mst_eval_layernorm(N.ptr(x), N.ptr(gamma), N.ptr(beta), N.ptr(y), R, W, kc.LN_EPS, case["leaky"], stream()))
    out = host(y)
    assert untouched(out, R, W)
    got = out[:R]
    held("layernorm", "layernorm " + case["name"], got, kc.ln_ref(case, np.float32), kc.ln_ref(case, np.float64))
    beta = ef.leaky(d["beta"]) if case["leaky"] else d["beta"]           # float32: 0.2f * beta, the kernel's own product
    if W == 1:                                                           # x - mean = 0 exactly
        assert np.array_equal(got, np.broadcast_to(beta, got.shape))
    if case["kind"] == "constant":                                       # variance 0: 0 / sqrt(eps)
        assert np.isfinite(got[0]).all() and np.array_equal(got[0], beta)


# ------------------------------------------------------------------------------------------ mst_eval_gru
def gru(case, steps=None, max_steps=None):
    """-> out [B, 2 H]; the row after it and both halves of `work` start as sentinel / NaN."""
    H, B = case["H"], case["B"]
    xproj, steps = kc.gru_data(case, steps)
    sd = kc.gru_state(H)
    w_hh = cu(np.stack([sd["gru.weight_hh_l0"], sd["gru.weight_hh_l0_reverse"]]))
    b_hh = cu(np.stack([sd["gru.bias_hh_l0"], sd["gru.bias_hh_l0_reverse"]]))
    hidden = cu(sd["hidden"].reshape(2, H))
    work = torch.full((2, B, 2 * H), float("nan"), dtype=torch.float32, device=dev())
    out = torch.full((B + 1, 2 * H), SENT, dtype=torch.float32, device=dev())
    xp, st = cu(xproj), cu(steps)
    N.check(N.lib().mst_eval_gru(N.ptr(xp), N.ptr(w_hh), N.ptr(b_hh), N.ptr(hidden), N.ptr(st), B, kc.GRU_POSITIONS, H,
                                 case["S"] if max_steps is None else max_steps, N.ptr(work), N.ptr(out), stream()))
    res = host(out)
    assert untouched(res, B, 2 * H)
    return res[:B]


@pytest.mark.parametrize("case", kc.gru_cases(), ids=name_of)
def test_gru(case):
    """positions 6 >= max_steps: both parities of the ping-pong, the direct write at one step, mixed step counts, NaN projections at
    every position its clip does not reach."""
    held("gru", "gru " + case["name"], gru(case), kc.gru_ref(case, np.float32), kc.gru_ref(case, np.float64))


@pytest.mark.parametrize("H", kc.GRU_H)
def test_gru_clamps_its_step_counts(H):
    case = dict(H=H, B=17, S=kc.GRU_POSITIONS)
    plain = kc.gru_steps(17, kc.GRU_POSITIONS)
    steps = plain.copy()
    steps[[0, 16]], steps[[3, 5]] = (0, -2), (7, 1 << 20)                # none, a negative count; beyond `positions`
    got = gru(case, steps)
    init = kc.gru_state(H)["hidden"].reshape(2 * H)
    assert np.array_equal(got[0], init) and np.array_equal(got[16], init)            # the initial state, bit for bit
    as_positions = np.clip(steps, 0, kc.GRU_POSITIONS)
    assert np.array_equal(got, gru(case, as_positions))
    held("gru", f"gru clamps h{H}", got, kc.gru_ref(case, np.float32, steps), kc.gru_ref(case, np.float64, steps))
    assert np.array_equal(np.delete(got, [0, 3, 5, 16], 0), np.delete(gru(case, plain), [0, 3, 5, 16], 0))      # the others do not notice


# ------------------------------------------------------------------------------------------ mst_eval_dist_rank
def dist_rank(e1, e2, want_rank):
    n1, n2, d = e1.shape[0], e2.shape[0], e1.shape[1]
    dist = torch.full((n1 + 1, n2), SENT, dtype=torch.float32, device=dev())
    rank = torch.full((n1 + 1,), -7, dtype=torch.int32, device=dev()) if want_rank else None
    a, b = cu(e1), cu(e2)
    N.check(N.lib().mst_eval_dist_rank(N.ptr(a), N.ptr(b), n1, n2, d, N.ptr(dist), N.ptr(rank), stream()))
    out = host(dist)
    assert untouched(out, n1, n2)
    if want_rank:
        assert host(rank)[n1] == -7
    return out[:n1], host(rank)[:n1] if want_rank else None


def one_ulp(got, want):
    return (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(want)).all()


@pytest.mark.parametrize("shape", [(n, n, d) for n, d in kc.DIST_SQUARE] + list(kc.DIST_RECT), ids=str)
def test_dist_rank_on_integers_is_exact(shape):
    n1, n2, d = shape
    e1, e2 = kc.dist_int_case(n1, n2, d)
    rad = kc.radicands(e1, e2)
    got, rank = dist_rank(e1, e2, n1 == n2)
    want = np.sqrt(rad.astype(np.float32))
    f64 = np.sqrt(rad.astype(np.float64))
    print(f"eval: dist int {shape} ref {ef.relmax(want, f64):.3e} got {ef.relmax(got, f64):.3e} bar {2.0 ** -23:.3e}")
    assert one_ulp(got, want)
    if n1 == n2:
        assert np.array_equal(rank, kc.integer_ranks(rad))
        assert np.array_equal(host(mt.diagonal_ranks(cu(e1), cu(e2))), rank)
    if n1 > 1:
        same, _ = dist_rank(e1, e1, False)                               # against itself: finite, >= 0, the diagonal 0
        assert np.isfinite(same).all() and (same >= 0).all() and (np.diag(same) == 0).all()


@pytest.mark.parametrize("shape", kc.DIST_REAL, ids=str)
def test_dist_on_normals(shape):
    e1, e2 = kc.dist_real_case(*shape)
    got, rank = dist_rank(e1, e2, shape[0] == shape[1])
    held("dist", f"dist {shape}", got, ef.euclidean_distance_matrix(e1, e2, np.float32), ef.euclidean_distance_matrix(e1, e2, np.float64))
    if rank is not None:
        assert np.array_equal(rank, (got < np.diag(got)[:, None]).sum(1))             # the count over the matrix it wrote


# ------------------------------------------------------------------------------------------ mst_eval_pair_norms
def pair_norms(a, b, ia, ib):
    out = torch.full((len(ia) + 1,), SENT, dtype=torch.float32, device=dev())
    da, db, dia, dib = cu(a), cu(b), cu(np.asarray(ia, np.int32)), cu(np.asarray(ib, np.int32))
    N.check(N.lib().mst_eval_pair_norms(N.ptr(da), N.ptr(db), N.ptr(dia), N.ptr(dib), len(ia), a.shape[0], b.shape[0], a.shape[1], N.ptr(out),
                                        stream()))
    res = host(out)
    assert res[len(ia)] == kc.SENTINEL
    return res[:len(ia)]


@pytest.mark.parametrize("case", kc.pair_cases(), ids=name_of)
def test_pair_norms(case):
    a, b, ia, ib = kc.pair_data(case)
    got = pair_norms(a, b, ia, ib)
    f32, f64 = kc.pair_ref(case, np.float32), kc.pair_ref(case, np.float64)
    bound = (case["d"] + 4) * kc.EPS32
    rel = np.abs(got - f64) / np.maximum(f64, 1e-300)
    print(f"eval: pair {case['name']} ref {ef.relmax(f32, f64):.3e} got {ef.relmax(got, f64):.3e} bar {bound:.3e}")
    note("pair", case["name"], ef.relmax(f32, f64), ef.relmax(got, f64))
    if case["kind"] == "int":
        assert one_ulp(got, np.sqrt((f64 ** 2).round().astype(np.float32)))
    else:
        assert (rel <= bound).all(), (case["name"], rel.max(), bound)


def test_pair_norms_index_outside_its_matrix_is_nan():
    case = dict(d=65, pairs=9, kind="normal")
    a, b, ia, ib = kc.pair_data(case)
    base = pair_norms(a, b, ia, ib)
    for slot, (da, db) in ((2, (-1, None)), (0, (kc.PAIR_NA, None)), (8, (None, kc.PAIR_NB)), (5, (None, -1)), (4, (-(1 << 31), 1 << 30))):
        ja, jb = ia.copy(), ib.copy()
        if da is not None:
            ja[slot] = da
        if db is not None:
            jb[slot] = db
        got = pair_norms(a, b, ja, jb)
        assert np.isnan(got[slot]) and np.array_equal(np.delete(got, slot), np.delete(base, slot))


# ------------------------------------------------------------------------------------------ mst_eval_cov
@pytest.mark.parametrize("d", kc.COV_D)
@pytest.mark.parametrize("n", kc.COV_N)
def test_cov_none_gives_the_mean_alone(n, d):
    rows = kc.cov_rows(n, d)
    a = cu(rows)
    buf = torch.full((d + d * d,), SENT, dtype=torch.float64, device=dev())       # the mean, then where a covariance would follow
    N.check(N.lib().mst_eval_cov(N.ptr(a), n, d, N.ptr(buf), None, stream()))
    res = host(buf)
    assert np.array_equal(res[d:], np.full(d * d, SENT))
    if n >= 2:
        mu, cov = torch.empty(d, dtype=torch.float64, device=dev()), torch.empty(d, d, dtype=torch.float64, device=dev())
        N.check(N.lib().mst_eval_cov(N.ptr(a), n, d, N.ptr(mu), N.ptr(cov), stream()))
        assert np.array_equal(res[:d], host(mu))
    else:
        assert np.array_equal(res[:d], rows[0].astype(np.float64))
    mu64 = rows.astype(np.float64).mean(0)
    assert (np.abs(res[:d] - mu64) <= 2.0 ** -24 * np.abs(mu64)).all()


# ------------------------------------------------------------------------------------------ non-finite inputs
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_row_of_e1_is_never_a_hit(value):
    e1, e2 = ef.stat_embeddings()
    n, r = len(e1), kc.bad_row()
    clean, clean_rank = dist_rank(e1, e2, True)
    bad = kc.poisoned(e1, value)
    got, rank = dist_rank(bad, e2, True)
    assert not np.isfinite(got[r]).any()                                 # never 0
    assert np.array_equal(np.delete(got, r, 0), np.delete(clean, r, 0))
    assert rank[r] == n and np.array_equal(np.delete(rank, r), np.delete(clean_rank, r))
    assert np.array_equal(rank, ef.diagonal_ranks(bad, e2, np.float64))
    for k in (1, 3, n):
        hits = host(mt.calculate_R_precision(cu(bad), cu(e2), k))
        assert hits.shape == (n, k) and not hits[r].any()
        assert np.array_equal(np.delete(hits, r, 0), np.delete(clean_rank[:, None] < np.arange(1, k + 1)[None], r, 0))
    assert not np.isfinite(host(mt.euclidean_distance_matrix(cu(bad), cu(e2)))[r]).any()


def test_nan_row_of_e2_is_a_nan_column():
    e1, e2 = ef.stat_embeddings()
    n, r = len(e1), kc.bad_row()
    clean, clean_rank = dist_rank(e1, e2, True)
    bad = kc.poisoned(e2, np.nan)
    got, rank = dist_rank(e1, bad, True)
    assert np.isnan(got[:, r]).all()
    assert np.array_equal(np.delete(got, r, 1), np.delete(clean, r, 1))
    want = clean_rank - (clean[:, r] < np.diag(clean))                   # the NaN column is "not below": numpy's <
    want[r] = n
    assert np.array_equal(rank, want) and (want != clean_rank).sum() >= 3
    assert np.array_equal(rank, ef.diagonal_ranks(e1, bad, np.float64))


def small_evaluator():
    mv, mo, tx = ef.nets(ef.SMALL_POSE)
    t = lambda sd: {k: torch.from_numpy(v) for k, v in sd.items()}
    return ew.MotionEvaluator(t(mv), t(mo), t(tx), dim_pose=ef.SMALL_POSE, device=dev())


def test_nan_frame_poisons_its_own_clip_only():
    ev = small_evaluator()
    motions, lens = kc.small_invariant_case()
    base = host(ev.embed_motions(cu(motions), lens))
    assert np.isfinite(base).all()
    for b, frame in ((0, 0), (7, lens[7] - 1), (18, 4 * (lens[18] // 4) + 2)):       # the first frame, the last of the length, the last read
        bad = motions.copy()
        bad[b, frame, 3] = np.nan
        got = host(ev.embed_motions(cu(bad), lens))
        assert not np.isfinite(got[b]).any()
        assert np.array_equal(np.delete(got, b, 0), np.delete(base, b, 0))
    dropped = motions.copy()
    dropped[:, :, ef.SMALL_POSE - 4:] = np.nan                           # the four trailing features are not read at all
    assert np.array_equal(host(ev.embed_motions(cu(dropped), lens)), base)


def test_nan_in_frames_past_a_clips_length_is_not_read():
    """test_gpu_evaluator.test_frames_past_a_clips_length_are_not_read with NaN in place of 7.0."""
    ev = small_evaluator()
    motions, lens = kc.small_invariant_case()
    base = host(ev.embed_motions(cu(motions), lens))
    changed = motions.copy()
    for b, n in enumerate(lens):
        changed[b, 4 * (n // 4) + 3:] = np.nan
    assert any(4 * (n // 4) + 3 < motions.shape[1] for n in lens)
    assert np.array_equal(host(ev.embed_motions(cu(changed), lens)), base)


def test_statistics_of_a_nan_row_are_nan():
    e1, e2 = ef.stat_embeddings()
    r, c = kc.bad_row(), kc.BAD_COL
    bad = kc.poisoned(e1, np.nan)
    mu0, cov0 = (host(t) for t in mt.calculate_activation_statistics(cu(e1)))
    mu, cov = (host(t) for t in mt.calculate_activation_statistics(cu(bad)))
    assert np.isnan(mu[c]) and np.isnan(cov[c]).all() and np.isnan(cov[:, c]).all()
    keep = np.arange(e1.shape[1]) != c
    assert np.array_equal(mu[keep], mu0[keep]) and np.array_equal(cov[keep][:, keep], cov0[keep][:, keep])
    match0, match = host(mt.calculate_matching_score(cu(e1), cu(e2))), host(mt.calculate_matching_score(cu(bad), cu(e2)))
    assert np.isnan(match[r]) and np.array_equal(np.delete(match, r), np.delete(match0, r))
    assert np.isnan(mt.calculate_matching_score(bad, e2, sum_all=True))


def test_report_the_worst_ratios():
    """Kernel distance over the fp32 restatement's, per group: reported, not asserted."""
    for group, (ratio, tag) in sorted(WORST.items()):
        print(f"eval: worst kernel / fp32 ratio, {group}: {ratio:.2f} ({tag})")
