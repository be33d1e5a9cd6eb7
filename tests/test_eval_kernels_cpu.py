"""The cases of tests/test_gpu_eval_kernels.py themselves (tests/eval_kernel_cases.py), without a GPU: a failure there then means the
kernel is wrong and not its input.  The case lists cover what they claim to cover; the integer distance cases are exact in fp32 and hold
the ranks and ties they are there for; the float32 numpy restatement of every case lies inside the derived bound or, where the bar is
4 x its own distance from float64, has a distance small enough for that bar to mean something."""
import itertools

import numpy as np
import pytest

import eval_fixture as ef
import eval_kernel_cases as kc

# fp32 against float64 where the bar is eval_fixture.bar of the restatement's own distance.  Measured: LayerNorm at most 1.6e-7 but for
# two cases that cancel by construction -- five rows of width 2 (a close pair: 1.0e-6) and the rows at mean 100 (the fp32 mean of
# values near 100 is good to 1e-5 of a unit spread: 3.6e-6); GRU 2.2e-7; distances 1.2e-7.  1e-6 = 4 x 2.5e-7 is the bar's floor; a
# bar stops meaning anything from 1e-4 on
OWN_DISTANCE = 1e-6
CANCELLING = {"w2_r5_l0": 2e-6, "w2_r5_l1": 2e-6, "mean100_w100_r5_l1": 5e-6}


def pairs_of(cases, x, y):
    return {(c[x], c[y]) for c in cases}


def test_gemm_list_is_pairwise_covering():
    cases = kc.gemm_cases()
    assert len(cases) <= 40 and len({c["name"] for c in cases}) == len(cases)
    assert pairs_of(cases, "M", "N") == set(itertools.product(kc.GEMM_M, kc.GEMM_N))
    assert pairs_of(cases, "M", "K") == set(itertools.product(kc.GEMM_M, kc.GEMM_K))
    assert pairs_of(cases, "N", "K") == set(itertools.product(kc.GEMM_N, kc.GEMM_K))
    for opt in ("bias", "add", "leaky", "padded"):
        assert {bool(c[opt]) for c in cases} == {False, True}, opt
    assert any(c["add"] and c["leaky"] for c in cases) and any(c["add"] and not c["bias"] for c in cases)
    for c in cases:
        d = kc.gemm_data(c)
        if c["padded"]:
            assert (d["lda"], d["ldc"], d["ldadd"]) == (c["K"] + 5, c["N"] + 3, c["N"] + 7)
            assert np.isnan(d["a"][:, c["K"]:]).all() and (not c["add"] or np.isnan(d["add"][:, c["N"]:]).all())
        assert np.isfinite(d["a"][:, :c["K"]]).all()
        if c["bias"]:
            assert np.abs(d["bias"]).min() > 0.1                     # dropping it is visible against a bound of ~1e-6
        if c["add"]:
            assert np.abs(d["add"][:, :c["N"]]).min() > 0.1


def test_conv_list_is_pairwise_covering():
    cases = kc.conv_cases()
    axes = dict(T=kc.CONV_FRAMES, C=kc.CONV_CHANNELS, B=kc.CONV_BATCH, N=kc.CONV_N)
    for x, y in itertools.combinations(axes, 2):
        assert pairs_of(cases, x, y) == set(itertools.product(axes[x], axes[y])), (x, y)
    assert max(c["B"] * ef.conv_frames(c["T"]) for c in cases) > 64      # more than one row tile
    for c in cases:
        d = kc.conv_data(c)
        B, T, C, F = c["B"], c["T"], c["C"], d["F"]
        assert F == C + 4 and d["sb"] == T * F + 11
        rows, sample = d["rows"][:, :T * F].reshape(B, T, F), d["sample"][:, :T * F].reshape(B, F, T)
        assert np.array_equal(rows[:, :, :C], d["x"]) and np.array_equal(sample[:, :C].transpose(0, 2, 1), d["x"])
        assert np.isnan(rows[:, :, C:]).all() and np.isnan(sample[:, C:]).all()
        assert np.isnan(d["rows"][:, T * F:]).all() and np.isnan(d["sample"][:, T * F:]).all()
        assert np.array_equal(d["wk"].reshape(c["N"], 4, C)[:, 2], d["w"][:, :, 2])                  # k = tap * C + channel


@pytest.mark.parametrize("case", kc.gemm_cases(), ids=lambda c: c["name"])
def test_gemm_restatement_lies_inside_the_bound(case):
    err = np.abs(kc.gemm_ref(case, np.float32).astype(np.float64) - kc.gemm_ref(case, np.float64))
    assert (err <= kc.gemm_bound(case)).all()


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("case", kc.conv_cases(), ids=lambda c: c["name"])
def test_conv_restatement_lies_inside_the_bound(case, affine):
    f32, f64 = kc.conv_ref(case, affine, np.float32), kc.conv_ref(case, affine, np.float64)
    assert f32.dtype == np.float32 and f64.shape == (case["B"] * ef.conv_frames(case["T"]), case["N"])
    assert (np.abs(f32.astype(np.float64) - f64) <= kc.conv_bound(case, affine)).all()


def test_bound_catches_what_it_is_there_for():
    """A dropped k-remainder, a dropped bias and an f16-rounded operand each leave the bound by a wide margin."""
    case = next(c for c in kc.gemm_cases() if c["K"] == 33 and c["bias"] and c["M"] > 1)
    d, f64, bound = kc.gemm_data(case), kc.gemm_ref(case, np.float64), kc.gemm_bound(case)
    act = ef.leaky if case["leaky"] else (lambda v: v)
    full = lambda a, w, b: act(a.astype(np.float64) @ w.astype(np.float64).T + b + (d["add"][:, :case["N"]] if case["add"] else 0.0))
    a, w, b = d["a"][:, :33], d["w"], d["bias"].astype(np.float64)
    assert (np.abs(full(a, w, b) - f64) <= bound).all()
    for wrong in (full(a[:, :32], w[:, :32], b), full(a, w, 0.0), full(a.astype(np.float16), w, b)):
        assert (np.abs(wrong - f64) > bound).mean() > 0.9


def test_layernorm_cases():
    cases = kc.ln_cases()
    assert {(c["W"], c["R"], c["leaky"]) for c in cases if c["kind"] == "normal"} == set(itertools.product(kc.LN_WIDTHS, kc.LN_ROWS, (0, 1)))
    worst = 0.0
    for c in cases:
        d, f32, f64 = kc.ln_data(c), kc.ln_ref(c, np.float32), kc.ln_ref(c, np.float64)
        dist = ef.relmax(f32, f64)
        worst = max(worst, dist)
        assert dist <= CANCELLING.get(c["name"], OWN_DISTANCE), (c["name"], dist)
        if c["leaky"] and c["W"] >= 63:
            assert (f64 < 0).any() and (f64 > 0).any()                  # both branches of the activation
        if c["kind"] == "mean100":
            assert abs(d["x"].mean() - 100) < 0.5 and 0.8 < d["x"].std() < 1.2
        if c["kind"] == "constant":
            want = d["beta"].astype(np.float64)
            assert np.array_equal(f64[0], ef.leaky(want) if c["leaky"] else want) and len(set(d["x"][0])) == 1 and len(set(d["x"][1])) > 1
        if c["W"] == 1:
            want = np.broadcast_to(d["beta"].astype(np.float64), f64.shape)
            assert np.array_equal(f64, ef.leaky(want) if c["leaky"] else want)
    print(f"evalk: layernorm fp32 distance at most {worst:.3e}")


def test_gru_cases():
    cases = kc.gru_cases()
    assert {(c["H"], c["B"], c["S"]) for c in cases} == set(itertools.product(kc.GRU_H, kc.GRU_BATCH, kc.GRU_MAX_STEPS))
    for c in cases:
        xproj, steps = kc.gru_data(c)
        assert steps.max() == c["S"] and steps.min() >= 1 and (c["B"] == 1 or c["S"] == 1 or (steps[0] < c["S"] and len(set(steps)) > 1))
        for b in range(c["B"]):
            assert np.isfinite(xproj[b, :steps[b]]).all() and np.isnan(xproj[b, steps[b]:]).all()
    worst = 0.0
    for c in cases:
        if c["B"] in (1, 33):                                            # the larger batches hold the smaller ones' arithmetic
            f64 = kc.gru_ref(c, np.float64)
            assert np.isfinite(f64).all() and f64.shape == (c["B"], 2 * c["H"])
            dist = ef.relmax(kc.gru_ref(c, np.float32), f64)
            worst = max(worst, dist)
            assert dist <= OWN_DISTANCE, (c["name"], dist)
    print(f"evalk: gru fp32 distance at most {worst:.3e}")


def test_projected_recurrence_is_gru_last():
    """`gru_last` is its own input projection followed by `gru_last_projected`: the split changed no number."""
    H, B, L = 64, 5, 6
    sd = kc.gru_state(H)
    x = ef.syn.normal(ef.SEED, "evalk/gru/x", (B, L, H))
    steps = [6, 1, 3, 6, 2]
    for dtype in (np.float32, np.float64):
        xd = np.asarray(x, dtype)
        proj = [xd @ np.asarray(sd[f"gru.weight_ih_l0{r}"], dtype).T + np.asarray(sd[f"gru.bias_ih_l0{r}"], dtype) for r in ("", "_reverse")]
        assert np.array_equal(ef.gru_last(sd, xd, steps, dtype), ef.gru_last_projected(sd, proj, steps, dtype))
    clamped = kc.gru_ref(dict(H=H, B=3, S=6), np.float64, steps=[0, 9, -2])          # the clamps: 0, positions, 0
    init = np.asarray(sd["hidden"], np.float64).reshape(2 * H)
    assert np.array_equal(clamped[0], init) and np.array_equal(clamped[2], init)
    assert np.array_equal(clamped[1], kc.gru_ref(dict(H=H, B=3, S=6), np.float64, steps=[0, 6, -2])[1])


@pytest.mark.parametrize("shape", [(n, n, d) for n, d in kc.DIST_SQUARE] + list(kc.DIST_RECT), ids=str)
def test_integer_distance_cases_are_exact_in_fp32(shape):
    n1, n2, d = shape
    e1, e2 = kc.dist_int_case(n1, n2, d)
    assert e1.shape == (n1, d) and e2.shape == (n2, d) and e1.dtype == np.float32
    for e in (e1, e2):
        assert np.array_equal(e, np.round(e)) and np.abs(e).max() <= 3
    assert 4 * 9 * d < 2 ** 24                                           # |-2 a.b| + |a|^2 + |b|^2 <= 4 * 9 d: every partial sum is exact
    rad = kc.radicands(e1, e2)
    assert rad.min() >= 0 and rad.max() < 2 ** 24
    f32 = ef.euclidean_distance_matrix(e1, e2, np.float32)
    assert f32.dtype == np.float32 and np.array_equal(f32, np.sqrt(rad.astype(np.float32)))
    if n1 == n2:                                                         # the root keeps the order and the ties of the radicands
        assert np.array_equal(ef.diagonal_ranks(e1, e2, np.float32), kc.integer_ranks(rad))
        assert np.array_equal(ef.diagonal_ranks(e1, e2, np.float64), kc.integer_ranks(rad))


def test_integer_distance_cases_hold_ranks_and_ties():
    for n, d in kc.DIST_SQUARE:
        rad = kc.radicands(*kc.dist_int_case(n, n, d))
        ranks, ties = kc.integer_ranks(rad), kc.tie_rows(rad)
        print(f"evalk: dist ({n}, {d}) rank >= 3 in {np.mean(ranks >= 3):.2f} of the rows, a tie in {ties.mean():.2f}, max rank {ranks.max()}")
        if n >= 33:
            assert np.mean(ranks >= 3) >= 1 / 3, (n, d)
        if (n, d) in ((300, 37), (260, 65)):
            assert ties.mean() >= 0.1, (n, d)
    rad = kc.radicands(*kc.dist_int_case(257, 257, 1))
    ranks = kc.integer_ranks(rad)
    # no rank can exceed n2 - 1 = 256: one row reaches it, every other entry strictly below its diagonal one, so the count's second trip
    # (j = 256) contributes; and column 256 is below the diagonal for many rows
    assert ranks.max() == 256 and ranks[5] == 256
    assert (rad[:, 256] < np.diag(rad)).sum() >= 20


def test_real_distance_and_pair_cases():
    for n1, n2, d in kc.DIST_REAL:
        e1, e2 = kc.dist_real_case(n1, n2, d)
        dist = ef.relmax(ef.euclidean_distance_matrix(e1, e2, np.float32), ef.euclidean_distance_matrix(e1, e2, np.float64))
        assert dist <= OWN_DISTANCE, (n1, n2, d, dist)
    cases = kc.pair_cases()
    assert {(c["d"], c["pairs"]) for c in cases} == set(itertools.product(kc.PAIR_D, kc.PAIR_COUNTS)) and kc.PAIR_NA != kc.PAIR_NB
    for c in cases:
        a, b, ia, ib = kc.pair_data(c)
        assert a.shape == (kc.PAIR_NA, c["d"]) and b.shape == (kc.PAIR_NB, c["d"])
        assert 0 <= ia.min() and ia.max() == kc.PAIR_NA - 1 and 0 <= ib.min() and ib.max() == kc.PAIR_NB - 1
        f32, f64 = kc.pair_ref(c, np.float32), kc.pair_ref(c, np.float64)
        if c["kind"] == "int":
            assert np.array_equal(f32, np.sqrt(((a[ia] - b[ib]) ** 2).sum(1, dtype=np.float64).astype(np.float32)))
        else:
            assert (np.abs(f32 - f64) <= (c["d"] + 4) * kc.EPS32 * f64).all()


def test_rank_restatement_with_non_finite_rows():
    e1, e2 = ef.stat_embeddings()
    clean = ef.diagonal_ranks(e1, e2, np.float64)
    n, r = len(e1), kc.bad_row()
    for value in (np.nan, np.inf):
        ranks = ef.diagonal_ranks(kc.poisoned(e1, value), e2, np.float64)
        assert ranks[r] == n and np.array_equal(np.delete(ranks, r), np.delete(clean, r))
        with np.errstate(invalid="ignore"):
            assert not np.isfinite(ef.euclidean_distance_matrix(kc.poisoned(e1, value), e2, np.float32)[r]).any()
    ranks = ef.diagonal_ranks(e1, kc.poisoned(e2, np.nan), np.float64)     # column r is NaN: not below any diagonal
    d = ef.euclidean_distance_matrix(e1, e2, np.float64)
    assert ranks[r] == n and np.array_equal(np.delete(ranks, r), np.delete(clean - (d[:, r] < np.diag(d)), r))
    assert (d[:, r] < np.diag(d)).sum() >= 2                                 # and for some row that changes the rank
    motions, lens = kc.small_invariant_case()
    assert motions.shape == (19, 24, ef.SMALL_POSE) and {n // 4 for n in lens} == {1, 2, 3, 4, 5, 6}
    assert any(4 * (n // 4) + 3 < motions.shape[1] for n in lens)
