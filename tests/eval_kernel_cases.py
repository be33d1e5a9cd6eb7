"""Cases for the `mst_eval_*` entry points taken one by one (tests/test_gpu_eval_kernels.py runs them on the GPU,
tests/test_eval_kernels_cpu.py holds the cases themselves): inputs from a seed through mst_amd.synthetic, and for every case the same
operation in numpy at a dtype of the caller's choice -- float64 is the reference, float32 its restatement, whose distance from float64
sets a bar or is shown to lie inside a derived bound.  The operations are eval_fixture's (`linear`, `conv_k4s2p1`, `leaky`,
`gru_last_projected`, `euclidean_distance_matrix`, `matching_score`); nothing here knows the kernels.

Buffers are laid out as the entry points read them, with every element that must never be read set to NaN and every element that must
never be written set to SENTINEL."""
import functools

import numpy as np

import eval_fixture as ef

syn = ef.syn
SEED = ef.SEED
SENTINEL = np.float32(-77.25)
EPS32 = 2.0 ** -24
LN_EPS = 1e-5


def _n(tag, shape):
    return syn.normal(SEED, "evalk/" + tag, shape)


def _ints(tag, shape, lo, hi):
    """Integers lo .. hi inclusive as float32."""
    n = int(np.prod(shape))
    return (lo + np.floor(syn.uniform01(SEED, "evalk/" + tag, n) * (hi - lo + 1))).astype(np.float32).reshape(shape)


# ------------------------------------------------------------------------------------------ mst_eval_gemm, plain
GEMM_M = (1, 63, 64, 65, 130)
GEMM_N = (1, 15, 64, 65, 200)
GEMM_K = (1, 3, 4, 31, 32, 33, 70)


def gemm_cases():
    """35 cases, pairwise covering: K index i and M index j meet once each, N takes index (i + j) % 5, so every K meets every N (j runs
    over 0 .. 4) and every M meets every N (i runs over 0 .. 6).  The options cycle with different periods over the case number c."""
    out = []
    for i, K in enumerate(GEMM_K):
        for j, M in enumerate(GEMM_M):
            c = len(out)
            out.append(dict(name=f"m{M}_n{GEMM_N[(i + j) % 5]}_k{K}", M=M, N=GEMM_N[(i + j) % 5], K=K, bias=c % 3 != 1, add=c % 2 == 1,
                            leaky=(c // 2) % 2 == 1, padded=c % 5 != 4))
    return out


@functools.lru_cache(maxsize=None)
def _gemm_data(name, M, N, K, bias, add, padded):
    lda, ldc, ldadd = (K + 5, N + 3, N + 7) if padded else (K, N, N)
    a = np.full((M, lda), np.nan, np.float32)
    a[:, :K] = _n(f"gemm/a/{name}", (M, K))
    w = _n(f"gemm/w/{name}", (N, K))
    b = (1.0 + 0.2 * _n(f"gemm/b/{name}", (N,))).astype(np.float32) if bias else None
    ad = None
    if add:
        ad = np.full((M, ldadd), np.nan, np.float32)
        ad[:, :N] = -2.0 + 0.25 * _n(f"gemm/add/{name}", (M, N))
    return dict(a=a, w=w, bias=b, add=ad, lda=lda, ldc=ldc, ldadd=ldadd)


def gemm_data(case):
    """-> a [M, lda], w [N, K], bias [N] or None, add [M, ldadd] or None; the padding columns of a and add are NaN."""
    return _gemm_data(case["name"], case["M"], case["N"], case["K"], case["bias"], case["add"], case["padded"])


def gemm_ref(case, dtype):
    d, M, N, K = gemm_data(case), case["M"], case["N"], case["K"]
    y = ef.linear(np.asarray(d["a"][:, :K], dtype), d["w"], d["bias"] if case["bias"] else np.zeros(N, np.float32), dtype)
    if case["add"]:
        y = y + np.asarray(d["add"][:, :N], dtype)
    return ef.leaky(y) if case["leaky"] else y


def gemm_bound(case):
    """(K + 4) 2^-24 (|A| |W|^T + |bias| + |add|), element-wise: any order of a K-term fp32 sum, then the bias, the add, the join of the
    two chains; LeakyReLU is 1-Lipschitz."""
    d, N, K = gemm_data(case), case["N"], case["K"]
    mag = np.abs(d["a"][:, :K].astype(np.float64)) @ np.abs(d["w"].astype(np.float64)).T
    if case["bias"]:
        mag = mag + np.abs(d["bias"].astype(np.float64))
    if case["add"]:
        mag = mag + np.abs(d["add"][:, :N].astype(np.float64))
    return (K + 4) * EPS32 * mag


# ------------------------------------------------------------------------------------------ mst_eval_gemm, conv prologues
CONV_FRAMES = (2, 3, 4, 5, 9)
CONV_CHANNELS = (1, 7, 12, 37)
CONV_BATCH = (1, 3, 17)
CONV_N = (16, 70)
CONV_EXTRA, CONV_GAP = 4, 11                   # features a frame past `channels`; floats between clips past the minimum stride


def conv_cases():
    """20 geometries, pairwise covering: every (frames, channels) pair once, batch and N by (i + j) % 3 and (i + j) % 2, so that i + j
    mod 6 meets all six (batch, N) pairs and each of them every frames and channels value."""
    return [dict(name=f"t{T}_c{C}_b{CONV_BATCH[(i + j) % 3]}_n{CONV_N[(i + j) % 2]}", T=T, C=C, B=CONV_BATCH[(i + j) % 3], N=CONV_N[(i + j) % 2])
            for i, T in enumerate(CONV_FRAMES) for j, C in enumerate(CONV_CHANNELS)]


@functools.lru_cache(maxsize=None)
def _conv_data(name, T, C, B, N):
    F = C + CONV_EXTRA
    x = _n(f"conv/x/{name}", (B, T, C))
    sb = T * F + CONV_GAP
    rows = np.full((B, sb), np.nan, np.float32)                         # mode 1: [B][T][F], features C .. F - 1 and the gap NaN
    view = rows[:, :T * F].reshape(B, T, F)
    view[:, :, :C] = x
    sample = np.full((B, sb), np.nan, np.float32)                       # mode 2: [B][F][T], the same
    sample[:, :T * F].reshape(B, F, T)[:, :C] = x.transpose(0, 2, 1)
    w = _n(f"conv/w/{name}", (N, C, 4))
    return dict(x=x, rows=rows, sample=sample, sb=sb, F=F, w=w, wk=np.ascontiguousarray(w.transpose(0, 2, 1).reshape(N, 4 * C)),
                bias=(1.0 + 0.2 * _n(f"conv/b/{name}", (N,))).astype(np.float32),
                scale=(0.5 + syn.uniform01(SEED, f"evalk/conv/scale/{name}", C)).astype(np.float32),
                shift=(0.5 * _n(f"conv/shift/{name}", (C,))).astype(np.float32))


def conv_data(case):
    """-> x [B, T, C]; rows / sample: the mode 1 / mode 2 buffers [B, sb] holding it; w [N, C, 4] and wk [N, 4 C] (k = tap C + channel);
    bias [N]; scale, shift [C]."""
    return _conv_data(case["name"], case["T"], case["C"], case["B"], case["N"])


def conv_ref(case, affine, dtype):
    """conv_k4s2p1 on the affine-transformed input, then LeakyReLU -> [B * T_out, N]."""
    d = conv_data(case)
    x = np.asarray(d["x"], dtype)
    if affine:
        x = x * np.asarray(d["scale"], dtype) + np.asarray(d["shift"], dtype)
    return ef.leaky(ef.conv_k4s2p1(x, d["w"], d["bias"], dtype)).reshape(-1, case["N"])


def conv_bound(case, affine):
    """(K + 4) 2^-24 (|A| |W|^T + |bias|) with K = 4 channels; with the affine |A| = |x scale| + |shift| and K + 6."""
    d, K = conv_data(case), 4 * case["C"]
    x = np.abs(d["x"].astype(np.float64))
    if affine:
        x = x * np.abs(d["scale"].astype(np.float64)) + np.abs(d["shift"].astype(np.float64))
    mag = ef.conv_k4s2p1(x, np.abs(d["w"]), np.abs(d["bias"]), np.float64).reshape(-1, case["N"])
    return (K + (6 if affine else 4)) * EPS32 * mag


# ------------------------------------------------------------------------------------------ mst_eval_layernorm
LN_WIDTHS = (1, 2, 63, 64, 65, 100, 512)
LN_ROWS = (1, 5)


def ln_cases():
    out = [dict(name=f"w{W}_r{R}_l{L}", W=W, R=R, leaky=L, kind="normal") for W in LN_WIDTHS for R in LN_ROWS for L in (0, 1)]
    out.append(dict(name="mean100_w100_r5_l1", W=100, R=5, leaky=1, kind="mean100"))
    out.append(dict(name="constant_w100_r2_l0", W=100, R=2, leaky=0, kind="constant"))
    out.append(dict(name="constant_w100_r2_l1", W=100, R=2, leaky=1, kind="constant"))
    return out


@functools.lru_cache(maxsize=None)
def _ln_data(name, W, R, kind):
    x = _n(f"ln/x/{W}/{R}", (R, W))
    if kind == "mean100":
        x = (100.0 + x).astype(np.float32)
    if kind == "constant":                                               # row 0 constant: 3.25 and its multiples up to 325 are exact in fp32,
        x[0] = 3.25                                                      # so mean = 3.25 and variance = 0 in any summation order
    return dict(x=x, gamma=(1.0 + 0.1 * _n(f"ln/g/{W}", (W,))).astype(np.float32), beta=(0.1 * _n(f"ln/b/{W}", (W,)) + 0.05).astype(np.float32))


def ln_data(case):
    return _ln_data(case["name"], case["W"], case["R"], case["kind"])


def ln_ref(case, dtype):
    d = ln_data(case)
    x = np.asarray(d["x"], dtype)
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    y = (x - mean) / np.sqrt(var + dtype(LN_EPS)) * np.asarray(d["gamma"], dtype) + np.asarray(d["beta"], dtype)
    return ef.leaky(y) if case["leaky"] else y


# ------------------------------------------------------------------------------------------ mst_eval_gru
GRU_H = (64, 128, 192)
GRU_BATCH = (1, 16, 17, 33)
GRU_POSITIONS = 6
GRU_MAX_STEPS = (1, 2, 5, 6)


def gru_cases():
    return [dict(name=f"h{H}_b{B}_s{S}", H=H, B=B, S=S) for H in GRU_H for B in GRU_BATCH for S in GRU_MAX_STEPS]


def gru_steps(B, S):
    """Step counts 1 .. S mixed, the longest clip second where there is one, not first."""
    steps = [1 + b % S for b in range(B)]
    steps[min(1, B - 1)] = S
    return np.asarray(steps, np.int32)


def gru_state(H):
    return ef.recurrent_state("kernel", H, H, 32)


@functools.lru_cache(maxsize=None)
def _gru_xproj(H, B):
    return (0.8 * _n(f"gru/xproj/{H}/{B}", (B, GRU_POSITIONS, 2, 3, H))).astype(np.float32)


def gru_data(case, steps=None):
    """-> xproj [B, positions, 2, 3, H] with NaN at every position its clip does not reach, steps [B] int32."""
    steps = gru_steps(case["B"], case["S"]) if steps is None else np.asarray(steps, np.int32)
    xproj = _gru_xproj(case["H"], case["B"]).copy()
    reach = np.clip(steps, 0, GRU_POSITIONS)
    for b in range(case["B"]):
        xproj[b, reach[b]:] = np.nan
    return xproj, steps


def gru_ref(case, dtype, steps=None):
    """`gru_last_projected` on the case's projections and state -> [B, 2 H]."""
    xproj, steps = gru_data(case, steps)
    B, H = case["B"], case["H"]
    proj = [xproj[:, :, d].reshape(B, GRU_POSITIONS, 3 * H) for d in (0, 1)]
    return ef.gru_last_projected(gru_state(H), proj, np.clip(steps, 0, GRU_POSITIONS), dtype)


# ------------------------------------------------------------------------------------------ mst_eval_dist_rank
DIST_SQUARE = ((300, 37), (260, 65), (257, 1), (33, 512), (40, 8192), (3, 100), (1, 5))
DIST_RECT = ((5, 300, 37), (300, 2, 64), (7, 1, 3))
DIST_REAL = ((64, 64, 100), (5, 70, 513))
PROTOTYPES = 6


@functools.lru_cache(maxsize=None)
def dist_int_case(n1, n2, d):
    """Integer embeddings in [-3, 3]: every row is one of PROTOTYPES prototype rows with 0 .. 3 entries redrawn.  Half the rows of E2
    follow their E1 row's prototype (a small diagonal distance, a low rank), half another one (every E2 row of E1's prototype then lies
    below the diagonal); a row with nothing redrawn equals every other such row of its prototype, so exact ties are common.  d = 1 has no
    room for prototypes: plain draws, and row 5 set so that every other entry of its row lies strictly below its diagonal one."""
    tag = f"dist/{n1}/{n2}/{d}"
    if d == 1:
        e1, e2 = _ints(tag + "/e1", (n1, 1), -3, 3), _ints(tag + "/e2", (n2, 1), -2, 3)
        if n1 > 5 and n2 > 5:
            e1[5], e2[5] = 3.0, -3.0
        return e1, e2
    proto = _ints(tag + "/proto", (PROTOTYPES, d), -3, 3)
    u = lambda name, n: syn.uniform01(SEED, f"evalk/{tag}/{name}", n)
    p1 = np.floor(u("p1", n1) * PROTOTYPES).astype(np.int64)
    p2 = np.floor(u("p2", n2) * PROTOTYPES).astype(np.int64)
    follow = u("follow", n2) < 0.5
    m = min(n1, n2)
    p2[:m] = np.where(follow[:m], p1[:m], p2[:m])

    def rows(which, name, n):
        e = proto[which].copy()
        count = np.floor(u(name + "/count", n) * 4).astype(np.int64)      # 0 .. 3 entries redrawn
        col = np.floor(u(name + "/col", 3 * n) * d).astype(np.int64).reshape(n, 3)
        val = _ints(f"{tag}/{name}/val", (n, 3), -3, 3)
        for r in range(n):
            e[r, col[r, :count[r]]] = val[r, :count[r]]
        return e
    return rows(p1, "e1", n1), rows(p2, "e2", n2)


def radicands(e1, e2):
    """|a - b|^2 as exact integers [n1, n2]."""
    a, b = np.asarray(e1, np.int64), np.asarray(e2, np.int64)
    return -2 * (a @ b.T) + (a * a).sum(1, keepdims=True) + (b * b).sum(1)


def integer_ranks(rad):
    return (rad < np.diag(rad)[:, None]).sum(1)


def tie_rows(rad):
    """Rows that hold an entry equal to their diagonal one, elsewhere."""
    same = rad == np.diag(rad)[:, None]
    return same.sum(1) > 1


@functools.lru_cache(maxsize=None)
def dist_real_case(n1, n2, d):
    return _n(f"dist/real/{n1}/{n2}/{d}/e1", (n1, d)), _n(f"dist/real/{n1}/{n2}/{d}/e2", (n2, d))


# ------------------------------------------------------------------------------------------ mst_eval_pair_norms
PAIR_D = (1, 63, 64, 65, 513)
PAIR_COUNTS = (1, 3, 4, 5, 9)
PAIR_NA, PAIR_NB = 7, 5


def pair_cases():
    return [dict(name=f"d{d}_p{p}_{kind}", d=d, pairs=p, kind=kind) for d in PAIR_D for p in PAIR_COUNTS for kind in ("int", "normal")]


@functools.lru_cache(maxsize=None)
def _pair_data(d, pairs, kind):
    tag = f"pair/{d}/{pairs}/{kind}"
    if kind == "int":
        a, b = _ints(tag + "/a", (PAIR_NA, d), -3, 3), _ints(tag + "/b", (PAIR_NB, d), -3, 3)
    else:
        a, b = _n(tag + "/a", (PAIR_NA, d)), _n(tag + "/b", (PAIR_NB, d))
    ia = np.floor(syn.uniform01(SEED, "evalk/" + tag + "/ia", pairs) * PAIR_NA).astype(np.int32)
    ib = np.floor(syn.uniform01(SEED, "evalk/" + tag + "/ib", pairs) * PAIR_NB).astype(np.int32)
    ia[0], ib[0] = PAIR_NA - 1, PAIR_NB - 1                              # the last row of each matrix is read
    return a, b, ia, ib


def pair_data(case):
    return _pair_data(case["d"], case["pairs"], case["kind"])


def pair_ref(case, dtype):
    a, b, ia, ib = pair_data(case)
    return ef.matching_score(a[ia], b[ib], dtype)


# ------------------------------------------------------------------------------------------ mst_eval_cov
COV_N = (1, 2, 65)
COV_D = (1, 20)


def cov_rows(n, d):
    return (3.0 * _n(f"cov/{n}/{d}", (n, d)) + (1.0 + np.arange(d, dtype=np.float32) % 7)).astype(np.float32)


# ------------------------------------------------------------------------------------------ non-finite inputs
BAD_COL = 17


@functools.lru_cache(maxsize=None)
def bad_row():
    """The row of eval_fixture.stat_embeddings that takes the non-finite value: the first whose column of the clean distance matrix lies
    below the diagonal entry of at least two other rows, so that a NaN column there changes ranks."""
    d = ef.euclidean_distance_matrix(*ef.stat_embeddings(), np.float64)
    below = (d < np.diag(d)[:, None]).sum(0)
    return int(np.nonzero(below >= 2)[0][0])


def poisoned(e, value, row=None, col=BAD_COL):
    out = np.array(e, np.float32, copy=True)
    out[bad_row() if row is None else row, col] = value
    return out


def small_invariant_case():
    """test_gpu_evaluator.invariant_case at SMALL_POSE: 19 clips of 24 frames, 1 .. 6 movement frames."""
    B, T, F = 19, 24, ef.SMALL_POSE
    motions = _n("invariant/small", (B, T, F))
    lens = [min(4 * (1 + (b + 3) % 6) + b % 3, T) for b in range(B)]
    return motions, lens
