"""oracle/philox.py -- the float64 statement of the engine's in-kernel noise -- held to what can be known without a GPU:

  * the generator: Random123's published known-answer vectors for Philox4x32-10;
  * the uniform mapping at its edges (no log(0), the largest radius, an exact zero);
  * the counter layout: element (clip, f, t) of a step against a direct call with counter (t >> 2, f, clip, step), counters
    pairwise distinct over clips x features x quads x steps, a clip's noise independent of the batch it is in;
  * the distribution at the headline shape (64 x 263 x 196 = 3.3 M values per step): moments, Kolmogorov-Smirnov, tails, and the
    correlations along every axis of the counter and of the key;
  * sharding.rank_seed: distinct keys per (rank, pass).

The statistical bars are conditions fixed in advance (|z| < 4.5: p ~ 7e-6 per test under the null; sqrt(n) D < 1.95: p ~ 1e-3),
seeds and steps are fixed, so the tests are deterministic.  tests/test_gpu_noise.py holds every kernel that draws to this oracle."""
import math

import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
from oracle import philox

B, F, T = 64, 263, 196                  # the headline shape (bench.py's default workload)
Z_BAR, KS_BAR = 4.5, 1.95
HI = 1 << 32


# ------------------------------------------------------------------------------ the generator
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_philox4x32_10_known_answers(ctr, key, want):
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    got = philox.philox4x32_10(*ctr, *key)
    assert tuple(int(g) for g in got) == want, [hex(int(g)) for g in got]


def test_philox4x32_10_is_vectorised():
    """The three known answers in one call (arrays broadcast), so the array path is the scalar path."""
    c = np.array([k[0] for k in KAT], dtype=np.uint64).T
    for i, (_, key, want) in enumerate(KAT):
        got = philox.philox4x32_10(c[0], c[1], c[2], c[3], *key)
        assert tuple(int(g[i]) for g in got) == want


# ------------------------------------------------------------------------------ the uniform mapping
def test_uniform_mapping_edges():
    top, zero = np.uint32(0xffffffff), np.uint32(0)
    u0, u1, u2, u3 = philox.uniforms(top, top, zero, zero)
    assert u0 == 1.0 and u2 == 2.0 ** -24                       # radius uniforms: (0, 1]
    assert u1 == 1.0 - 2.0 ** -24 and u3 == 0.0                 # angle uniforms: [0, 1)
    n = philox.box_muller(u0, u1, u2, u3)
    assert n[0] == 0.0 and n[1] == 0.0                          # u0 = 1: radius exactly 0
    assert abs(n[2] - math.sqrt(48.0 * math.log(2.0))) < 1e-14 and n[3] == 0.0      # u2 = 2^-24 at angle 0: the largest value, sqrt(48 ln 2) = 5.768
    # the low 8 bits do not reach the uniforms; no word gives log(0)
    for r in (0, 1, 0xff, 0x100, 0x7fffffff, 0x80000000, 0xffffff00, 0xffffffff):
        a, b, c, d = philox.uniforms(*(np.uint32(r),) * 4)
        assert 0.0 < a <= 1.0 and 0.0 <= b < 1.0 and a == c and b == d
        assert a == ((r >> 8) + 1) / 2 ** 24 and b == (r >> 8) / 2 ** 24
        assert all(np.isfinite(v) for v in philox.box_muller(a, b, c, d))


# ------------------------------------------------------------------------------ the counter layout
@pytest.mark.parametrize("clip,f,t,step,seed", [(0, 0, 0, 0, 0), (2, 5, 9, 3, 1234), (1, 6, 2, 7, 5 * HI + 11), (3, 1, 11, 2 ** 32 - 1, 2 ** 63 - 1)])
def test_element_is_component_t_and_3_of_counter_tq_f_clip_step(clip, f, t, step, seed):
    """Element (clip, f, t) of step `step` = component t & 3 of counter (t >> 2, f, clip, step) under key (seed lo, seed hi):
    spelled out here with scalar arguments, indices all different so that no permutation of the counter words passes."""
    r = philox.philox4x32_10(t >> 2, f, clip, step, seed & 0xffffffff, seed >> 32)
    want = philox.box_muller(*philox.uniforms(*r))[t & 3]
    got = philox.normal(4, 7, 13, seed, step)
    assert got.shape == (4, 7, 13) and got.dtype == np.float64
    assert got[clip, f, t] == want
    rad, ang = philox.uniform_planes(4, 7, 13, seed, step)
    u = philox.uniforms(*r)
    assert rad[clip, f, t] == u[(t & 3) // 2 * 2] and ang[clip, f, t] == u[(t & 3) // 2 * 2 + 1]


def test_counters_are_pairwise_distinct_and_a_clip_does_not_depend_on_its_batch():
    Bs, Fs, Ts, steps = 5, 7, 18, 4                              # 5 quads per row (the last one ragged)
    seen = set()
    for step in range(steps):
        tq, f, clip, st = (np.broadcast_to(a, (Bs, Fs, (Ts + 3) // 4)).astype(np.uint64) for a in philox.counters(Bs, Fs, Ts, step))
        seen.update((int(a) << 96) | (int(b) << 64) | (int(c) << 32) | int(d)
                    for a, b, c, d in zip(tq.ravel(), f.ravel(), clip.ravel(), st.ravel()))
    assert len(seen) == Bs * Fs * ((Ts + 3) // 4) * steps
    whole = philox.normal(Bs, Fs, Ts, 1234, 2)
    for c in range(Bs):
        assert np.array_equal(philox.normal(c + 1, Fs, Ts, 1234, 2)[c], whole[c])
    # ... nor on the frame count beyond its own frames (the quad index is t >> 2 whatever T is)
    assert np.array_equal(philox.normal(Bs, Fs, 7, 1234, 2), whole[..., :7])
    # the generator's output is as distinct as its counters: no two elements of the block share a value by construction
    assert np.unique(philox.words(Bs, Fs, Ts, 1234, 2).reshape(4, -1), axis=1).shape[1] == Bs * Fs * ((Ts + 3) // 4)


# ------------------------------------------------------------------------------ the distribution at the headline shape
_N = {}


def draws(seed, step):
    if (seed, step) not in _N:
        _N[(seed, step)] = philox.normal(B, F, T, seed, step)
    return _N[(seed, step)]


def phi(x):
    return (0.5 * torch.erfc(torch.from_numpy(-x / math.sqrt(2.0)))).numpy()


STREAMS = [(1234, 0), (1234, 1), (1235, 0), (1234 + HI, 0)]


@pytest.mark.parametrize("seed,step", STREAMS, ids=[f"seed{s & 0xffffffff}{'+2^32' if s >> 32 else ''}-step{j}" for s, j in STREAMS])
def test_moments_ks_and_tails_at_the_headline_shape(seed, step):
    x = draws(seed, step).ravel()
    n = x.size
    assert n == B * F * T
    z_mean = x.mean() * math.sqrt(n)                                     # Var x = 1
    z_var = ((x * x).mean() - 1.0) / math.sqrt(2.0 / n)                    # Var x^2 = E x^4 - 1 = 2
    z_m4 = ((x ** 4).mean() - 3.0) / math.sqrt(96.0 / n)                   # Var x^4 = E x^8 - 9 = 105 - 9
    s = np.sort(x)
    cdf = phi(s)
    i = np.arange(1, n + 1, dtype=np.float64)
    ks = math.sqrt(n) * max(float((i / n - cdf).max()), float((cdf - (i - 1) / n).max()))
    p4 = math.erfc(4.0 / math.sqrt(2.0))                                   # P(|x| > 4) = 6.33e-5: ~209 of 3.3 M
    z_tail = (float((np.abs(x) > 4.0).sum()) - n * p4) / math.sqrt(n * p4 * (1.0 - p4))
    print(f"\nseed {seed} step {step}: z mean {z_mean:+.2f} var {z_var:+.2f} m4 {z_m4:+.2f} tail {z_tail:+.2f}; sqrt(n) D = {ks:.3f}; "
          f"max |x| = {np.abs(x).max():.4f}")
    assert max(abs(z_mean), abs(z_var), abs(z_m4), abs(z_tail)) < Z_BAR
    assert ks < KS_BAR
    assert np.abs(x).max() <= math.sqrt(48.0 * math.log(2.0))             # the mapping's largest radius


def corr_z(a, b):
    """z-score of the sample correlation of two unit-variance, zero-mean arrays under independence: mean(a b) sqrt(n)."""
    a, b = a.ravel(), b.ravel()
    return float((a * b).mean() * math.sqrt(a.size))


def test_neighbours_are_uncorrelated_along_every_counter_word_and_key_word():
    x = draws(1234, 0)
    z = {"t lag 1 (inside a counter and across)": corr_z(x[..., :-1], x[..., 1:]),
         "t lag 1, same Box-Muller pair": corr_z(x[..., 0::4], x[..., 1::4]),
         "t lag 2, the two pairs of a counter": corr_z(x[..., 0::4], x[..., 2::4]),
         "t lag 4 (next counter)": corr_z(x[..., :-4], x[..., 4:]),
         "f": corr_z(x[:, :-1], x[:, 1:]),
         "clip": corr_z(x[:-1], x[1:]),
         "step j / j + 1": corr_z(x, draws(1234, 1)),
         "seed s / s + 1": corr_z(x, draws(1235, 0)),
         "seed high word": corr_z(x, draws(1234 + HI, 0))}
    # squares too: a shared radius or a shared angle shows in x^2 where the plain correlation cancels
    c = lambda a: (a * a - 1.0) / math.sqrt(2.0)
    z.update({"squares, t lag 2": corr_z(c(x[..., 0::4]), c(x[..., 2::4])),
              "squares, step": corr_z(c(x), c(draws(1234, 1))),
              "squares, seed": corr_z(c(x), c(draws(1235, 0))),
              "squares, seed high word": corr_z(c(x), c(draws(1234 + HI, 0)))})
    print("\n" + "\n".join(f"  {k}: z = {v:+.2f}" for k, v in z.items()))
    assert all(abs(v) < Z_BAR for v in z.values()), z
    # (the two components of ONE Box-Muller pair share their radius: their squares are anti-correlated by construction -- cos^2 + sin^2
    # = 1 -- which is the property of the transform, not a defect, and is why "same pair" is tested on the values only)


# ------------------------------------------------------------------------------ per-rank keys
def test_rank_seed_distinct_for_16_ranks_and_64_passes():
    """rank * 7919 + pass: two (rank, pass) pairs meet only from pass 7919 on; the range the data-parallel driver uses is far inside."""
    from mst_amd.sharding import rank_seed
    for base in (0, 1234, 2 ** 31 - 2):
        keys = {rank_seed(base, r, p) for r in range(16) for p in range(64)}
        assert len(keys) == 16 * 64
        assert all(0 <= k < 1 << 63 for k in keys)
    assert rank_seed(7, 1, 0) == rank_seed(7, 0, 7919)           # the collision the docstring speaks of, stated
