"""Oracle: the engine's counter-based Gaussian noise, in numpy float64.  (test infrastructure)

The contract restated here is the one include/mst_engine.h gives for MST_NOISE_PHILOX / mst_philox_normal and the comment above
`philox4x32_10` in csrc/mst_common.h, with the generator itself taken from its publication (Salmon, Moraes, Dror, Shaw: "Parallel
random numbers: as easy as 1, 2, 3", SC'11; Random123's philox4x32 with 10 rounds):

  round     (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0))
            M0 = 0xD2511F53, M1 = 0xCD9E8D57, hi / lo = the halves of the 64-bit product;
  key       the round keys advance by the Weyl constants (k0, k1) += (0x9E3779B9, 0xBB67AE85) mod 2^32 BETWEEN rounds: ten rounds
            use ten keys, the first of which is the caller's;
  element   (clip, f, t) of step `step` is component t & 3 of the four normals made from counter (t >> 2, f, clip, step) under key
            (seed & 0xffffffff, seed >> 32): one counter serves four consecutive frames;
  uniforms  from the top 24 bits of each word: u0, u2 = ((r >> 8) + 1) / 2^24 in (0, 1] (the radius: never log 0),
            u1, u3 = (r >> 8) / 2^24 in [0, 1) (the angle, in revolutions);
  normals   Box-Muller: (R0 cos 2 pi u1, R0 sin 2 pi u1, R2 cos 2 pi u3, R2 sin 2 pi u3), R = sqrt(-2 ln u).

Everything up to the uniforms is integer arithmetic and exact in both implementations (a 24-bit integer times 2^-24 is a float32);
the kernel then evaluates log2 / sqrt / sin / cos with the hardware's approximations in float32, this file in float64.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
ROUNDS = 10
MASK32 = 0xFFFFFFFF


def _u64(a):
    return np.asarray(a, dtype=np.uint64) & np.uint64(MASK32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of counters (c0..c3) under key (k0, k1); arrays broadcast against each other.  Returns four uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(_u64(c0), _u64(c1), _u64(c2), _u64(c3))
    k0, k1 = int(k0) & MASK32, int(k1) & MASK32
    lo, sh = np.uint64(MASK32), np.uint64(32)
    for _ in range(ROUNDS):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                 # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ np.uint64(k0), p1 & lo, (p0 >> sh) ^ c3 ^ np.uint64(k1), p0 & lo
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def uniforms(r0, r1, r2, r3):
    """The four float64 uniforms of one counter's words: (u0, u2) in (0, 1] for the radii, (u1, u3) in [0, 1) for the angles."""
    q = [(np.asarray(r, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) for r in (r0, r1, r2, r3)]
    s = 1.0 / 16777216.0
    return (q[0] + 1.0) * s, q[1] * s, (q[2] + 1.0) * s, q[3] * s


def box_muller(u0, u1, u2, u3):
    """Four normals of one counter, in the component order the kernels store them (frames 4 q .. 4 q + 3)."""
    ra, rb = np.sqrt(-2.0 * np.log(u0)), np.sqrt(-2.0 * np.log(u2))
    a, b = 2.0 * np.pi * u1, 2.0 * np.pi * u3
    return ra * np.cos(a), ra * np.sin(a), rb * np.cos(b), rb * np.sin(b)


def key(seed):
    seed = int(seed)
    assert 0 <= seed < 1 << 64
    return seed & MASK32, seed >> 32


def counters(batch, feats, frames, step, clip0=0):
    """Counter words of every (clip, feature, frame quad) of one step: four arrays broadcastable to [batch, feats, ceil(frames / 4)]."""
    tq = np.arange((frames + 3) // 4, dtype=np.uint64)[None, None, :]
    f = np.arange(feats, dtype=np.uint64)[None, :, None]
    clip = (np.arange(batch, dtype=np.uint64) + np.uint64(clip0))[:, None, None]
    return tq, f, clip, np.uint64(int(step) & MASK32)


def words(batch, feats, frames, seed, step, clip0=0):
    """The raw generator output: uint32 [4, batch, feats, ceil(frames / 4)]."""
    return np.stack(philox4x32_10(*counters(batch, feats, frames, step, clip0), *key(seed)))


def planes(batch, feats, frames, seed, step):
    """(normal, radius uniform, angle uniform) of every element, each float64 [batch, feats, frames], from one pass of the generator."""
    u0, u1, u2, u3 = uniforms(*words(batch, feats, frames, seed, step))
    cut = lambda parts: np.ascontiguousarray(np.stack(parts, axis=-1).reshape(batch, feats, -1)[..., :frames])
    return cut(box_muller(u0, u1, u2, u3)), cut([u0, u0, u2, u2]), cut([u1, u1, u3, u3])


def uniform_planes(batch, feats, frames, seed, step):
    """(radius uniform, angle uniform) of every element: what `normal` is made from (tests select elements by them, e.g. the
    angles where sin / cos cross zero)."""
    return planes(batch, feats, frames, seed, step)[1:]


def normal(batch, feats, frames, seed, step):
    """float64 [batch, feats, frames]: the standard normals of step `step` under `seed`."""
    return planes(batch, feats, frames, seed, step)[0]
