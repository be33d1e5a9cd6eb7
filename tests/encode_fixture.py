"""numpy restatement of the reference's motion encoders: `process_file_with_rotation` (data_loaders/humanml/common/bvh_utils.py:1091-1287,
mode "posrot", 9 J + 1 columns) and `process_file` (:898-1088, mode "hml", 12 J - 1 columns) with the smoothed root rotation and the chain
IK of `Skeleton.inverse_kinematics_np` (common/skeleton.py:55-103), the z-normalisation and zero padding of `process_np_motion`
(data_loaders/humanml/data/dataset.py:484-519), and `recover_from_ric` (bvh_utils.py:1299-1363) for the round trip.

Nothing here imports the reference and no table is taken from it: skeletons and clips are generated from a seed.  Every function takes a
dtype; the whole evaluation -- the 161-tap filter included -- runs in it, so one set of inputs can be evaluated in float32 and in float64.

One stated deviation from the reference, shared with the kernel: the arcsin argument of the root's angular velocity is clipped into
[-1, 1].  `assert_clear` keeps every test input away from the discontinuities of the computation (see its docstring)."""
import numpy as np

import ik_fixture as ik
import mst_amd.synthetic as syn

POSROT, HML = "posrot", "hml"
SIGMA, RADIUS = 20.0, 80
FEET_THRE = 0.002
# (mode, joints, frames) of the cases tests/golden/encode.npz holds
GOLDEN_CASES = ((POSROT, 20, 76), (POSROT, 21, 197), (HML, 22, 197), (HML, 22, 5))
rel, bar = ik.rel, ik.bar


def golden_frames(name, n):
    """The frames of a reference output tests/golden/encode.npz keeps (the file stays under 500 KiB)."""
    every = {"global_positions": 2, "recover": 4, "positions": n}.get(name, 1)
    return sorted(set(range(0, n, every)) | {n - 1})


def feats(J, mode):
    return 9 * J + 1 if mode == POSROT else 12 * J - 1


# ------------------------------------------------------------------------------------------ quaternions, (w, x, y, z)
def _cross(a, b):
    a, b = np.broadcast_arrays(a, b)
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _norm(a):
    return np.sqrt((a * a).sum(-1, keepdims=True))


def qinv(q):
    return q * np.array([1, -1, -1, -1], q.dtype)


def qmul(a, b):
    a, b = np.broadcast_arrays(a, b)
    w = a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1] - a[..., 2] * b[..., 2] - a[..., 3] * b[..., 3]
    x = a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0] + a[..., 2] * b[..., 3] - a[..., 3] * b[..., 2]
    y = a[..., 0] * b[..., 2] - a[..., 1] * b[..., 3] + a[..., 2] * b[..., 0] + a[..., 3] * b[..., 1]
    z = a[..., 0] * b[..., 3] + a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1] + a[..., 3] * b[..., 0]
    return np.stack([w, x, y, z], -1)


def qrot(q, v):
    """quaternion.py:88-99."""
    u = q[..., 1:]
    uv = _cross(u, v)
    uuv = _cross(u, uv)
    return v + q.dtype.type(2) * (q[..., :1] * uv + uuv)


def qbetween(v0, v1):
    """quaternion.py:421-431 (and rotation.py:97-108, the same expression).  -> (q, w / |(w, v)| before normalisation)."""
    v0, v1 = np.broadcast_arrays(v0, v1)
    v = _cross(v0, v1)
    w = np.sqrt((v0 * v0).sum(-1, keepdims=True) * (v1 * v1).sum(-1, keepdims=True)) + (v0 * v1).sum(-1, keepdims=True)
    q = np.concatenate([w, v], -1)
    n = _norm(q)
    return q / n, (w / n)[..., 0]


def _two_columns(q, two):
    r, i, j, k = (q[..., a] for a in range(4))
    one = q.dtype.type(1)
    return np.stack([one - two * (j * j + k * k), two * (i * j + k * r), two * (i * k - j * r),
                     two * (i * j - k * r), one - two * (i * i + k * k), two * (j * k + i * r)], -1)


def q2cont6d(q):
    """rotation.py:766-769 over q2rotm (:139-160): q as it is."""
    return _two_columns(q, q.dtype.type(2))


def quaternion_to_cont6d(q):
    """quaternion.py:335-338 over quaternion_to_matrix (:300-327): q normalised, then 2 / |q_n|^2."""
    qn = q / _norm(q)
    return _two_columns(qn, q.dtype.type(2) / (qn * qn).sum(-1))


# ------------------------------------------------------------------------------------------ the filter
def taps():
    """scipy.ndimage's _gaussian_kernel1d(sigma 20, order 0, radius int(4 * 20 + 0.5)): 161 normalised weights, float64."""
    x = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)
    phi = np.exp(-0.5 / (SIGMA * SIGMA) * x ** 2)
    return phi / phi.sum()


def smooth(x, dtype):
    """gaussian_filter1d(x, 20, axis=0, mode='nearest') in `dtype`: the clip extended by its edge rows, one product with the window
    matrix."""
    x = np.asarray(x, dtype)
    n = x.shape[0]
    ext = np.concatenate([np.repeat(x[:1], RADIUS, 0), x, np.repeat(x[-1:], RADIUS, 0)], 0)
    windows = np.lib.stride_tricks.sliding_window_view(ext, 2 * RADIUS + 1, axis=0)          # [n, C, 161]
    assert windows.shape[0] == n
    w = taps().astype(dtype)
    out = np.zeros(x.shape, dtype)
    for k in range(2 * RADIUS + 1):
        out = out + w[k] * windows[..., k]
    return out


# ------------------------------------------------------------------------------------------ one clip
class Skeleton:
    """chains, face joints (r_hip, l_hip, sdr_r, sdr_l), fid_l, fid_r, raw unit offsets [J, 3] (HML), bone offsets [J, 3] (clip making)."""

    def __init__(self, chains, face, fid_l, fid_r, offsets):
        self.chains, self.face, self.fid_l, self.fid_r = [list(c) for c in chains], list(face), list(fid_l), list(fid_r)
        self.offsets = np.asarray(offsets, np.float64)
        self.J = len(self.offsets)
        self.parents = ik.parents_of(self.chains, self.J)
        n = np.linalg.norm(self.offsets, axis=-1, keepdims=True)
        self.raw = np.where(n > 0, self.offsets / np.maximum(n, 1e-300), 0.0).astype(np.float32)
        self.raw[0] = 0

    def kw(self):
        return dict(chains=self.chains, raw_offsets=self.raw, face_joint_indx=self.face, fid_l=self.fid_l, fid_r=self.fid_r)


def encode_clip(positions, rotations, sk, mode, dtype=np.float32, feet_thre=FEET_THRE, restart=True):
    """One clip [T, J, 3] (and rotations [T, J, 4] in POSROT) -> (data [T-1, F], global_positions [T, J, 3], positions [T, J, 3],
    l_velocity [T-1, 2], diag).  restart=False: the chain IK accumulates R down the tree instead of restarting every chain from the root
    quaternion -- NOT what the reference does; the chain test tells the two apart.  diag: what `assert_clear` looks at."""
    dt = np.dtype(dtype).type
    pos = np.array(positions, dtype)
    T, J = pos.shape[:2]
    r_hip, l_hip, sdr_r, sdr_l = sk.face
    diag = {}
    pos[:, :, 1] -= pos[:, :, 1].min()
    init = pos[0].copy()
    pos = pos - init[0] * np.array([1, 0, 1], dtype)
    across = (init[r_hip] - init[l_hip]) + (init[sdr_r] - init[sdr_l])
    n0 = _norm(across)
    across = across / n0
    fwd = np.array([across[2], 0, -across[0]], dtype)
    fwd = fwd / _norm(fwd)
    z = np.array([0, 0, 1], dtype)
    qi, w0 = qbetween(fwd, z)
    pos = qrot(qi, pos)
    glob = pos.copy()
    # the root rotation (skeleton.py:55-86, smooth_forward=True)
    ac = (pos[:, r_hip] - pos[:, l_hip]) + (pos[:, sdr_r] - pos[:, sdr_l])
    n1 = _norm(ac)
    ac = ac / n1
    fw = smooth(np.stack([ac[:, 2], np.zeros(T, dtype), -ac[:, 0]], -1), dtype)
    n2 = _norm(fw)
    fw = fw / n2
    rq, w1 = qbetween(z, fw)
    rq[0] = (1, 0, 0, 0)
    diag.update(across=np.concatenate([n0, n1[:, 0]]), smoothed=n2[:, 0], qbetween_w=np.concatenate([[w0], w1[1:]]))
    # root velocities
    vel = qrot(qinv(rq[1:]), pos[1:, 0] - pos[:-1, 0])
    rv = qmul(rq[1:], qinv(rq[:-1]))[:, 2]
    diag["asin"] = rv.copy()
    rot_vel = np.arcsin(np.clip(rv, dt(-1), dt(1)))
    lvel = vel[:, [0, 2]]
    # local pose
    local = pos.copy()
    local[..., 0] -= pos[:, 0:1, 0]
    local[..., 2] -= pos[:, 0:1, 2]
    local = qrot(qinv(rq)[:, None], local)
    cols = [rot_vel[:, None], lvel, local[:-1, 0, 1:2], local[:-1, 1:].reshape(T - 1, -1)]
    if mode == POSROT:
        rot = np.array(rotations, dtype)
        rot[:, 0] = qmul(qinv(rq), qmul(qi, rot[:, 0]))
        cols.append(quaternion_to_cont6d(rot).reshape(T, -1)[:-1])
    else:
        quats = np.zeros((T, J, 4), dtype)
        Rg = {0: rq}
        bones, ws = [], []
        raw = np.asarray(sk.raw, dtype)
        for chain in sk.chains:
            R = rq if restart else Rg[chain[0]]
            for a, c in zip(chain[:-1], chain[1:]):
                v = pos[:, c] - pos[:, a]
                nv = _norm(v)
                bones.append(nv[:, 0])
                quv, w = qbetween(raw[c][None], v / nv)
                ws.append(w)
                loc = qmul(qinv(R), quv)
                quats[:, c] = loc
                R = qmul(R, loc)
                Rg[c] = R
        diag["bones"] = np.concatenate(bones)
        diag["qbetween_w"] = np.concatenate([diag["qbetween_w"]] + ws)
        cols.append(q2cont6d(quats)[:-1, 1:].reshape(T - 1, -1))
        cols.append(qrot(qinv(rq[:-1])[:, None], glob[1:] - glob[:-1]).reshape(T - 1, -1))
        feet = sk.fid_l + sk.fid_r
        d = glob[1:, feet] - glob[:-1, feet]
        d2 = (d[..., 0] ** 2 + d[..., 1] ** 2) + d[..., 2] ** 2
        diag["feet"] = d2
        cols.append((d2 < dt(feet_thre)).astype(dtype))
    data = np.concatenate(cols, -1).astype(dtype)
    assert data.shape == (T - 1, feats(J, mode))
    return data, glob, local, lvel, diag


def encode(positions, rotations, sk, mode, dtype=np.float32, lengths=None, mean=None, std=None, frames_out=None, feet_thre=FEET_THRE,
           restart=True):
    """The batch: positions [B, T, J, 3] -> dict(sample [B, F, 1, frames_out], lengths int32 [B], global_positions, positions [B, T, J, 3],
    l_velocity [B, T-1, 2]; zero past a clip), and the per-clip diags."""
    positions = np.asarray(positions)
    B, T, J = positions.shape[:3]
    fo = T if frames_out is None else frames_out
    F = feats(J, mode)
    out = dict(sample=np.zeros((B, F, 1, fo), dtype), lengths=np.zeros(B, np.int32), global_positions=np.zeros((B, T, J, 3), dtype),
               positions=np.zeros((B, T, J, 3), dtype), l_velocity=np.zeros((B, T - 1, 2), dtype))
    diags = []
    for b in range(B):
        n = T if lengths is None else int(lengths[b])
        data, glob, local, lvel, diag = encode_clip(positions[b, :n], None if rotations is None else rotations[b, :n], sk, mode, dtype,
                                                    feet_thre, restart)
        if mean is not None:
            data = (data - np.asarray(mean, dtype)) / np.asarray(std, dtype)
        rows = min(n - 1, fo)
        out["sample"][b, :, 0, :rows] = data[:rows].T
        out["lengths"][b] = rows
        out["global_positions"][b, :n], out["positions"][b, :n], out["l_velocity"][b, :n - 1] = glob, local, lvel
        diags.append(diag)
    return out, diags


def recover_from_ric(data, J, dtype=np.float32):
    """bvh_utils.py:1299-1363 on rows [T, F]: r_rot_quat = (cos a, 0, sin a, 0) of the running sum of the yaw velocity, applied as it is."""
    data = np.asarray(data, dtype)
    T = data.shape[0]
    ang = np.zeros(T, dtype)
    ang[1:] = np.cumsum(data[:-1, 0], dtype=dtype)
    q = np.zeros((T, 4), dtype)
    q[:, 0], q[:, 2] = np.cos(ang), np.sin(ang)
    step = np.zeros((T, 3), dtype)
    step[1:, 0], step[1:, 2] = data[:-1, 1], data[:-1, 2]
    r_pos = np.cumsum(qrot(q, step), 0, dtype=dtype)
    r_pos[:, 1] = data[:, 3]
    p = qrot(q[:, None], data[:, 4:4 + 3 * (J - 1)].reshape(T, J - 1, 3))
    p[..., 0] += r_pos[:, 0:1]
    p[..., 2] += r_pos[:, 2:3]
    return np.concatenate([r_pos[:, None], p], 1)


# ------------------------------------------------------------------------------------------ clearance
def clear(diags, mode, feet_thre=FEET_THRE):
    """-> None, or what sits on a discontinuity."""
    for b, d in enumerate(diags):
        if d["across"].min() <= 1e-3:
            return f"clip {b}: |across| {d['across'].min():.3g} <= 1e-3"
        if d["smoothed"].min() <= 0.1:
            return f"clip {b}: smoothed forward of norm {d['smoothed'].min():.3g} <= 0.1"
        if d["qbetween_w"].min() <= 1e-2:
            return f"clip {b}: a qbetween with w / norm {d['qbetween_w'].min():.3g} <= 1e-2 (a half turn)"
        if np.abs(d["asin"]).max() >= 0.99:
            return f"clip {b}: arcsin argument {np.abs(d['asin']).max():.3g} >= 0.99"
        if mode == HML:
            if d["bones"].min() <= 1e-3:
                return f"clip {b}: a bone of length {d['bones'].min():.3g} <= 1e-3"
            gap = np.abs(d["feet"] - feet_thre).min() / feet_thre if d["feet"].size else 1.0
            if gap <= 0.01:
                return f"clip {b}: a foot's squared displacement within {gap:.3g} of feet_thre"
    return None


def assert_clear(diags, mode, feet_thre=FEET_THRE):
    """Fails (never skips) when an input sits on a discontinuity: |across| and, in HML, every bone length > 1e-3; the norm of the
    smoothed forward > 0.1; the w of every qbetween before normalisation > 1e-2 x its norm; |arcsin argument| < 0.99; every foot's squared
    displacement farther than 1 % of feet_thre from it.  diags: of the float64 evaluation."""
    why = clear(diags, mode, feet_thre)
    assert why is None, why


# ------------------------------------------------------------------------------------------ skeletons and clips
def skeleton(seed, J, scale=1.0):
    """J >= 19: ik_fixture.humanoid -- legs 1-4 (+x) and 5-8 (-x), a spine, two arms; the -x side is the right one, so that the character
    faces +z.  J = 5: a tiny tree with one mid-tree chain (it starts at joint 1)."""
    if J == 5:
        chains = [[0, 1, 2], [0, 3], [1, 4]]
        off = np.array([[0, 0, 0], [-0.2, 0.1, 0.02], [0.03, 0.3, 0.05], [0.2, 0.1, -0.02], [-0.25, 0.2, 0.01]]) * scale
        return Skeleton(chains, (1, 3, 4, 2), (3, 2), (1, 4), off)
    chains, _, off = ik.humanoid(seed, J, scale)
    off = off.astype(np.float64)
    off[0] = 0
    a0 = chains[3][1]
    return Skeleton(chains, (5, 1, a0 + 4, a0), (3, 4), (7, 8), off)


def _axis_angle(axis, ang):
    axis = axis / np.linalg.norm(axis, axis=-1, keepdims=True)
    return np.concatenate([np.cos(ang / 2)[..., None], axis * np.sin(ang / 2)[..., None]], -1)


def _clip(seed, tag, T, sk, B, scale, pace=1.0, gated=False):
    J = sk.J
    t = np.arange(T)[None, :, None]
    ph = 6.28 * syn.uniform01(seed, tag + "/ph", B * J * 2).reshape(2, B, 1, J)
    amp = 0.1 + 0.35 * syn.uniform01(seed, tag + "/amp", B * J).reshape(B, 1, J)
    freq = np.where(np.arange(J) < 9, 0.05 * pace, 0.13)[None, None, :]          # the legs swing slowly: few crossings of the contact threshold
    ang = amp * np.sin(freq * t + ph[0]) + 0.2 * np.sin(np.where(np.arange(J) < 9, 0.041 * pace, 0.041)[None, None, :] * t + ph[1])
    axis = syn.normal(seed, tag + "/axis", (B, 1, J, 3)).astype(np.float64) + 0.3 * np.sin(0.07 * t[..., None] + ph[1][..., None])
    q = _axis_angle(axis, ang)
    yaw0 = 1.6 * (syn.uniform01(seed, tag + "/yaw", B) - 0.5)
    yaw = yaw0[:, None] + 0.5 * np.sin(0.045 * pace * t[..., 0] + ph[0][:, :, 0]) + 0.004 * t[..., 0]
    q[:, :, 0] = _axis_angle(np.broadcast_to(np.array([0.05, 1.0, 0.03]), (B, T, 3)), yaw)
    speed = 0.015 + 0.045 * (0.5 + 0.5 * np.sin(0.06 * pace * t[..., 0] + ph[1][:, :, 0]))
    if gated:                                                          # stand or stride, with a steep switch between the two
        speed = 0.006 + 0.10 * 0.5 * (1 + np.tanh(6 * np.sin(0.06 * pace * t[..., 0] + ph[1][:, :, 0])))
    step = np.stack([np.sin(yaw) * speed, np.broadcast_to(0.01 * np.sin(0.2 * pace * t[..., 0]), yaw.shape), np.cos(yaw) * speed], -1) * scale
    root = np.cumsum(step, 1) + np.array([0.4, 0.95, -0.3]) * scale + syn.normal(seed, tag + "/root", (B, 1, 3)) * scale
    pos = np.zeros((B, T, J, 3))
    G = [None] * J
    pos[:, :, 0], G[0] = root, q[:, :, 0]
    for chain in sk.chains:
        for a, c in zip(chain[:-1], chain[1:]):
            pos[:, :, c] = pos[:, :, a] + qrot(G[a], np.broadcast_to(sk.offsets[c], (B, T, 3)))
            G[c] = qmul(G[a], q[:, :, c])
    return pos.astype(np.float32), q.astype(np.float32)


def make_clip(seed, tag, T, sk, mode, B=1, scale=1.0, lengths=None, feet_thre=FEET_THRE, pace=1.0, gated=False):
    """-> (positions [B, T, J, 3], rotations [B, T, J, 4]) float32: forward kinematics of smooth random joint rotations over a root that
    drifts and turns.  Per clip the first variant of the tag whose float64 evaluation is clear of every discontinuity (`clear`), at the
    clip's length, is taken; the tests assert it again on what they run.  pace < 1 slows the legs, the turning and the speed changes down:
    fewer crossings of the contact threshold; gated: the root either nearly stands or strides, so that a foot's displacement is far below
    or far above the threshold except in the frame or two between -- with both a long HML clip has clear variants at all."""
    clips = []
    for b in range(B):
        n = T if lengths is None else int(lengths[b])
        for variant in range(200):
            pos, rot = _clip(seed, f"{tag}/b{b}/v{variant}" if b else f"{tag}/v{variant}", T, sk, 1, scale, pace, gated)
            why = clear(encode(pos[:, :n], rot[:, :n], sk, mode, np.float64, feet_thre=feet_thre)[1], mode, feet_thre)
            if why is None:
                break
        else:
            raise AssertionError(f"{tag}: no variant of clip {b} is clear of the discontinuities: {why}")
        clips.append((pos, rot))
    return np.concatenate([c[0] for c in clips]), np.concatenate([c[1] for c in clips])


def golden_inputs(seed, mode, J, T):
    """The skeleton and clip of one golden case: Xia-sized bones at J = 20, larger ones (Bandai's scale) at 21, HumanML's count at 22."""
    scale = 6.0 if J == 21 else 1.0
    sk = skeleton(seed, J, scale)
    pos, rot = make_clip(seed, f"enc/golden/{mode}/J{J}T{T}", T, sk, mode, scale=scale)
    return sk, pos[0], rot[0]
