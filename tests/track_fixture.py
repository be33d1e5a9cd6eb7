"""numpy restatement of the reference's pose-track path: `downsample` / `joints_downsample` / `amass_to_pose`
(utils/process_smpl_from_hybrik.py:56-180) over `qslerp`, `qpow`, `lerp` (data_loaders/humanml/common/quaternion.py:371-457), `q2axangle`
and `rotm2q` (common/rotation.py:163-250), the body model's first 22 joints (Rodrigues as tests/smplify_fixture.py states it, J = J0 +
Jdirs beta, the rigid chain) and the re-axing.

Nothing here imports the reference: bodies, tracks and lengths are generated from a seed.  Every function takes a dtype and runs in it,
so one set of inputs is evaluated in float64 (the oracle) and in float32 (the arithmetic the kernels use).  Two things stay double in
both, as in the kernels and in the reference: the parameter t (rounded once to `dtype` for the rotations) and the lerp of points and
translations (rounded to `dtype` at the end)."""
from fractions import Fraction

import numpy as np

PARENTS22 = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19]
SMPL_PARENTS = PARENTS22 + [20, 21]
CHAIN, NB = 22, 10
FLOOR = 1e-6
# (source frames, rate) -> output frames, as the reference's own functions returned them (tests/golden/track.npz holds the same counts)
COUNTS = {(2, Fraction(5, 4)): 1, (3, Fraction(3, 2)): 2, (9, Fraction(5, 4)): 7, (7, Fraction(3, 2)): 4, (6, Fraction(1)): 5,
          (5, Fraction(1, 2)): 8}


def distance(a, b):
    """max |a - b| over the largest magnitude of b."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)) if b.size else 0.0


def quat_distance(a, b):
    """The same, every quaternion of `a` first given the sign of its partner (q and -q are one rotation)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return distance(a * np.where((a * b).sum(-1, keepdims=True) < 0, -1.0, 1.0), b)


def bar(own):
    """4 x the float32 restatement's own distance from float64, floor 1e-6."""
    return max(4.0 * float(own), FLOOR)


# ------------------------------------------------------------------------------------------ the output-frame rule
def up_down(rate):
    """The reference's lcm arithmetic: rate num / den -> (up-sampling factor den, stride num)."""
    r = Fraction(rate)
    return r.denominator, r.numerator


def out_frames(length, rate):
    """ceil((L - 1) * up / down): the reference resamples intervals, so the source's last frame is dropped even at rate 1."""
    up, down = up_down(rate)
    return max(-(-(int(length) - 1) * up // down), 0)


def frame_params(length, rate):
    """-> (interval i [K], t [K] float64) of the K output frames; t is the reference's `np.linspace(0, 1, up + 1)` entry."""
    up, down = up_down(rate)
    k = np.arange(out_frames(length, rate), dtype=np.int64) * down
    return k // up, np.linspace(0, 1, up + 1)[k % up]


# ------------------------------------------------------------------------------------------ quaternions, (w, x, y, z)
def _norm(q):
    return np.sqrt((q * q).sum(-1, keepdims=True))


def qmul(a, b):
    a, b = np.broadcast_arrays(a, b)
    w = a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1] - a[..., 2] * b[..., 2] - a[..., 3] * b[..., 3]
    x = a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0] + a[..., 2] * b[..., 3] - a[..., 3] * b[..., 2]
    y = a[..., 0] * b[..., 2] - a[..., 1] * b[..., 3] + a[..., 2] * b[..., 0] + a[..., 3] * b[..., 1]
    z = a[..., 0] * b[..., 3] + a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1] + a[..., 3] * b[..., 0]
    return np.stack([w, x, y, z], -1)


def qinv(q):
    return q * np.array([1, -1, -1, -1], q.dtype)


def qpow(q, t):
    """quaternion.py:371-398 for one t per quaternion (t broadcasts over the leading axes)."""
    q = q / _norm(q)
    theta0 = np.arccos(q[..., :1])
    theta0 = np.where((theta0 <= 10e-10) & (theta0 >= -10e-10), q.dtype.type(10e-10), theta0)
    v0 = q[..., 1:] / np.sin(theta0)
    theta = t * theta0
    return np.concatenate([np.cos(theta), v0 * np.sin(theta)], -1)


def qslerp(q0, q1, t, shortest=False):
    """quaternion.py:403-418.  q0, q1 [..., 4]; t broadcastable to [..., 1], already in the quaternions' dtype.  shortest: the relative
    quaternion is negated where its w is negative (not in the reference)."""
    q0, q1 = q0 / _norm(q0), q1 / _norm(q1)
    rel = qmul(q1, qinv(q0))
    if shortest:
        rel = np.where(rel[..., :1] < 0, -rel, rel)
    return qmul(qpow(rel, t), q0)


def q2axangle(q):
    """rotation.py:234-250."""
    q = q / _norm(q)
    theta = np.arccos(q[..., :1]) * q.dtype.type(2)
    s = np.sin(theta / q.dtype.type(2))
    s = np.where(s == 0, q.dtype.type(0.1), s)
    return q[..., 1:] / s * theta


def rotm2q(R):
    """The dominant eigenvector of rotm2q's K matrix (rotation.py:163-206) in closed form on the largest of the four diagonal
    combinations; its sign is this form's (the reference's is LAPACK's)."""
    R = np.asarray(R)
    m = R.reshape(R.shape[:-2] + (9,))
    d = np.stack([m[..., 0] + m[..., 4] + m[..., 8], m[..., 0] - m[..., 4] - m[..., 8], m[..., 4] - m[..., 0] - m[..., 8],
                  m[..., 8] - m[..., 0] - m[..., 4]], -1)                                  # w, x, y, z
    pick = np.where((d[..., 0] >= d[..., 1]) & (d[..., 0] >= d[..., 2]) & (d[..., 0] >= d[..., 3]), 0,
                    np.where((d[..., 1] >= d[..., 2]) & (d[..., 1] >= d[..., 3]), 1, np.where(d[..., 2] >= d[..., 3], 2, 3)))
    one, two, quarter = R.dtype.type(1), R.dtype.type(2), R.dtype.type(0.25)
    s = two * np.sqrt(one + np.take_along_axis(d, pick[..., None], -1)[..., 0])
    a, b, c = m[..., 7] - m[..., 5], m[..., 2] - m[..., 6], m[..., 3] - m[..., 1]          # 4 w x, 4 w y, 4 w z
    xy, xz, yz = m[..., 1] + m[..., 3], m[..., 2] + m[..., 6], m[..., 5] + m[..., 7]
    forms = np.stack([np.stack([quarter * s, a / s, b / s, c / s], -1), np.stack([a / s, quarter * s, xy / s, xz / s], -1),
                      np.stack([b / s, xy / s, quarter * s, yz / s], -1), np.stack([c / s, xz / s, yz / s, quarter * s], -1)], -2)
    return np.take_along_axis(forms, pick[..., None, None], -2)[..., 0, :]


def q2rotm(q):
    q = q / _norm(q)
    r, i, j, k = (q[..., a] for a in range(4))
    m = np.stack([1 - 2 * (j * j + k * k), 2 * (i * j - k * r), 2 * (i * k + j * r), 2 * (i * j + k * r), 1 - 2 * (i * i + k * k),
                  2 * (j * k - i * r), 2 * (i * k - j * r), 2 * (j * k + i * r), 1 - 2 * (i * i + j * j)], -1)
    return m.reshape(q.shape[:-1] + (3, 3))


def rodrigues(theta):
    """tests/smplify_fixture.py's form: |theta + 1e-8|, K = skew(theta / angle), I + sin K + (1 - cos) K K, written out."""
    dt = theta.dtype.type
    e = theta + dt(1e-8)
    a = np.sqrt((e * e).sum(-1))
    x, y, z = (theta[..., c] / a for c in range(3))
    s, c1 = np.sin(a), dt(1) - np.cos(a)
    m = np.stack([dt(1) - c1 * (y * y + z * z), c1 * (x * y) - s * z, c1 * (x * z) + s * y,
                  c1 * (x * y) + s * z, dt(1) - c1 * (x * x + z * z), c1 * (y * z) - s * x,
                  c1 * (x * z) - s * y, c1 * (y * z) + s * x, dt(1) - c1 * (x * x + y * y)], -1)
    return m.reshape(theta.shape[:-1] + (3, 3))


# ------------------------------------------------------------------------------------------ resampling
def resample_quats(q, rate, dtype, length=None, shortest=False):
    """q [T, J, 4] -> [K, J, 4] in `dtype`."""
    q = np.asarray(q, dtype)
    i, t = frame_params(len(q) if length is None else length, rate)
    return qslerp(q[i], q[i + 1], t.astype(dtype)[:, None, None], shortest)


def resample_points(p, rate, dtype, length=None):
    """p [T, ..., 3] -> [K, ..., 3]: the lerp in double on the inputs as `dtype` holds them, rounded to `dtype` once."""
    p = np.asarray(p, dtype).astype(np.float64)
    i, t = frame_params(len(p) if length is None else length, rate)
    t = t.reshape((-1,) + (1,) * (p.ndim - 1))
    return (p[i] + t * (p[i + 1] - p[i])).astype(dtype)


def lerp64(p, rate, length=None, as_reference=False):
    """-> float64.  The kernels' lerp: everything in double.  as_reference: the reference's `lerp` on float32 input with its float64 `t`
    -- the difference p1 - p0 is formed in float32 before the product promotes to float64."""
    p = np.asarray(p)
    i, t = frame_params(len(p) if length is None else length, rate)
    t = t.reshape((-1,) + (1,) * (p.ndim - 1))
    if as_reference:
        return p[i].astype(np.float64) + t * (p[i + 1] - p[i]).astype(np.float64)
    p = p.astype(np.float64)
    return p[i] + t * (p[i + 1] - p[i])


# ------------------------------------------------------------------------------------------ the body's joints
def joint_table(body, num_betas=NB):
    """-> (J0 [22, 3], Jdirs [22, 3, 10]) float32, formed in double: what BodyJoints holds."""
    jr = np.asarray(body["J_regressor"], np.float64)[:CHAIN]
    J0 = jr @ np.asarray(body["v_template"], np.float64)
    Jd = np.einsum("jv,vci->jci", jr, np.asarray(body["shapedirs"], np.float64)[..., :num_betas])
    return J0.astype(np.float32), Jd.astype(np.float32)


def chain(R, J, parents=PARENTS22):
    """R [N, 22, 3, 3], J [22, 3] -> the posed joints [N, 22, 3]: G_R[j] = G_R[p] R[j], G_t[j] = G_R[p] (J[j] - J[p]) + G_t[p]."""
    GR, Gt = [R[:, 0]], [np.broadcast_to(J[0], (R.shape[0], 3))]
    for j in range(1, CHAIN):
        p = parents[j]
        GR.append(GR[p] @ R[:, j])
        Gt.append((GR[p] @ (J[j] - J[p])[None, :, None])[..., 0] + Gt[p])
    return np.stack(Gt, 1)


def reaxis(p):
    """np.dot(p, trans_matrix) with trans_matrix the x / z swap, then y negated."""
    return np.stack([p[..., 2], -p[..., 1], p[..., 0]], -1)


def track_joints(track, table, rate, dtype, with_trans=False, length=None, shortest=False, parents=PARENTS22):
    """One track -> (model joints [K, 22, 3], estimator joints [K, 22, 3] or None) in `dtype`.  track: dict with `quats` [T, >= 22, 4]
    or `mats` [T, >= 22, 3, 3], `transl` [T, 3], `betas` [10], optionally `joints` [T, >= 22, 3]; table: (J0, Jdirs)."""
    dt = np.dtype(dtype).type
    if "mats" in track:
        q, shortest = rotm2q(np.asarray(track["mats"], dtype)[:, :CHAIN]), True
    else:
        q = np.asarray(track["quats"], dtype)[:, :CHAIN]
    q = resample_quats(q, rate, dtype, length, shortest)
    R = rodrigues(q2axangle(q))
    J0, Jd = (np.asarray(a, dtype) for a in table)
    J = J0.copy()
    for n in range(NB):                                   # the kernel's chain of fused multiply-adds, term by term
        J = J + Jd[..., n] * dt(np.asarray(track["betas"], dtype)[n])
    pos = chain(R, J, parents).astype(np.float64)
    tr = lerp64(np.asarray(track["transl"], dtype), rate, length) if with_trans else np.zeros((len(pos), 3))
    model = reaxis(pos + tr[:, None]).astype(dtype)
    est = None
    if "joints" in track:
        e = lerp64(np.asarray(track["joints"], dtype)[:, :CHAIN], rate, length)
        est = reaxis(e + tr[:, None]).astype(dtype)
    return model, est


# ------------------------------------------------------------------------------------------ seeded inputs
def body(V=40, seed=7):
    """A synthetic body under SMPL's key names (an .npz of it is what BodyJoints.from_npz reads): 24 joints, V vertices."""
    g = np.random.default_rng([seed, V])
    vt = g.uniform(-1.0, 1.0, (V, 3)) * np.array([0.5, 1.0, 0.3])
    jr = np.zeros((24, V))
    for r in range(24):
        idx = g.choice(V, size=6, replace=False)
        w = g.uniform(0.1, 1.0, 6)
        jr[r, idx] = w / w.sum()
    kin = np.stack([np.array([2 ** 32 - 1] + SMPL_PARENTS[1:], np.int64), np.arange(24)])
    return {"v_template": vt, "shapedirs": g.standard_normal((V, 3, 16)) * 1e-2, "J_regressor": jr, "kintree_table": kin}


def random_quats(g, shape, angle=(0.3, 1.2)):
    axis = g.standard_normal(shape + (3,))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    half = g.uniform(*angle, shape + (1,)) / 2
    return np.concatenate([np.cos(half), np.sin(half) * axis], -1)


def track(seed, T, J=24, flips=False, matrices=False, estimator=True):
    """A seeded track: per joint a rotation that drifts by 0.05 .. 0.4 rad a frame about a slowly turning axis (the relative rotation of
    an interval stays well inside (0, pi)), quaternions scaled off unit length, a drifting root and per-frame shapes.  flips: every
    third quaternion negated (the same rotations, the longer arc under the reference's formula)."""
    g = np.random.default_rng([seed, T, J])
    q = [random_quats(g, (J,))]
    for _ in range(T - 1):
        q.append(qmul(random_quats(g, (J,), (0.05, 0.4)), q[-1]))
    q = np.stack(q)
    if flips:
        sign = np.where(g.integers(0, 3, (T, J, 1)) == 0, -1.0, 1.0)
        sign[0] = 1.0
        q = q * sign
    shape = (g.standard_normal((T, NB)) * 0.5).astype(np.float32)
    out = {"transl": np.cumsum(g.standard_normal((T, 3)) * 0.05, 0) + np.array([0.1, 0.9, 3.0]), "shape": shape, "betas": shape.mean(0)}
    if matrices:
        out["mats"] = q2rotm(q)
    else:
        out["quats"] = q * g.uniform(0.8, 1.25, (T, J, 1))
    if estimator:
        out["joints"] = g.standard_normal((T, J, 3)) * 0.4
    return {k: v.astype(np.float32) for k, v in out.items()}


def lengths(seed, B, T):
    """Mixed lengths for a batch: the full clip first, a clip of 2 second, the rest from the seed."""
    g = np.random.default_rng([seed, B, T])
    n = g.integers(2, T + 1, B)
    n[0], n[1 % B] = T, 2 if B > 1 else T
    return n.astype(np.int32)


# ------------------------------------------------------------------------------------------ the estimator's files
def write_track(path, tr, kind):
    """A seeded track as one of the three files `amass_to_pose` reads, under the reference's key names.  kind: 'pt', 'pk' or 'pkl'."""
    import pickle
    import torch
    T = len(tr["transl"])
    if kind == "pt":
        torch.save([{"pred_theta_mats": torch.from_numpy(tr["mats"].reshape(T, -1)), "pred_shape": torch.from_numpy(tr["shape"]),
                     "pred_xyz_jts_24_struct": torch.from_numpy(tr["joints"].reshape(T, -1)), "transl": torch.from_numpy(tr["transl"])}], path)
        return
    if kind == "pk":
        d = {"pred_thetas": tr["mats"].reshape(T, -1), "pred_betas": tr["shape"], "pred_xyz_24_struct": tr["joints"], "transl": tr["transl"]}
    elif kind == "pkl":
        d = [{"smpl_pose_quat_wroot": tr["quats"], "smpl_beta": tr["shape"], "root_trans": tr["transl"]}]
    else:
        raise KeyError(kind)
    with open(path, "wb") as fh:
        pickle.dump(d, fh)


def write_trans(path, transl):
    import pickle
    with open(path, "wb") as fh:
        pickle.dump([{"root_trans": np.asarray(transl, np.float32)}], fh)


# name -> (file kind, source frames, fps, with_trans, rows of a separate translation file or 0): what tests/golden/track.npz holds of
# `amass_to_pose`
GOLDEN_FILES = {"pk25": ("pk", 9, 25, False, 0), "pk25t": ("pk", 9, 25, True, 0), "pkl30t": ("pkl", 7, 30, True, 0),
                "pt30cut": ("pt", 9, 30, True, 7)}
SEED = 20261021


def golden_track(name):
    kind, T, _, _, cut = GOLDEN_FILES[name]
    tr = track(SEED + len(name), T, flips=kind == "pkl", matrices=kind != "pkl", estimator=kind != "pkl")
    extra = None
    if cut:
        extra = (np.random.default_rng([SEED, cut]).standard_normal((cut, 3)) * 0.3).astype(np.float32)
    return tr, extra


def as_case(pose_track):
    """A PoseTrack (read_pose_track) -> the dict `track_joints` above takes."""
    d = {"transl": np.asarray(pose_track.transl, np.float32), "betas": np.asarray(pose_track.betas, np.float32)}
    if pose_track.matrices is not None:
        d["mats"] = np.asarray(pose_track.matrices, np.float32)
    else:
        d["quats"] = np.asarray(pose_track.rotations, np.float32)
    if pose_track.joints is not None:
        d["joints"] = np.asarray(pose_track.joints, np.float32)
    return d


# ------------------------------------------------------------------------------------------ a humanoid in HumanML3D's joint order
T2M_CHAINS = [[0, 2, 5, 8, 11], [0, 1, 4, 7, 10], [0, 3, 6, 9, 12, 15], [9, 14, 17, 19, 21], [9, 13, 16, 18, 20]]
T2M_FACE, T2M_FID_L, T2M_FID_R, T2M_LEGS = (2, 1, 17, 16), (7, 10), (8, 11), (5, 8)
_X, _Y, _Z = np.eye(3)
# bone directions of a standing figure that faces +z with its left side on +x, and bone lengths in metres: hips, knees, ankles, toes;
# three spine bones, neck, head; collars, shoulders, elbows, wrists
HUMAN_DIRS = np.array([0 * _X, _X, -_X, _Y, -_Y, -_Y, _Y, -_Y, -_Y, _Y, _Z, _Z, _Y, _X, -_X, _Z, -_Y, -_Y, -_Y, -_Y, -_Y, -_Y])
HUMAN_LENGTHS = np.array([0, 0.10, 0.10, 0.12, 0.40, 0.40, 0.13, 0.41, 0.41, 0.06, 0.15, 0.15, 0.21, 0.12, 0.12, 0.10, 0.11, 0.11, 0.26, 0.26,
                          0.25, 0.25])


def human(scale=1.0):
    """-> encode_fixture.Skeleton of the figure; its `raw` are the unit bone directions."""
    import encode_fixture as ef
    return ef.Skeleton(T2M_CHAINS, T2M_FACE, T2M_FID_L, T2M_FID_R, HUMAN_DIRS * HUMAN_LENGTHS[:, None] * scale)


def human_clip(tag, T, scale=1.0):
    """[T, 22, 3] float32: the figure moving, clear of every discontinuity of `process_file` (encode_fixture.make_clip)."""
    import encode_fixture as ef
    return ef.make_clip(SEED, f"track/{tag}", T, human(scale), ef.HML, scale=scale)[0][0]


def hml_rows(joints, tgt_offsets, dtype):
    """`pos2hmlrep` restated: bvh_fixture.retarget, then encode_fixture.encode_clip in HML mode -> [T - 1, 263]."""
    import bvh_fixture as bf
    import encode_fixture as ef
    sk = human()
    moved, _ = bf.retarget(np.asarray(joints, np.float32), tgt_offsets, sk.raw, sk.chains, list(T2M_LEGS), sk.face, dtype)
    return ef.encode_clip(moved.astype(np.float32), None, sk, ef.HML, dtype, 0.002)[0]
