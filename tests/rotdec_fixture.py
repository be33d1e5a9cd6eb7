"""numpy restatement of the reference's rotation-channel decoders (data_loaders/humanml/common/bvh_utils.py): `recover_root_rot_pos`
(:1299-1318), `output_bvh` (:1382-1441), `recover_from_rot` (:1321-1335), `output_bvh_from_real_rot` (:1538-1563),
`recover_from_real_rot` (:1337-1345), `process_pos_from_real_rot` (:1366-1378), and of the skeleton `output_bvh` writes (`expand_chains`).
`output_bvh_with_pos` (:1444-1511) over `Skeleton.inverse_kinematics_np(smooth_forward=True)` (common/skeleton.py:55-103) is `pos_ik`.

Nothing here imports the reference and no table is taken from it: trees, offsets and rows are generated from a seed.  Every function takes
a dtype and runs in it, so one set of inputs can be evaluated in the reference's precision (float32) and in float64.  The small vector
helpers are ik_fixture's (they round fp32 as torch's CPU kernels do).

`make_rows` keeps every 6D block's rotation angle ANGLE_MARGIN away from 0 and pi (`ik_fixture.assert_angles_clear`: cont6d2q divides by
sin theta) except ONE joint whose block is exactly the identity, which takes the reference's theta = 0 branch: its quaternion is exactly
(1, 0, 0, 0)."""
import math
from copy import deepcopy

import numpy as np

import ik_fixture as ik
import mst_amd.synthetic as syn

SEED = 20261003                              # tests/golden/make_golden.py's: the goldens were made from it
FLOOR = ik.FLOOR                             # 1e-6, the floor of the BVH and fit tests' bars
HML, REAL, POS = "hml_rot", "real_rot", "pos_ik"
ROUTES = (HML, REAL, POS)
TREES = ("tree3", "t2m22", "mid21")
FRAMES = (1, 2, 63, 64, 65, 255, 256, 257)   # scan edges: wave and workgroup strides
LONG = 4096
STORED = (7, 65)                             # frame counts whose reference outputs rotdec.npz holds (clip 0); distances: every case
_cross, _norm, _mm, _dot = ik._cross, ik._norm, ik._mm, ik._dot


def feats(J, route):
    return 12 * J - 1 if route != REAL else 9 * J + 1


def lengths_of(T):
    return [T, 1, (T + 1) // 2]


def bar(distance):
    """4 x the reference's own fp32-to-f64 distance, floor 1e-6."""
    return max(4.0 * float(distance), FLOOR)


def relmax(a, b):
    """max |a - b| relative to the largest magnitude of b."""
    a, b = ik.f64(a), ik.f64(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def quat_relmax(a, b):
    """The same, every quaternion of `a` first given the sign of its partner (q and -q are one rotation)."""
    a, b = ik.f64(a), ik.f64(b)
    s = np.where((a * b).sum(-1, keepdims=True) < 0, -1.0, 1.0)
    return relmax(a * s, b)


def quat_gap(a, b):
    """max of 1 - |<q, q_ref>| over unit-normalised partners."""
    a, b = ik.f64(a), ik.f64(b)
    na, nb = np.linalg.norm(a, axis=-1), np.linalg.norm(b, axis=-1)
    ok = (na > 0) & (nb > 0)
    d = np.abs((a * b).sum(-1))[ok] / (na * nb)[ok]
    return float((1 - d).max()) if d.size else 0.0


# ------------------------------------------------------------------------------------------ trees
def tree(name):
    """-> (J, chains, offsets [J, 3] float32).  tree3: a root with two chains of one bone.  t2m22: HumanML's 22 joints -- two legs, a spine
    and two arms that begin at spine joint 9.  mid21: 21 joints with a chain that begins mid-tree, numbered chain by chain."""
    if name == "tree3":
        J, chains = 3, [[0, 1], [0, 2]]
    elif name == "t2m22":
        J, chains = 22, [[0, 2, 5, 8, 11], [0, 1, 4, 7, 10], [0, 3, 6, 9, 12, 15], [9, 14, 17, 19, 21], [9, 13, 16, 18, 20]]
    elif name == "mid21":
        J, chains = 21, [[0, 1, 2, 3, 4], [0, 5, 6, 7, 8], [0, 9, 10, 11, 12], [10, 13, 14, 15, 16], [10, 17, 18, 19, 20]]
    else:
        raise KeyError(name)
    off = 0.12 * syn.normal(SEED, f"rotdec/{name}/off", (J, 3)) + np.array([0.0, 0.2, 0.0])
    off[0] = (0.3, -0.2, 0.5)                # not zero: the decoders ignore or zero it, as the reference does
    return J, chains, off.astype(np.float32)


def raw_of(offsets):
    """The unit bone directions of a tree's offsets, row 0 zero: what the reference calls n_raw_offsets."""
    off = np.asarray(offsets, np.float64)
    raw = off / np.linalg.norm(off, axis=-1, keepdims=True)
    raw[0] = 0
    return raw.astype(np.float32)


def rest_pose(chains, offsets):
    rest = np.zeros((len(offsets), 3))
    for ch in chains:
        for a, c in zip(ch[:-1], ch[1:]):
            rest[c] = rest[a] + np.asarray(offsets, np.float64)[c]
    return rest


def face_of(J):
    """r_hip, l_hip, sdr_r, sdr_l of the tree with J joints.  The seeded trees are no humans: the two joints furthest apart in x, z of the
    rest pose along x serve as hips, the next such pair as shoulders, the sides named so that the rest pose faces +z (the root quaternion of the
    chain IK is qbetween((0, 0, 1), forward): a character facing -z sits on its half turn)."""
    _, chains, off = tree({3: "tree3", 22: "t2m22", 21: "mid21"}[J])
    rest = rest_pose(chains, off)[:, [0, 2]]
    gap = np.abs(rest[:, None] - rest[None])
    d = gap[..., 0] - 3 * gap[..., 1]                        # far apart in x, close in z: the rest pose faces +z within a few degrees
    d[0], d[:, 0] = -1e9, -1e9
    r_hip, l_hip = np.unravel_index(np.argmax(d), d.shape)
    if J > 4:
        d[[r_hip, l_hip]], d[:, [r_hip, l_hip]] = -1e9, -1e9
    sdr_r, sdr_l = np.unravel_index(np.argmax(d), d.shape)
    if np.dot(rest[r_hip] - rest[l_hip], rest[sdr_r] - rest[sdr_l]) < 0:
        sdr_r, sdr_l = sdr_l, sdr_r
    across = (rest[r_hip] - rest[l_hip]) + (rest[sdr_r] - rest[sdr_l])
    face = (r_hip, l_hip, sdr_r, sdr_l) if -across[0] > 0 else (l_hip, r_hip, sdr_l, sdr_r)
    return tuple(int(a) for a in face)


def chain_parents(chains, J):
    parents = [-1] * J
    for c in chains:
        for k in range(1, len(c)):
            parents[c[k]] = c[k - 1]
    return parents


def expand_chains(chains, offsets):
    """bvh_utils.py:1397-1427 -> (parents, offsets, source): see mst_amd.utils.rot_decode.expand_chains, which this restates."""
    off = np.asarray(offsets)
    new = deepcopy([list(c) for c in chains])
    for chain in new:
        now = chain[1]
        for other in new:
            for k, j in enumerate(other):
                if j >= now:
                    other[k] += 1
        chain.insert(1, now)
    for index in sorted((c[1] for c in chains), reverse=True):
        off = np.concatenate([off[:index], np.zeros((1, 3), off.dtype), off[index:]], 0)
    Jx = len(off)
    source, parents = [-1] * Jx, [-1] * Jx
    for old, chain in zip(chains, new):
        source[chain[0]] = old[0]
        tail = chain[1:]
        for k, i in enumerate(tail):
            parents[i] = chain[k]
            source[i] = old[k + 1] if k != len(tail) - 1 else old[k]
    return parents, off, source


# ------------------------------------------------------------------------------------------ the conversions
def root(data, dtype):
    """recover_root_rot_pos on rows [..., T, F] -> (r_rot_quat [..., T, 4], r_pos [..., T, 3]).  torch.cumsum on the CPU accumulates fp32 in
    double and rounds every output; so does this."""
    data = np.asarray(data, dtype)
    ang = np.zeros(data.shape[:-1], np.float64)
    ang[..., 1:] = np.cumsum(data[..., :-1, 0].astype(np.float64), -1)
    ang = ang.astype(dtype)
    q = np.zeros(data.shape[:-1] + (4,), dtype)
    q[..., 0], q[..., 2] = np.cos(ang), np.sin(ang)
    v = np.zeros(data.shape[:-1] + (3,), dtype)
    v[..., 1:, 0], v[..., 1:, 2] = data[..., :-1, 1], data[..., :-1, 2]
    step = qrot(q, v)
    rp = np.cumsum(step.astype(np.float64), -2).astype(dtype)
    rp[..., 1] = data[..., 3]
    return q, rp


def qrot(q, v):
    """rotation.py:47-56."""
    q, v = np.asarray(q), np.asarray(v)
    u = np.broadcast_to(q[..., 1:], np.broadcast_shapes(q[..., 1:].shape, v.shape))
    uv = _cross(u, v)
    uuv = _cross(u, uv)
    return v + q.dtype.type(2) * (q[..., :1] * uv + uuv)


def qinv(q):
    return q * np.array([1, -1, -1, -1], q.dtype)


def qmultipy(a, b):
    """rotation.py:110-128."""
    a, b = np.broadcast_arrays(a, b)
    w = a[..., :1] * b[..., :1] - _dot(a[..., 1:], b[..., 1:])
    v = a[..., :1] * b[..., 1:] + b[..., :1] * a[..., 1:] + _cross(a[..., 1:], b[..., 1:])
    return np.concatenate([w, v], -1)


def matrix_to_quat(M):
    """rotm2axangle (rotation.py:453-474; 0.1 where the angle is 0) then axangle2q (:209-232)."""
    dt = M.dtype.type
    ac = np.clip((M[..., 0, 0] + M[..., 1, 1] + M[..., 2, 2] - dt(1)) / dt(2), -1, 1)
    th = np.arccos(ac)[..., None]
    th = np.where(th == 0, dt(0.1), th)
    ax = np.stack([M[..., 2, 1] - M[..., 1, 2], M[..., 0, 2] - M[..., 2, 0], M[..., 1, 0] - M[..., 0, 1]], -1) / (dt(2) * np.sin(th))
    aa = ax * th
    th2 = _norm(aa)
    axis = aa / np.where(th2 == 0, dt(0.1), th2)
    return np.concatenate([np.cos(th2 / dt(2)), axis * np.sin(th2 / dt(2))], -1).astype(M.dtype)


def q2cont6d(q):
    """rotation.py:766-769 over q2rotm (:139-160)."""
    two = q.dtype.type(2)
    one = q.dtype.type(1)
    q0, q1, q2, q3 = (q[..., a] for a in range(4))
    return np.stack([one - two * np.square(q2) - two * np.square(q3), two * q1 * q2 + two * q0 * q3, two * q1 * q3 - two * q0 * q2,
                     two * q1 * q2 - two * q0 * q3, one - two * np.square(q1) - two * np.square(q3), two * q2 * q3 + two * q0 * q1], -1)


def hml_rot(data, J, chains, offsets, dtype=np.float32):
    """One clip [T, 12 J - 1] -> dict: quats [T, Jx, 4] (local, on the expanded skeleton), root_pos [T, 3], joints [T, J, 3], parents,
    offsets [Jx, 3]."""
    data = np.asarray(data, dtype)
    T = data.shape[0]
    off = np.asarray(offsets, dtype)
    r, rp = root(data, dtype)
    c = data[:, 4 + 3 * (J - 1):4 + 9 * (J - 1)].reshape(T, J - 1, 6)
    M = ik.cont6d_to_matrix(c)[0]
    quats = matrix_to_quat(M)
    world = np.zeros((T, J, 4), dtype)
    world[:, 0] = r
    M0 = ik.cont6d_to_matrix(q2cont6d(r))[0]
    joints = np.zeros((T, J, 3), dtype)
    joints[:, 0] = rp
    for chain in chains:
        R, G = r, M0
        for a, j in zip(chain[:-1], chain[1:]):
            R = qmultipy(R, quats[:, j - 1])
            world[:, j] = R
            G = _mm(G, M[:, j - 1])
            joints[:, j] = _mm(G, off[j][:, None])[..., 0] + joints[:, a]
    local, parents, xoff = _localise(world, chains, off)
    return dict(quats=local, root_pos=rp, joints=joints, parents=parents, offsets=xoff)


def _localise(world, chains, off):
    """World quaternions [T, J, 4] -> local ones on the expanded skeleton (bvh_utils.py:1416-1434)."""
    T, dtype = world.shape[0], world.dtype
    parents, xoff, source = expand_chains(chains, off)
    ident = np.zeros((T, 4), dtype)
    ident[:, 0] = 1
    xw = np.stack([world[:, s] if s >= 0 else ident for s in source], 1)
    local = np.concatenate([xw[:, :1], qmultipy(qinv(xw[:, parents[1:]]), xw[:, 1:])], 1)
    return local, parents, xoff


def pos_ik(data, J, chains, offsets, dtype=np.float32, diag=None):
    """One clip [T, 12 J - 1] -> dict: quats [T, Jx, 4], root_pos, joints [T, J, 3] (recover_from_ric's), parents, offsets.  The raw offsets
    are the unit directions of `offsets`, the face joints `face_of(J)`.  In float32 the forward direction is smoothed and normalised in float64
    and cast where the reference's qbetween_np casts.  diag (a dict): filled with what `assert_pos_clear` looks at."""
    import encode_fixture as ef
    data = np.asarray(data, dtype)
    T = data.shape[0]
    off = np.asarray(offsets, dtype)
    raw = raw_of(offsets).astype(dtype)
    r_hip, l_hip, sdr_r, sdr_l = face_of(J)
    r, rp = root(data, dtype)
    pos = qrot(r[:, None], data[:, 4:4 + 3 * (J - 1)].reshape(T, J - 1, 3))
    pos[..., 0] += rp[:, 0:1]
    pos[..., 2] += rp[:, 2:3]
    pos = np.concatenate([rp[:, None], pos], 1)
    ac = (pos[:, r_hip] - pos[:, l_hip]) + (pos[:, sdr_r] - pos[:, sdr_l])
    n1 = np.sqrt((ac ** 2).sum(-1))[:, None]
    ac = ac / n1
    fw = ef.smooth(np.stack([ac[:, 2], np.zeros(T, dtype), -ac[:, 0]], -1), np.float64)
    n2 = np.sqrt((fw ** 2).sum(-1))[:, None]
    fw = (fw / n2).astype(dtype)
    z = np.array([0, 0, 1], dtype)
    rq, w1 = ef.qbetween(z, fw)
    rq[0] = (1, 0, 0, 0)
    world = np.zeros((T, J, 4), dtype)
    world[:, 0] = r
    ws, bones = [w1[1:]], []
    for chain in chains:
        R, Rw = rq, r
        for a, c in zip(chain[:-1], chain[1:]):
            v = pos[:, c] - pos[:, a]
            nv = np.sqrt((v ** 2).sum(-1))[:, None]
            bones.append(nv[:, 0])
            quv, w = ef.qbetween(raw[c][None], v / nv)
            ws.append(w)
            loc = ef.qmul(ef.qinv(R), quv)
            R = ef.qmul(R, loc)
            Rw = qmultipy(Rw, loc)
            world[:, c] = Rw
    if diag is not None:
        diag.update(across=n1[:, 0], smoothed=n2[:, 0], qbetween_w=np.concatenate(ws), bones=np.concatenate(bones))
    local, parents, xoff = _localise(world, chains, off)
    return dict(quats=local.astype(dtype), root_pos=rp, joints=pos, parents=parents, offsets=xoff)


def assert_pos_clear(diag):
    """The POS_IK inputs stay away from the discontinuities: |across| and every bone > 1e-3, the smoothed forward's norm > 0.1, the w of
    every qbetween before normalisation > 1e-2 x its norm (no half turn).  diag: of the float64 evaluation."""
    assert diag["across"].min() > 1e-3 and diag["bones"].min() > 1e-3, (diag["across"].min(), diag["bones"].min())
    assert diag["smoothed"].min() > 0.1, diag["smoothed"].min()
    assert diag["qbetween_w"].min() > 1e-2, diag["qbetween_w"].min()


def real_rot(data, J, chains, offsets, dtype=np.float32):
    """One clip [T, 9 J + 1] -> dict: quats [T, J, 4], root_pos, joints [T, J, 3], local [T, 3 (J - 1)], parents, offsets (row 0 zeroed)."""
    data = np.asarray(data, dtype)
    T = data.shape[0]
    off = np.asarray(offsets, dtype)
    parents = chain_parents(chains, J)
    r, rp = root(data, dtype)
    c = data[:, 4 + 3 * (J - 1):].reshape(T, J, 6)
    M = ik.cont6d_to_matrix(c)[0]
    quats = matrix_to_quat(M)
    quats[:, 0] = qmultipy(r, quats[:, 0].copy())
    Y = ik.quaternion_to_matrix(r)[0]
    G, p = [None] * J, [None] * J
    G[0], p[0] = _mm(Y, M[:, 0]), rp
    order = [j for ch in chains for j in ch[1:]]          # every joint after its parent; the reference walks 1 .. J - 1, parents[j] < j
    for j in order:
        a = parents[j]
        p[j] = _mm(G[a], off[j][:, None])[..., 0] + p[a]
        G[j] = _mm(G[a], M[:, j])
    joints = np.stack(p, 1)
    # root-relative, as the function is meant.  The reference's `pos[..., 0] -= pos[..., 0:1, 0]` runs in place on the storage it reads, joint
    # 0 first, so what it returns depends on how torch splits the loop: `local_as_run` is what a short clip gives.
    rel = joints.copy()
    rel[..., 0] -= joints[:, 0:1, 0]
    rel[..., 2] -= joints[:, 0:1, 2]
    local = qrot(qinv(r)[:, None], rel[:, 1:]).reshape(T, -1)
    local_as_run = qrot(qinv(r)[:, None], joints[:, 1:]).reshape(T, -1)
    xoff = off.copy()
    xoff[0] = 0
    return dict(quats=quats, root_pos=rp, joints=joints, local=local, local_as_run=local_as_run, parents=parents, offsets=xoff)


DECODE = {HML: hml_rot, REAL: real_rot, POS: pos_ik}
OUTPUTS = {HML: ("quats", "root_pos", "joints"), REAL: ("quats", "root_pos", "joints", "local"), POS: ("quats", "root_pos", "joints")}


def decode_batch(route, data, J, chains, offsets, lengths, dtype):
    """[B, T, F] with lengths -> dict of zero-padded [B, T, ...] arrays (every clip decoded at its own length)."""
    B, T = data.shape[:2]
    out = {}
    for b in range(B):
        n = int(lengths[b])
        one = DECODE[route](data[b, :n], J, chains, offsets, dtype)
        for k in OUTPUTS[route]:
            if k not in out:
                out[k] = np.zeros((B, T) + one[k].shape[1:], dtype)
            out[k][b, :n] = one[k]
    return out


def distance(key, a, b):
    return quat_relmax(a, b) if key == "quats" else relmax(a, b)


# ------------------------------------------------------------------------------------------ rows
def identity_joint(chains):
    """The joint whose 6D block is exactly the identity: the first chain's last joint but one (never the root), whose world quaternion and
    whose predecessor's both reach the expanded skeleton (`identity_carriers`)."""
    c = chains[0]
    return c[max(1, len(c) - 2)]


def make_rows(name, route, T, B=3):
    """-> data [B, T, F] float32 of tree `name`: a root that turns and drifts, positions that no decoder here reads, 6D blocks that are two
    columns of a rotation by 0.45 .. 1.45 rad about a drifting axis, scaled and perturbed as a network emits them -- and one joint's block
    exactly (1, 0, 0, 0, 1, 0) in every frame."""
    J, chains, off = tree(name)
    F = feats(J, route)
    nb = J - 1 if route != REAL else J
    tag = f"rotdec/{name}/{route}/T{T}"
    data = np.zeros((B, T, F))
    data[..., 0] = 0.03 * syn.normal(SEED, tag + "/rv", (B, T))
    data[..., 1:3] = 0.04 * syn.normal(SEED, tag + "/lv", (B, T, 2))
    data[..., 3] = 0.9 + 0.03 * syn.normal(SEED, tag + "/y", (B, T))
    data[..., 4:] = syn.normal(SEED, tag + "/rest", (B, T, F - 4))
    axis = syn.normal(SEED, tag + "/axis", (B, 1, nb, 3)).astype(np.float64) + 0.2 * syn.normal(SEED, tag + "/axis_t", (B, T, nb, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    ang = 0.55 + 0.8 * syn.uniform01(SEED, tag + "/ang", B * nb).reshape(B, 1, nb) + 0.1 * np.sin(
        np.arange(T)[None, :, None] * 0.21 + 6.0 * syn.uniform01(SEED, tag + "/ph", B * nb).reshape(B, 1, nb))
    K = np.zeros((B, T, nb, 3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -axis[..., 2], axis[..., 1], axis[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -axis[..., 0], -axis[..., 1], axis[..., 0]
    R = np.eye(3) + np.sin(ang)[..., None, None] * K + (1 - np.cos(ang))[..., None, None] * _mm(K, K)
    scale = 0.8 + 0.4 * syn.uniform01(SEED, tag + "/scale", B * T * nb * 2).reshape(B, T, nb, 2, 1)
    c = np.stack([R[..., :, 0], R[..., :, 1]], -2) * scale + 0.03 * syn.normal(SEED, tag + "/c6", (B, T, nb, 2, 3))
    c = c.reshape(B, T, nb, 6)
    idj = identity_joint(chains)
    blk = idj - 1 if route != REAL else idj
    keep = [k for k in range(nb) if k != blk]
    ik.assert_angles_clear(c.astype(np.float32)[:, :, keep])
    c[:, :, blk] = (1, 0, 0, 0, 1, 0)
    R0 = 4 + 3 * (J - 1)
    data[..., R0:R0 + 6 * nb] = c.reshape(B, T, 6 * nb)
    if route == POS:
        # positions the chain IK is well conditioned on: the tree's rest pose, every joint displaced a little per frame, heights absolute
        # (every bone the tree's own offset turned and stretched by a tenth of its length per frame, so that no bone comes near the half turn
        # from its raw direction however short it is)
        length = np.linalg.norm(off.astype(np.float64), axis=-1)[None, None, :, None]
        bone = off.astype(np.float64)[None, None] + 0.1 * length * syn.normal(SEED, tag + "/bone", (B, T, J, 3))
        pose = np.zeros((B, T, J, 3))
        for ch in chains:
            for a, c_ in zip(ch[:-1], ch[1:]):
                pose[:, :, c_] = pose[:, :, a] + bone[:, :, c_]
        ric = pose[:, :, 1:] + np.array([0.0, 0.9, 0.0])
        data[..., 4:R0] = ric.reshape(B, T, 3 * (J - 1))
        # a yaw that swings and does not drift (r_rot_quat turns by TWICE the summed angle: +-0.4 rad here), so that the forward direction
        # stays clear of -z however long the clip
        ang = 0.2 * np.sin(0.013 * np.arange(T + 1)[None] + 6.0 * syn.uniform01(SEED, tag + "/yaw", B)[:, None])
        data[..., 0] = ang[:, 1:] - ang[:, :-1] + 0.001 * syn.normal(SEED, tag + "/rv2", (B, T))
    data = data.astype(np.float32)
    if route == POS:
        for b in range(B):
            diag = {}
            pos_ik(data[b], J, chains, off, np.float64, diag)
            assert_pos_clear(diag)
    return data


def identity_carriers(name):
    """HML: the expanded joints whose local quaternion is qinv(w) (x) w of one and the same world quaternion because of the identity block
    -- they carry the identity joint's world quaternion and their parent carries its chain predecessor's, which is the same number bit
    for bit (q (x) (1, 0, 0, 0) = q).  Their x, y, z are exactly 0."""
    J, chains, off = tree(name)
    parents, _, source = expand_chains(chains, off)
    j = identity_joint(chains)
    a = chain_parents(chains, J)[j]
    return [i for i in range(1, len(parents)) if source[i] == j and source[parents[i]] == a]


def consistency_case():
    """A HumanML clip whose rotation and position channels both come from one set of joints: encode_fixture's seeded 22-joint clip of 65
    frames, encoded by its float32 and float64 restatements of `process_file`.  -> (skeleton, positions [1, T, J, 3], offsets [J, 3]
    float32, rows32 [T - 1, 263], rows64)."""
    import encode_fixture as ef
    J, T = 22, 65
    sk = ef.skeleton(SEED, J)
    pos, _ = ef.make_clip(SEED, "rotdec/consistency", T, sk, ef.HML)
    e32, _ = ef.encode(pos, None, sk, ef.HML, np.float32, frames_out=T - 1)
    e64, diags = ef.encode(pos, None, sk, ef.HML, np.float64, frames_out=T - 1)
    ef.assert_clear(diags, ef.HML)
    return sk, pos, sk.offsets.astype(np.float32), e32["sample"][0, :, 0].T.copy(), e64["sample"][0, :, 0].T.copy()


def euler_clear_share(quats, margin_deg=85.0):
    """Share of frame-joints whose middle Euler angle (the y angle of a 'zyx' file) is beyond +-margin_deg: the frames the file test
    leaves out."""
    q = ik.f64(quats)
    q = q / np.maximum(np.linalg.norm(q, axis=-1, keepdims=True), 1e-300)
    s = np.clip(2 * (q[..., 0] * q[..., 2] - q[..., 3] * q[..., 1]), -1, 1)
    out = np.abs(s) > math.sin(math.radians(margin_deg))
    return float(out.mean()), out
