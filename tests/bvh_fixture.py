"""numpy restatement of what the reference computes between a BVH file's text and its arrays: `eul2q` (utils/rotation.py:344-361), the sign
continuity of `remove_quat_discontinuities` (:666-683), `quat_fk` (:646-663), `q2eul` (:364-382) with `save_bvh`'s channel layout
(data_loaders/humanml/common/bvh_utils.py:588-612), the joint selection of `decode_channels`, and `uniform_skeleton_basic`
(data_loaders/humanml/scripts/motion_process.py:12-35 over common/skeleton.py:43-151).

Nothing here imports the reference and no table is taken from it: trees, channels and clips are generated from a seed.  Every function
takes a dtype and runs in it, so one set of inputs can be evaluated in float32 and in float64.  The quaternion helpers are
encode_fixture's.  `assert_clear` keeps every test input away from the two discontinuities (see its docstring); the generators meet it by
construction -- decode inputs step a few degrees a frame (the smallest neighbour dot at 4 degree steps is 0.97), writer inputs are built
from Euler angles with the middle one within +-80 degrees (|sin| <= 0.985)."""
import numpy as np

import encode_fixture as ef
import ik_fixture as ik
import mst_amd.synthetic as syn
from mst_amd.utils import bvh

rel, bar = ik.rel, ik.bar
qmul, qinv, qrot, qbetween, _norm = ef.qmul, ef.qinv, ef.qrot, ef.qbetween, ef._norm
SEED = 20261003                              # tests/golden/make_golden.py's: the goldens were made from it
AXES = {"x": (1, 0, 0), "y": (0, 1, 0), "z": (0, 0, 1)}
ORDERS = ("zyx", "xzy", "xyz", "yzx", "zxy", "yxz")
# name -> (non-End joints, frames, layout, file order): the cases tests/golden/bvh.npz holds
GOLDEN_WRITE = {"w6": (6, 40, "root6", "zyx"), "w31": (31, 76, "root6", "zyx"), "wpos": (6, 40, "all6", "zyx"), "wxzy": (7, 33, "root6", "xzy")}
# name -> (file joints, frames, layout, file order): drifting channels written by format_bvh and read by the reference
GOLDEN_DECODE = {"d31": (31, 76, "root6", "zyx"), "dall6": (9, 40, "all6", "yxz")}
GOLDEN_RETARGET = ((22, 60), (5, 24))


# ------------------------------------------------------------------------------------------ the conversions
def eul2q(deg, order, dtype):
    """Euler degrees [..., 3] in the file's channel order -> q(e0, axis0) (x) (q(e1, axis1) (x) q(e2, axis2))."""
    e = np.asarray(deg, dtype) * dtype(np.pi / 180.0) / dtype(2)
    qs = []
    for k in range(3):
        ax = np.asarray(AXES[order[k]], dtype)
        qs.append(np.concatenate([np.cos(e[..., k:k + 1]), np.sin(e[..., k:k + 1]) * ax], -1))
    return qmul(qs[0], qmul(qs[1], qs[2]))


def sign_scan(raw):
    """raw [T, J, 4] -> (signs [T, J], dots [T-1, J]): s[0] = +1, s[t] = -1 iff s[t-1] * dot(raw[t-1], raw[t]) < 0."""
    dots = (raw[:-1] * raw[1:]).sum(-1)
    s = np.ones(raw.shape[:2], raw.dtype)
    for t in range(1, raw.shape[0]):
        s[t] = np.where(s[t - 1] * dots[t - 1] < 0, -1, 1)
    return s, dots


def quat_fk(lrot, lpos, parents):
    lrot = lrot / _norm(lrot)
    gr, gp = [lrot[:, 0]], [lpos[:, 0]]
    for j in range(1, len(parents)):
        gp.append(qrot(gr[parents[j]], lpos[:, j]) + gp[parents[j]])
        gr.append(qmul(gr[parents[j]], lrot[:, j]))
    return np.stack(gr, 1), np.stack(gp, 1)


def decode(channels, sk, dtype=np.float32, scale=1.0, stride=1, phase=0, joints=None):
    """One clip [T, C] -> dict(rotations [T', J, 4], positions [T', J, 3], local_positions, global_rotations, dots [T-1, Jf], signs)."""
    ch = np.asarray(channels, dtype)
    T, Jf = ch.shape[0], sk.joints
    raw = np.zeros((T, Jf, 4), dtype)
    raw[..., 0] = 1
    lpos = np.broadcast_to(np.asarray(sk.offsets, dtype), (T, Jf, 3)).copy()
    for j in range(Jf):
        if sk.rot_col[j] >= 0:
            raw[:, j] = eul2q(ch[:, sk.rot_col[j]:sk.rot_col[j] + 3], sk.order, dtype)
        if sk.pos_col[j] >= 0:
            lpos[:, j] = ch[:, sk.pos_col[j]:sk.pos_col[j] + 3]
    lpos = lpos * dtype(scale)
    signs, dots = sign_scan(raw)
    lrot = raw * signs[..., None]
    lrot, lpos = lrot[phase::stride], lpos[phase::stride]
    gr, gp = quat_fk(lrot, lpos, sk.parents)
    out = dict(dots=dots, signs=signs)
    if joints is None:
        out.update(rotations=lrot, positions=gp, local_positions=lpos, global_rotations=gr)
        return out
    sel = [sk.names.index(j) if isinstance(j, str) else int(j) for j in joints]
    rot, loc = [], []
    for j in sel:
        a = sk.parents[j]
        while a >= 0 and a not in sel:
            a = sk.parents[a]
        if a == sk.parents[j]:
            rot.append(lrot[:, j])
            loc.append(lpos[:, j])
        elif a < 0:
            rot.append(gr[:, j])
            loc.append(gp[:, j])
        else:
            rot.append(qmul(qinv(gr[:, a]), gr[:, j]))
            loc.append(qrot(qinv(gr[:, a]), gp[:, j] - gp[:, a]))
    out.update(rotations=np.stack(rot, 1), positions=gp[:, sel], local_positions=np.stack(loc, 1), global_rotations=gr[:, sel])
    return out


def decode_batch(channels, sk, lengths=None, dtype=np.float32, **kw):
    """[B, T, C] -> the four outputs [B, T', ...], zero past a clip, its out-lengths, and the clips' dicts."""
    B, T = channels.shape[:2]
    stride, phase = kw.get("stride", 1), kw.get("phase", 0)
    To = (T - phase + stride - 1) // stride
    outs = [decode(channels[b, :(T if lengths is None else int(lengths[b]))], sk, dtype, **kw) for b in range(B)]
    res = {}
    for name in ("rotations", "positions", "local_positions", "global_rotations"):
        res[name] = np.zeros((B, To) + outs[0][name].shape[1:], dtype)
        for b, o in enumerate(outs):
            res[name][b, :len(o[name])] = o[name]
    res["lengths"] = np.array([len(o["rotations"]) for o in outs], np.int32)
    return res, outs


def q2eul_args(q, order):
    """The argument of the arcsin `q2eul` of order[::-1] takes, for a file of `order`."""
    q = q / _norm(q)
    q0, q1, q2, q3 = (q[..., k] for k in range(4))
    return 2 * (q0 * q2 - q3 * q1) if order == "zyx" else 2 * (q1 * q2 + q3 * q0)


def q2eul(q, order, dtype):
    """`q2eul(q, order[::-1])` for a file of `order` ('zyx' or 'xzy') -> radians by axis (x, y, z)."""
    q = np.asarray(q, dtype)
    q = q / _norm(q)
    q0, q1, q2, q3 = (q[..., k] for k in range(4))
    one, two = dtype(1), dtype(2)
    if order == "zyx":
        es = [np.arctan2(two * (q0 * q1 + q2 * q3), one - two * (q1 * q1 + q2 * q2)),
              np.arcsin(np.clip(two * (q0 * q2 - q3 * q1), -one, one)),
              np.arctan2(two * (q0 * q3 + q1 * q2), one - two * (q2 * q2 + q3 * q3))]
    elif order == "xzy":
        es = [np.arctan2(two * (q1 * q0 - q2 * q3), -q1 * q1 + q2 * q2 - q3 * q3 + q0 * q0),
              np.arctan2(two * (q2 * q0 - q1 * q3), q1 * q1 - q2 * q2 - q3 * q3 + q0 * q0),
              np.arcsin(np.clip(two * (q1 * q2 + q3 * q0), -one, one))]
    else:
        raise NotImplementedError(order)
    return np.stack(es, -1).astype(dtype)


def channels_from_quats(quats, root_pos, parents, order="zyx", positions=None, dtype=np.float32):
    """[T, J, 4], [T, 3] -> [T, 3 + 3 J] (or [T, 6 J]): degrees, the writer's joint sequence and channel order."""
    seq = bvh.writer_sequence(parents)
    deg = q2eul(np.asarray(quats, dtype)[:, seq], order, dtype) * dtype(180.0 / np.pi)
    deg = deg[..., ["xyz".index(a) for a in order]]
    T, J = deg.shape[:2]
    if positions is None:
        return np.concatenate([np.asarray(root_pos, dtype), deg.reshape(T, -1)], -1)
    pos = np.asarray(positions, dtype)[:, seq].copy()
    pos[:, 0] = root_pos
    return np.concatenate([pos, deg], -1).reshape(T, -1)


def retarget(positions, target_offset, raw, chains, l_idx, face, dtype=np.float32):
    """One clip [T, J, 3] -> (retargeted [T, J, 3], diag)."""
    pos = np.asarray(positions, dtype)
    tgt, raw = np.asarray(target_offset, dtype), np.asarray(raw, dtype)
    T, J = pos.shape[:2]
    par = ik.parents_of(chains, J)
    leg = lambda off: sum(np.abs(off(l)).max() for l in l_idx)
    src_leg = leg(lambda l: _norm(pos[0, l] - pos[0, par[l]]) * raw[l])
    ratio = dtype(leg(lambda l: tgt[l])) / dtype(src_leg)
    r_hip, l_hip, sdr_r, sdr_l = face
    ac = (pos[:, r_hip] - pos[:, l_hip]) + (pos[:, sdr_r] - pos[:, sdr_l])
    n0 = _norm(ac)
    ac = ac / n0
    fw = np.stack([ac[:, 2], np.zeros(T, dtype), -ac[:, 0]], -1)
    fw = fw / _norm(fw)
    rq, w0 = qbetween(np.array([0, 0, 1], dtype), fw)
    rq[0] = (1, 0, 0, 0)
    out = np.zeros((T, J, 3), dtype)
    out[:, 0] = pos[:, 0] * ratio
    bones, ws = [], [w0[1:]]
    with np.errstate(invalid="ignore", divide="ignore"):
        for chain in chains:
            R = rq
            for a, c in zip(chain[:-1], chain[1:]):
                v = pos[:, c] - pos[:, a]
                nv = _norm(v)
                bones.append(nv[:, 0])
                quv, w = qbetween(raw[c][None], v / nv)
                ws.append(w)
                loc = qmul(qinv(R), quv)
                R = qmul(R, loc)
                out[:, c] = qrot(R, np.broadcast_to(tgt[c], (T, 3))) + out[:, a]
    return out, dict(across=n0[:, 0], bones=np.concatenate(bones), qbetween_w=np.concatenate(ws))


# ------------------------------------------------------------------------------------------ clearance
def assert_clear(dots=None, writer=None, order="zyx", retarget_diag=None):
    """Fails (never skips, drops no case) unless every neighbouring raw pair of a decode input has |dot| >= 1e-3 (the sign decision),
    every quaternion handed to the writer has |2 (q0 q2 - q3 q1)| <= 0.99 -- for an 'xzy' file |2 (q1 q2 + q3 q0)|, the arcsin argument of
    the formula set it goes through -- and a retarget input has |across| and every bone > 1e-3 and no qbetween within 1e-2 of a half turn.  Of the float64 evaluation."""
    if dots is not None and np.size(dots):
        assert np.abs(dots).min() >= 1e-3, f"a neighbouring pair of raw quaternions with |dot| {np.abs(dots).min():.3g} < 1e-3"
    if writer is not None:
        q = np.asarray(writer, np.float64)
        a = np.abs(q2eul_args(q, order)).max()
        assert a <= 0.99, f"a quaternion for the writer with arcsin argument {a:.4f} > 0.99 ({order})"
    if retarget_diag is not None:
        d = retarget_diag
        assert d["across"].min() > 1e-3 and d["bones"].min() > 1e-3, (d["across"].min(), d["bones"].min())
        assert d["qbetween_w"].min() > 1e-2, f"a qbetween with w / norm {d['qbetween_w'].min():.3g} <= 1e-2 (a half turn)"


# ------------------------------------------------------------------------------------------ generators
def tree(seed, tag, Jn):
    """Parents of Jn joints in depth-first (file) order: every joint hangs off a joint of the path to its predecessor."""
    u = syn.uniform01(seed, f"bvh/{tag}/tree", max(Jn, 1))
    parents, path = [-1], [0]
    for j in range(1, Jn):
        depth = 1 + int(u[j] * len(path)) if j % 3 else len(path)           # every third joint extends the path: chains, not a bush
        path = path[:depth]
        parents.append(path[-1])
        path.append(j)
    return parents


def file_skeleton(seed, tag, Jf, layout="root6", order="zyx", scale=1.0):
    """A BvhSkeleton of Jf file joints, the last quarter of them End Sites under the first leaves.  layout: 'root6' (root 6 channels, the
    rest 3) or 'all6'."""
    E = Jf // 4 if Jf > 2 else Jf - 1
    Jn = Jf - E
    par = tree(seed, tag, Jn)
    leaves = [j for j in range(Jn) if j not in par]
    assert len(leaves) >= E, (tag, Jf, len(leaves), E)
    ends = set(leaves[:E])
    off = syn.normal(seed, f"bvh/{tag}/off", (Jn + E, 3)).astype(np.float64) * 0.1 * scale
    names, parents, is_end, rot_col, pos_col, index, col = [], [], [], [], [], {}, 0
    for j in range(Jn):
        index[j] = len(names)
        names.append(f"j{j}")
        parents.append(-1 if j == 0 else index[par[j]])
        is_end.append(False)
        six = layout == "all6" or j == 0
        pos_col.append(col if six else -1)
        rot_col.append(col + 3 if six else col)
        col += 6 if six else 3
        if j in ends:
            names.append(bvh.END_SITE)
            parents.append(index[j])
            is_end.append(True)
            rot_col.append(-1)
            pos_col.append(-1)
    offsets = np.round(off[:len(names)], 6).astype(np.float32)          # six decimals: what a file holds
    offsets[0] = 0
    return bvh.BvhSkeleton(names, parents, offsets, is_end, order, 1 / 30, rot_col, pos_col, col)


def channels(seed, tag, sk, T, B=1, step=3.0):
    """Euler channels [B, T, C] float32 that drift up to `step` degrees a frame and wrap into (-180, 180], so that the raw quaternions flip
    sign at every wrap; a root that walks; with 6 channels on every joint, positions that wobble around the offsets."""
    t = np.arange(T)[None, :, None]
    C = sk.channels
    u = syn.uniform01(seed, f"bvh/{tag}/ch", B * C * 3).reshape(3, B, 1, C)
    deg = 360 * u[0] - 180 + step * (2 * u[1] - 1) * t + 0.5 * np.sin(0.11 * t + 6.28 * u[2])
    deg = (deg + 180) % 360 - 180
    ch = deg.copy()
    for j in range(sk.joints):
        c = sk.pos_col[j]
        if c >= 0:
            ch[..., c:c + 3] = sk.offsets[j] + 0.02 * np.sin(0.07 * t + 6.28 * u[2][..., c:c + 3]) + (0.01 * t * (u[1][..., c:c + 3] - 0.5) if j == 0 else 0)
    return ch.astype(np.float32)


def writer_case(seed, name):
    """A golden writer case -> (names, parents, offsets, end_offsets, order, positions flag, quats [T, J, 4], pos [T, J, 3]) float32: joints
    in a depth-first order, quaternions from smooth Euler angles whose middle one stays within +-80 degrees, not normalised."""
    Jn, T, layout, order = GOLDEN_WRITE[name]
    par = tree(seed, f"write/{name}", Jn)
    t = np.arange(T)[:, None, None]
    u = syn.uniform01(seed, f"bvh/write/{name}/e", Jn * 9).reshape(3, 1, Jn, 3)
    e = 170 * (2 * u[0] - 1) + 2.5 * (2 * u[1] - 1) * t + 8 * np.sin(0.13 * t + 6.28 * u[2])
    e[..., 1] = 80 * np.sin(0.05 * t[..., 0] + 6.28 * u[2][..., 1])
    q = eul2q(e, order, np.float64) * (0.7 + 0.6 * u[1][..., :1])
    off = syn.normal(seed, f"bvh/write/{name}/off", (Jn, 3)) * 0.1
    off[0] = 0
    leaves = [j for j in range(Jn) if j not in par]
    end = syn.normal(seed, f"bvh/write/{name}/end", (len(leaves), 3)) * 0.05
    pos = np.broadcast_to(off, (T, Jn, 3)).copy()
    if layout == "all6":
        pos = pos + 0.01 * np.sin(0.09 * t + 6.28 * u[0])
    pos[:, 0] = np.cumsum(0.02 * syn.normal(seed, f"bvh/write/{name}/root", (T, 3)), 0) + (0.1, 0.9, -0.2)
    return ([f"b{j}" for j in range(Jn)], par, off.astype(np.float32), end.astype(np.float32), order, layout == "all6", q.astype(np.float32),
            pos.astype(np.float32))


def retarget_case(seed, J, T, B=1, lengths=None):
    """-> (encode_fixture skeleton, positions [B, T, J, 3] float32, target offsets [J, 3] float32, l_idx)."""
    sk = ef.skeleton(seed, J)
    pos, _ = ef.make_clip(seed, f"bvh/retarget/J{J}T{T}B{B}", max(T, 2), sk, ef.POSROT, B=B, lengths=None if lengths is None else np.maximum(lengths, 2))
    other = ef.skeleton(seed + 1, J, 1.3).offsets
    tgt = (other * (1 + 0.2 * syn.uniform01(seed, f"bvh/retarget/tgt{J}", J)[:, None])).astype(np.float32)
    tgt[0] = 0
    return sk, pos[:, :T], tgt, ((1, 3) if J == 5 else (2, 6))
