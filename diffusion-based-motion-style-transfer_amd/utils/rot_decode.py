"""A sample's rotation channels decoded on the GPU: joints and BVH files without a fit.  The counterparts of the reference's `output_bvh`
(data_loaders/humanml/common/bvh_utils.py:1382-1441), `recover_from_rot` (:1321-1335), `output_bvh_from_real_rot` (:1538-1563),
`recover_from_real_rot` (:1337-1345), `process_pos_from_real_rot` (:1366-1378) and `output_bvh_with_pos` (:1444-1511), all over `recover_root_rot_pos` (:1299-1318).  One
launch for a batch of clips (csrc/mst_rotdec.h); the files are written through `bvh.quats_to_channels`, `bvh.writer_skeleton` and
`bvh.format_bvh` with one device-to-host copy.

Three routes:
  'hml_rot'   the HumanML row, 12 J - 1 features (263 at 22 joints): the J - 1 6D blocks become world quaternions chain by chain -- every
              chain restarts from the root's yaw quaternion, also one that begins at a non-root joint, as the reference has it -- and are
              made local on the expanded skeleton (`expand_chains`: a zero-offset duplicate of every chain's second joint, the rotations
              shifted one joint down each chain, chains written in list order so that a later write wins).  The joints are
              `Skeleton.forward_kinematics_cont6d` (common/skeleton.py:177-198).
  'real_rot'  the position-rotation row, 9 J + 1 features (181 / 190): the J 6D blocks are local quaternions already, the root's multiplied
              from the left by the yaw quaternion.  The joints are `forward_kinematics_real_cont6d` (skeleton.py:200-222), the local rows
              those minus the root's x and z, un-rotated (root-relative: a stated deviation from what the reference's aliased in-place
              subtraction returns; csrc/mst_rotdec.h has it).
  'pos_ik'    the HumanML row read for its POSITIONS: `recover_from_ric`, then `Skeleton.inverse_kinematics_np(smooth_forward=True)`
              (skeleton.py:55-103; the forward direction smoothed by 161 taps summed in double), the IK's root dropped, and the same
              chain products and expanded skeleton as 'hml_rot'.  Needs `raw_offsets` (unit bone directions) and `face_joint_indx`.

Not covered: `output_bvh_with_22rot`, `fit_joints_bvh_quats`, and the `skel_joints=` / `do_root_R=False` arguments of the reference's forward-kinematics methods (no caller in
the reference uses those).  Not reproduced: `rotm2axangle`'s SVD branch for a rotation whose angle is an exact multiple of pi.  Nothing
here has a CPU path."""
import ctypes as C
from copy import deepcopy
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .. import _native as N
from . import bvh
from .joint_fit import _stat

_NO_CPU = bvh._NO_CPU
FRAME_TIME = 1 / 20
ROUTES = {"hml_rot": 0, "real_rot": 1, "pos_ik": 2}


@dataclass
class RotAnim:
    """What `decode_rotations` returns and `save_rot_bvhs` writes.  quats [B, T, Jx, 4]: local quaternions (w, x, y, z) on the skeleton
    `parents` / `offsets` describe -- the expanded one (Jx = J + chains) on 'hml_rot', the clip's own (Jx = J, row 0 of the offsets zeroed)
    on 'real_rot'; root_pos [B, T, 3].  Rows at or past a clip's length are zeros.  A tensor that was not asked for is None."""
    quats: Optional[torch.Tensor]
    root_pos: Optional[torch.Tensor]
    parents: list
    offsets: np.ndarray
    names: Optional[list] = None


def max_joints():
    """Most joints `decode_rotations` takes (mst_rot_decode_max_joints)."""
    return int(N.lib().mst_rot_decode_max_joints())


def max_frames(joints):
    """Longest clip `decode_rotations` takes at this joint count (mst_rot_decode_max_frames)."""
    n = int(N.lib().mst_rot_decode_max_frames(int(joints)))
    if n < 0:
        N.check(1)
    return n


def _checked_chains(what, chains, J):
    """-> list of lists of ints: every chain has two joints or more and starts at a joint already placed (joint 0 or an earlier chain's),
    every joint 1 .. J - 1 is a child exactly once."""
    chains = [[int(j) for j in c] for c in chains]
    if not chains:
        raise ValueError(f"{what}: no kinematic chains")
    placed = {0}
    for n, c in enumerate(chains):
        if len(c) < 2:
            raise ValueError(f"{what}: chain {n} has fewer than two joints")
        for j in c:
            if not 0 <= j < J:
                raise ValueError(f"{what}: joint {j} of chain {n} outside 0..{J - 1}")
        if c[0] not in placed:
            raise ValueError(f"{what}: chain {n} starts at joint {c[0]}, which no earlier chain has placed")
        for j in c[1:]:
            if j in placed:
                raise ValueError(f"{what}: joint {j} is named twice as a child (chain {n})")
            placed.add(j)
    missing = sorted(set(range(J)) - placed)
    if missing:
        raise ValueError(f"{what}: joint {missing[0]} is named by no chain (the reference's parent index -1 would wrap to the last joint)")
    return chains


def chain_parents(chains, J):
    """bvh_utils.py:1547-1551: a joint's parent is its predecessor in its chain; the root's is -1."""
    parents = [-1] * J
    for c in chains:
        for k in range(1, len(c)):
            parents[c[k]] = c[k - 1]
    return parents


def expand_chains(chains, offsets):
    """The skeleton `output_bvh` writes (bvh_utils.py:1397-1427), a pure function of the chains: a zero-offset duplicate of every chain's
    second joint in front of it, every new joint carrying the world rotation of the joint one step further down its chain (the last
    repeats the one before it).  Chains write in list order and a later write wins.
    -> (parents [Jx], offsets [Jx, 3] float32, source [Jx]: the joint whose world quaternion new joint i carries), Jx = J + len(chains)."""
    off = np.asarray(offsets, np.float32)
    if off.ndim != 2 or off.shape[1] != 3:
        raise ValueError(f"expand_chains: offsets of shape {off.shape}, expected [J, 3]")
    J = off.shape[0]
    chains = _checked_chains("expand_chains", chains, J)
    new = deepcopy(chains)
    for chain in new:
        now = chain[1]
        for other in new:
            for k, j in enumerate(other):
                if j >= now:
                    other[k] += 1
        chain.insert(1, now)
    for index in sorted((c[1] for c in chains), reverse=True):
        off = np.concatenate([off[:index], np.zeros((1, 3), np.float32), off[index:]], 0)
    Jx = off.shape[0]
    source, parents = [-1] * Jx, [-1] * Jx
    for old, chain in zip(chains, new):
        source[chain[0]] = old[0]
        tail = chain[1:]
        for k, i in enumerate(tail):
            parents[i] = chain[k]
            source[i] = old[k + 1] if k != len(tail) - 1 else old[k]
    return parents, off, source


def _checked_lengths(what, lengths, B, T, device):
    """-> int32 tensor [B] on `device` or None.  Host values (a list, an array, a CPU tensor) are checked, 1 <= len <= T, and uploaded.
    A CUDA tensor is taken as it is, without a copy back or a synchronisation: the kernel clamps its values into 1 .. T."""
    if lengths is None:
        return None
    if torch.is_tensor(lengths) and lengths.is_cuda:
        if lengths.numel() != B:
            raise ValueError(f"{what}: {lengths.numel()} lengths for {B} clips")
        return lengths.detach().reshape(-1).to(torch.int32).contiguous()
    host = lengths.detach().numpy() if torch.is_tensor(lengths) else np.asarray(lengths)
    host = host.reshape(-1).astype(np.int64)
    if host.shape[0] != B:
        raise ValueError(f"{what}: {host.shape[0]} lengths for {B} clips")
    if host.min() < 1 or host.max() > T:
        raise ValueError(f"{what}: lengths {host.min()}..{host.max()} outside 1..{T}")
    return torch.from_numpy(host.astype(np.int32)).to(device)


def _ints(v):
    return (C.c_int32 * max(len(v), 1))(*[int(a) for a in v])


def _layout(what, shape, F):
    if len(shape) == 3:
        B, T, feats = shape
        sampler = False
    elif len(shape) == 4 and shape[2] == 1:
        B, feats, _, T = shape
        sampler = True
    else:
        raise ValueError(f"{what}: sample of shape {tuple(shape)}, expected [B, T, {F}] or the samplers' [B, {F}, 1, T]")
    return B, T, feats, sampler


def decode_rotations(sample, joints_num, chains, offsets, *, route, mean=None, std=None, lengths=None, raw_offsets=None,
                     face_joint_indx=None, joints=False, local=False, quats=True, root_pos=True):
    """A batch of rows decoded in one launch on the caller's current stream.  -> RotAnim, or (RotAnim, joints [B, T, J, 3]),
    (RotAnim, local [B, T, 3 (J - 1)]) or (RotAnim, joints, local) when those are asked for.

    sample: [B, T, F] denormalised rows, or the samplers' [B, F, 1, T] output together with `mean` / `std` ([F]; the kernel denormalises as
    it reads); any strides, not modified.  route: 'hml_rot' or 'pos_ik' (F = 12 J - 1) or 'real_rot' (F = 9 J + 1).  raw_offsets [J, 3]
    (unit bone directions) and face_joint_indx (r_hip, l_hip, sdr_r, sdr_l) belong to 'pos_ik' and are refused on the other routes.  chains: the kinematic chains;
    offsets [J, 3]: the bone offsets of the forward kinematics and of the file (`tgt_offsets` / `skeleton._offset`).  lengths [B]: rows at
    or past a clip's length are zeros; host values are checked (1 .. T) and uploaded, a CUDA tensor is used as it is with no copy back and
    no synchronisation (the kernel clamps it into 1 .. T).  local: the rows of `process_pos_from_real_rot` ('real_rot' only).
    quats / root_pos = False leave that tensor out of the launch (None in the RotAnim).  On 'pos_ik' the joints are `recover_from_ric`'s."""
    what = "decode_rotations"
    if route not in ROUTES:
        raise ValueError(f"{what}: route {route!r} is none of {tuple(ROUTES)}")
    if not torch.is_tensor(sample):
        raise TypeError(f"{what}: sample is a tensor (the drop-ins take the reference's arguments)")
    J = int(joints_num)
    limit = max_joints()
    if J < 2 or J > limit:
        raise ValueError(f"{what}: {J} joints outside 2..{limit} (mst_rot_decode_max_joints)")
    F = 12 * J - 1 if route != "real_rot" else 9 * J + 1
    B, T, feats, sampler = _layout(what, sample.shape, F)
    if feats != F:
        raise ValueError(f"{what}: {feats} features, expected {'12 * J - 1' if route != 'real_rot' else '9 * J + 1'} = {F}, the row of route "
                         f"{route!r} at {J} joints")
    off = np.ascontiguousarray(offsets.detach().cpu().numpy() if torch.is_tensor(offsets) else np.asarray(offsets), dtype=np.float32)
    if off.shape != (J, 3):
        raise ValueError(f"{what}: offsets of shape {off.shape}, expected ({J}, 3)")
    chains = _checked_chains(what, chains, J)
    raw = face = None
    if route == "pos_ik":
        if raw_offsets is None or face_joint_indx is None:
            raise ValueError(f"{what}: route 'pos_ik' needs raw_offsets and face_joint_indx")
        raw = np.ascontiguousarray(raw_offsets.detach().cpu().numpy() if torch.is_tensor(raw_offsets) else np.asarray(raw_offsets),
                                   dtype=np.float32)
        if raw.shape != (J, 3):
            raise ValueError(f"{what}: raw_offsets of shape {raw.shape}, expected ({J}, 3)")
        face = [int(a) for a in face_joint_indx]
        if len(face) != 4 or any(not 0 <= a < J for a in face):
            raise ValueError(f"{what}: face_joint_indx {face}: four joints of 0..{J - 1} (r_hip, l_hip, sdr_r, sdr_l)")
    elif raw_offsets is not None or face_joint_indx is not None:
        raise ValueError(f"{what}: raw_offsets and face_joint_indx belong to route 'pos_ik', not {route!r}")
    if (mean is None) != (std is None):
        raise ValueError(f"{what}: mean and std come together")
    for name, v in (("mean", mean), ("std", std)):
        if v is not None and tuple(np.shape(v)) != (F,):
            raise ValueError(f"{what}: {name} of shape {tuple(np.shape(v))}, expected ({F},)")
    if B < 1 or T < 1:
        raise ValueError(f"{what}: {B} clips of {T} frames")
    if local and route != "real_rot":
        raise ValueError(f"{what}: the local rows (process_pos_from_real_rot) belong to route 'real_rot'")
    if not (quats or root_pos or joints or local):
        raise ValueError(f"{what}: no output asked for")
    frames = max_frames(J)
    if T > frames:
        raise RuntimeError(f"{what}: {T} frames > {frames}, the longest clip mst_rot_decode takes (mst_rot_decode_max_frames({J}))")
    ld = _checked_lengths(what, lengths, B, T, sample.device)
    if not sample.is_cuda or (ld is not None and not ld.is_cuda):
        raise RuntimeError(_NO_CPU.format(what))
    if route != "real_rot":
        parents, xoff, source = expand_chains(chains, off)
    else:
        parents, xoff, source = chain_parents(chains, J), off.copy(), None
        xoff[0] = 0
    Jx = len(parents)
    dev = sample.device
    data = sample.detach().to(torch.float32)
    if sampler:
        sb, sf, st = data.stride(0), data.stride(1), data.stride(3)
    else:
        sb, st, sf = data.stride()
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    q = new(B, T, Jx, 4) if quats else None
    rp = new(B, T, 3) if root_pos else None
    jp = new(B, T, J, 3) if joints else None
    lo = new(B, T, 3 * (J - 1)) if local else None
    m = None if mean is None else _stat(mean, dev)           # named: they must outlive the launch
    s = None if std is None else _stat(std, dev)
    flat = [j for c in chains for j in c]
    starts = [0]
    for c in chains:
        starts.append(starts[-1] + len(c))
    offs = (C.c_float * (3 * J))(*off.reshape(-1).tolist())
    with torch.cuda.device(dev):
        N.check(N.lib().mst_rot_decode(N.ptr(data), sb, st, sf, N.ptr(m), N.ptr(s), N.ptr(ld), B, T, F, J, ROUTES[route], _ints(flat),
                                       _ints(starts), len(chains), offs, None if face is None else _ints(face),
                                       None if raw is None else (C.c_float * (3 * J))(*raw.reshape(-1).tolist()),
                                       None if source is None else _ints(source),
                                       None if source is None else _ints(parents), Jx, N.ptr(q), N.ptr(rp), N.ptr(jp), N.ptr(lo),
                                       N.stream_ptr(dev)))
    anim = RotAnim(q, rp, parents, xoff)
    extra = tuple(t for t in (jp, lo) if t is not None)
    return (anim,) + extra if extra else anim


def save_rot_bvhs(paths, anim, lengths=None, frametime=FRAME_TIME):
    """A `RotAnim` batch written, one file per clip: one launch (`quats_to_channels`), one device-to-host copy, then text.  lengths [B]:
    the frames of each clip to write (None: all)."""
    if not isinstance(anim, RotAnim) or anim.quats is None or anim.root_pos is None:
        raise TypeError("save_rot_bvhs: anim is a RotAnim of decode_rotations with its quats and root_pos")
    B, T, Jx, _ = anim.quats.shape
    paths = list(paths)
    if len(paths) != B:
        raise ValueError(f"save_rot_bvhs: {len(paths)} paths for {B} clips")
    host = np.full(B, T, np.int64) if lengths is None else \
        (lengths.detach().cpu().numpy() if torch.is_tensor(lengths) else np.asarray(lengths)).reshape(-1).astype(np.int64)
    if host.shape[0] != B or host.min() < 1 or host.max() > T:
        raise ValueError(f"save_rot_bvhs: lengths {host.tolist()} for {B} clips of {T} frames")
    sk, _ = bvh.writer_skeleton(anim.names, anim.parents, anim.offsets, None, "zyx", False, frametime)
    ch = bvh.quats_to_channels(anim.quats, anim.root_pos, anim.parents).cpu().numpy()
    for b, p in enumerate(paths):
        with open(p, "w") as fh:
            fh.write(bvh.format_bvh(sk, ch[b, :host[b]]))


# ------------------------------------------------------------------------------------------ the reference's signatures
def _rows(what, data):
    """The reference's `data` -> (CUDA tensor [B, T, F], leading shape).  A CPU tensor is refused; a numpy array is uploaded."""
    if torch.is_tensor(data):
        if not data.is_cuda:
            raise RuntimeError(_NO_CPU.format(what))
        t = data
    else:
        if not torch.cuda.is_available():
            raise RuntimeError(_NO_CPU.format(what))
        t = torch.as_tensor(np.asarray(data, dtype=np.float32)).cuda()
    if t.dim() < 2:
        raise ValueError(f"{what}: data of shape {tuple(t.shape)}, expected [..., T, F]")
    lead = tuple(t.shape[:-1])
    return t.reshape((-1,) + tuple(t.shape[-2:])), lead


def _skeleton_parts(what, skeleton):
    for a in ("_offset", "_kinematic_tree", "_parents"):
        if not hasattr(skeleton, a):
            raise TypeError(f"{what}: skeleton has no `{a}` (anything with _offset, _kinematic_tree and _parents will do)")
    if skeleton._offset is None:
        raise ValueError(f"{what}: skeleton._offset is None (set_offset / get_offsets_joints first, as the reference needs)")
    return skeleton._kinematic_tree, skeleton._offset


def recover_from_rot(data, joints_num, skeleton):
    """The reference's `recover_from_rot`: data [..., T, 12 J - 1] -> joints [N, J, 3] over all N frames (its `view(-1, J, 6)`)."""
    chains, off = _skeleton_parts("recover_from_rot", skeleton)
    rows, _ = _rows("recover_from_rot", data)
    _, jp = decode_rotations(rows, joints_num, chains, off, route="hml_rot", joints=True, quats=False, root_pos=False)
    return jp.reshape(-1, int(joints_num), 3)


def recover_from_real_rot(data, joints_num, skeleton):
    """The reference's `recover_from_real_rot`: data [..., T, 9 J + 1] -> joints [..., T, J, 3]."""
    chains, off = _skeleton_parts("recover_from_real_rot", skeleton)
    rows, lead = _rows("recover_from_real_rot", data)
    _, jp = decode_rotations(rows, joints_num, chains, off, route="real_rot", joints=True, quats=False, root_pos=False)
    return jp.reshape(lead + (int(joints_num), 3))


def process_pos_from_real_rot(data, joints_num, skel):
    """The reference's `process_pos_from_real_rot`: data [..., T, 9 J + 1] -> the root-relative, un-rotated rows
    [..., T, 3 (J - 1)] (the module docstring has the deviation from what the reference's aliased subtraction returns)."""
    chains, off = _skeleton_parts("process_pos_from_real_rot", skel)
    rows, lead = _rows("process_pos_from_real_rot", data)
    _, lo = decode_rotations(rows, joints_num, chains, off, route="real_rot", local=True, quats=False, root_pos=False)
    return lo.reshape(lead + (3 * (int(joints_num) - 1),))


def _one_clip(what, data):
    rows, lead = _rows(what, data)
    if len(lead) != 1:
        raise ValueError(f"{what}: data of shape {tuple(lead) + (rows.shape[-1],)}, expected one clip [T, F]")
    return rows


def output_bvh(path, data, joints_num, kinematic_chain, tgt_offsets):
    """The reference's `output_bvh`: the 6D channels of one HumanML clip [T, 12 J - 1] written as a BVH file at 20 frames a second.
    -> the RotAnim that was written."""
    rows = _one_clip("output_bvh", data)
    anim = decode_rotations(rows, joints_num, kinematic_chain, tgt_offsets, route="hml_rot")
    save_rot_bvhs([path], anim)
    return anim


def output_bvh_from_real_rot(path, data, joints_num, kinematic_chain, tgt_offsets, names=None):
    """The reference's `output_bvh_from_real_rot`: the model's own rotations of one position-rotation clip [T, 9 J + 1] written as a BVH
    file, no fit.  -> the RotAnim that was written."""
    rows = _one_clip("output_bvh_from_real_rot", data)
    anim = decode_rotations(rows, joints_num, kinematic_chain, tgt_offsets, route="real_rot")
    anim.names = None if names is None else list(names)
    save_rot_bvhs([path], anim)
    return anim


def output_bvh_with_pos(path, data, joints_num, kinematic_chain, tgt_offsets, n_raw_offsets, face_joint_indx, bone_names=None):
    """The reference's `output_bvh_with_pos`: the POSITIONS of one HumanML clip [T, 12 J - 1] through the analytic chain IK, written as a
    BVH file.  bone_names: the expanded skeleton's names (J + chains of them), as the reference hands them to `Anim`.  -> the RotAnim."""
    rows = _one_clip("output_bvh_with_pos", data)
    anim = decode_rotations(rows, joints_num, kinematic_chain, tgt_offsets, route="pos_ik", raw_offsets=n_raw_offsets,
                            face_joint_indx=face_joint_indx)
    anim.names = None if bone_names is None else list(bone_names)
    save_rot_bvhs([path], anim)
    return anim


def output_bvh_with_22rot(path, pos_data, data, joints_num, kinematic_chain, tgt_offsets):
    raise NotImplementedError("output_bvh_with_22rot is not covered (no caller in the reference uses it); bvh.save_bvh writes given quaternions")


def fit_joints_bvh_quats(*args, **kwargs):
    raise NotImplementedError("fit_joints_bvh_quats is not covered (no caller in the reference uses it); fit_joints_bvh fits the 6D rotations")
