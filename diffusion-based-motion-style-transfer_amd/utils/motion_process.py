"""Post-sampling tensor ops on the GPU: counterparts of
`data_loaders/humanml/scripts/motion_process.py:444-461` (`recover_from_ric`) and the `inv_transform` that precedes it
in the reference's scripts (dataset.py:478-479), as one native launch -- batched sampling can emit joint positions
without the `.cpu()` round trip the scripts make."""
import ctypes as C

import numpy as np
import torch

from .. import _native as N


def _f32(t, dev):
    return torch.as_tensor(t, dtype=torch.float32).to(dev).contiguous()


def recover_joints(sample, mean, std, joints_num):
    """sample: [B, F, 1, T] normalised hml_vec GPU tensor (what p_sample_loop / ddim_sample_loop return);
    mean, std: [F].  Returns joint positions [B, 1, T, joints_num, 3] = recover_from_ric(inv_transform(permute(sample)))."""
    if not sample.is_cuda:
        raise RuntimeError("recover_joints runs on the GPU only (no CPU fallback); move the sample to cuda")
    x = sample.to(torch.float32).contiguous()
    B, F, one, T = x.shape
    assert one == 1, x.shape
    out = torch.empty(B, 1, T, joints_num, 3, dtype=torch.float32, device=x.device)
    m, s = _f32(mean, x.device), _f32(std, x.device)          # named: must outlive the launch (a freed temporary's block is
    N.check(N.lib().mst_recover_from_ric(N.ptr(x), N.ptr(m), N.ptr(s), B, F, T, joints_num,      # handed to the next allocation)
                                         N.ptr(out), N.stream_ptr(x.device)))
    return out


def recover_from_ric(data, joints_num):
    """Drop-in signature of the reference function: data [..., T, F] DENORMALISED rows -> [..., T, joints_num, 3]."""
    lead = data.shape[:-2]
    T, F = data.shape[-2:]
    x = data.reshape(-1, T, F).permute(0, 2, 1).unsqueeze(2)                 # [N, F, 1, T]
    out = recover_joints(x, torch.zeros(F), torch.ones(F), joints_num)       # [N, 1, T, J, 3]
    return out.reshape(*lead, T, joints_num, 3)


# ------------------------------------------------------------------------------------------ the opposite direction: joints -> features
# Counterparts of `process_file_with_rotation` (data_loaders/humanml/common/bvh_utils.py:1091-1287) and `process_file` (:898-1088)
# followed by `process_np_motion`'s normalisation and padding (data_loaders/humanml/data/dataset.py:484-519): one native launch, one
# workgroup per clip (csrc/mst_encode.h).
_NO_CPU = "{} runs on the GPU only (no CPU fallback); move the motion to cuda"
POSROT, HML = "posrot", "hml"
_MODES = {POSROT: 0, HML: 1}


def encode_feats(joints, mode):
    """Feature count of a mode: 9 J + 1 (POSROT) or 12 J - 1 (HML)."""
    return 9 * joints + 1 if mode == POSROT else 12 * joints - 1


def encode_max_frames(joints, mode=POSROT):
    """Longest clip `encode_joints` takes (mst_encode_max_frames)."""
    n = int(N.lib().mst_encode_max_frames(int(joints), _MODES[mode]))
    if n < 0:
        N.check(1)
    return n


def _encode_validate(what, pos_shape, rot_shape, mode, chains, raw_offsets, face_joint_indx, fid_l, fid_r, mean, std, frames_out):
    """Everything that can be refused without a GPU.  -> (mode, frames_out, face, feet, flattened chains, starts, offsets or None)."""
    if mode is None:
        mode = POSROT if rot_shape is not None else HML
    if mode not in _MODES:
        raise ValueError(f"{what}: mode {mode!r} is none of {tuple(_MODES)}")
    if len(pos_shape) != 4 or pos_shape[-1] != 3:
        raise ValueError(f"{what}: positions of shape {tuple(pos_shape)}, expected [B, T, J, 3]")
    B, T, J, _ = pos_shape
    if J < 2 or J > 24:
        raise ValueError(f"{what}: {J} joints outside 2..24")
    if B < 1:
        raise ValueError(f"{what}: {B} clips")
    if T < 2:
        raise IndexError(f"{what}: a clip of {T} frame has no velocity row; at least 2 frames are needed")
    if mode == POSROT and rot_shape is None:
        raise ValueError(f"{what}: mode {POSROT!r} needs the rotations")
    if rot_shape is not None and tuple(rot_shape) != (B, T, J, 4):
        raise ValueError(f"{what}: rotations of shape {tuple(rot_shape)}, expected [{B}, {T}, {J}, 4]")
    face = [int(i) for i in face_joint_indx]
    if len(face) != 4:
        raise ValueError(f"{what}: four face joints are needed (r_hip, l_hip, sdr_r, sdr_l), got {len(face)}")
    if min(face) < 0 or max(face) >= J:
        raise ValueError(f"{what}: face joints {face} outside 0..{J - 1}")
    if len(set(face)) != 4:
        raise ValueError(f"{what}: duplicate face joints {face}")
    feet = [int(i) for i in fid_l] + [int(i) for i in fid_r]
    if len(fid_l) != 2 or len(fid_r) != 2:
        raise ValueError(f"{what}: two foot joints a side are needed, got {list(fid_l)} and {list(fid_r)}")
    if min(feet) < 0 or max(feet) >= J:
        raise ValueError(f"{what}: foot joints {feet} outside 0..{J - 1}")
    flat, starts, placed = [], [0], {0}
    for c, chain in enumerate(chains):
        chain = [int(j) for j in chain]
        if not chain:
            raise ValueError(f"{what}: chain {c} is empty")
        if min(chain) < 0 or max(chain) >= J:
            raise ValueError(f"{what}: chain {c} names a joint outside 0..{J - 1}")
        if chain[0] not in placed:
            raise ValueError(f"{what}: chain {c} starts at joint {chain[0]}, which no earlier chain has placed")
        for j in chain[1:]:
            if j in placed:
                raise ValueError(f"{what}: joint {j} is named twice as a child (chain {c})")
            placed.add(j)
        flat += chain
        starts.append(len(flat))
    if mode == HML and not flat:
        raise ValueError(f"{what}: mode {HML!r} needs the kinematic chains")
    off = None
    if raw_offsets is not None:
        off = raw_offsets.detach().cpu().numpy() if torch.is_tensor(raw_offsets) else np.asarray(raw_offsets)
        off = np.ascontiguousarray(off, dtype=np.float32)
        if off.shape != (J, 3):
            raise ValueError(f"{what}: raw offsets of shape {off.shape}, expected ({J}, 3)")
    elif mode == HML:
        raise ValueError(f"{what}: mode {HML!r} needs the raw offsets")
    F = encode_feats(J, mode)
    if (mean is None) != (std is None):
        raise ValueError(f"{what}: mean and std come together")
    for name, v in (("mean", mean), ("std", std)):
        if v is not None and tuple(np.shape(v)) != (F,):
            raise ValueError(f"{what}: {name} of shape {tuple(np.shape(v))}, expected ({F},)")
    frames_out = T if frames_out is None else int(frames_out)
    if frames_out < 1:
        raise ValueError(f"{what}: frames_out {frames_out} < 1")
    limit = encode_max_frames(J, mode)
    if T > limit:
        raise RuntimeError(f"{what}: {T} frames > {limit}, the longest clip mst_encode_motion takes (mst_encode_max_frames({J}, {mode!r}))")
    return mode, frames_out, face, feet, flat, starts, off


def _encode_lengths(what, lengths, B, T, device):
    """-> int32 device tensor [B] or None.  Checked on the host (a CUDA tensor is copied back once for it): 2 <= len <= T."""
    if lengths is None:
        return None
    host = lengths.detach().cpu().numpy() if torch.is_tensor(lengths) else np.asarray(lengths)
    host = host.reshape(-1).astype(np.int64)
    if host.shape[0] != B:
        raise ValueError(f"{what}: {host.shape[0]} lengths for {B} clips")
    if host.min() < 2 or host.max() > T:
        raise ValueError(f"{what}: lengths {host.min()}..{host.max()} outside 2..{T}")
    if torch.is_tensor(lengths) and lengths.is_cuda and lengths.dtype == torch.int32 and lengths.is_contiguous():
        return lengths
    return torch.from_numpy(host.astype(np.int32)).to(device)


def encode_joints(positions, rotations=None, *, chains, raw_offsets, face_joint_indx, fid_l, fid_r, feet_thre=0.002, mode=None, lengths=None,
                  mean=None, std=None, frames_out=None, return_aux=False):
    """Joint positions [B, T, J, 3] (and, in POSROT, joint rotations [B, T, J, 4] as w, x, y, z quaternions) -> (sample [B, F, 1,
    frames_out] in the samplers' layout, lengths int32 [B]).  mode "posrot" (the default when rotations are given; F = 9 J + 1,
    `process_file_with_rotation`) or "hml" (F = 12 J - 1, `process_file`: rotations from the chain IK, local velocities, foot contacts).
    chains: the kinematic chains (HML's IK follows them, every chain restarting from the frame's root rotation, as in the reference);
    raw_offsets [J, 3]: the unit bone directions (HML); face_joint_indx: r_hip, l_hip, sdr_r, sdr_l; fid_l, fid_r: two foot joints a side.
    lengths [B]: every stage sees frames 0 .. len-1 of a clip.  Row t < min(len - 1, frames_out) of the sample is the clip's feature row
    (normalised as (row - mean) / std when mean / std [F] are given), every later one exact zeros; the returned lengths are those row
    counts.  frames_out defaults to T.  return_aux: also (global_positions [B, T, J, 3], local positions [B, T, J, 3], l_velocity
    [B, T-1, 2]), zero past a clip.  The inputs are not modified.  Everything is validated before the launch, which is enqueued on the
    caller's current stream; the host is not synchronised after the lengths check."""
    if not torch.is_tensor(positions) or (rotations is not None and not torch.is_tensor(rotations)):
        raise TypeError("encode_joints: positions and rotations are tensors (process_file takes the reference's numpy clip)")
    mode, fo, face, feet, flat, starts, off = _encode_validate(
        "encode_joints", positions.shape, None if rotations is None else rotations.shape, mode, chains, raw_offsets, face_joint_indx,
        fid_l, fid_r, mean, std, frames_out)
    B, T, J, _ = positions.shape
    ld = _encode_lengths("encode_joints", lengths, B, T, positions.device)
    if any(t is not None and not t.is_cuda for t in (positions, rotations, ld)):
        raise RuntimeError(_NO_CPU.format("encode_joints"))
    dev = positions.device
    pos = positions.detach().to(torch.float32).contiguous()
    rot = None if rotations is None or mode == HML else rotations.detach().to(torch.float32).contiguous()
    F = encode_feats(J, mode)
    sample = torch.empty(B, F, 1, fo, dtype=torch.float32, device=dev)
    out_len = torch.empty(B, dtype=torch.int32, device=dev)
    aux = tuple(torch.empty(*s, dtype=torch.float32, device=dev) for s in ((B, T, J, 3), (B, T, J, 3), (B, T - 1, 2))) if return_aux \
        else (None, None, None)
    m = None if mean is None else _f32(mean, dev)             # named: they must outlive the launch
    s = None if std is None else _f32(std, dev)
    ints = lambda v: (C.c_int32 * max(len(v), 1))(*v)
    offs = None if off is None else (C.c_float * (3 * J))(*off.reshape(-1).tolist())
    with torch.cuda.device(dev):
        N.check(N.lib().mst_encode_motion(N.ptr(pos), N.ptr(rot), N.ptr(ld), N.ptr(m), N.ptr(s), B, T, J, _MODES[mode], ints(face), ints(feet),
                                          ints(flat), ints(starts), len(starts) - 1, offs, float(feet_thre), fo, N.ptr(sample),
                                          N.ptr(out_len), N.ptr(aux[0]), N.ptr(aux[1]), N.ptr(aux[2]), N.stream_ptr(dev)))
    return (sample, out_len) + (aux if return_aux else ())


def _process(what, positions, rotations, face_joint_indx, fid_l, fid_r, feet_thre, n_raw_offsets, kinematic_chain):
    as_numpy = not torch.is_tensor(positions)
    pos = torch.as_tensor(np.asarray(positions, dtype=np.float32)) if as_numpy else positions
    rot = None
    if rotations is not None:
        rot = rotations if torch.is_tensor(rotations) else torch.as_tensor(np.asarray(rotations, dtype=np.float32))
    if pos.dim() != 3:
        raise ValueError(f"{what}: positions of shape {tuple(pos.shape)}, expected one clip [T, J, 3]")
    mode = HML if rot is None else POSROT
    _encode_validate(what, pos[None].shape, None if rot is None else rot[None].shape, mode, kinematic_chain, n_raw_offsets, face_joint_indx,
                     fid_l, fid_r, None, None, None)
    if not pos.is_cuda and torch.cuda.is_available():
        pos = pos.cuda()
    if not pos.is_cuda:
        raise RuntimeError(_NO_CPU.format(what))
    rot = None if rot is None else rot.to(pos.device)
    T = pos.shape[0]
    sample, _, glob, local, lvel = encode_joints(pos[None], None if rot is None else rot[None], chains=kinematic_chain,
                                                 raw_offsets=n_raw_offsets, face_joint_indx=face_joint_indx, fid_l=fid_l, fid_r=fid_r,
                                                 feet_thre=feet_thre, mode=mode, frames_out=T - 1, return_aux=True)
    out = (sample[0, :, 0, :].t().contiguous(), glob[0], local[0], lvel[0])
    return tuple(t.cpu().numpy() for t in out) if as_numpy else out


def process_file_with_rotation(positions, rotations, face_joint_indx, fid_l, fid_r, feet_thre, n_raw_offsets, kinematic_chain):
    """The reference's `process_file_with_rotation`, positional signature: one clip [T, J, 3] with rotations [T, J, 4], numpy (numpy comes
    back) or tensors.  -> (data [T-1, 9J+1], global_positions [T, J, 3], positions [T, J, 3], l_velocity [T-1, 2]).  Neither argument is
    modified (the reference rewrites both in place)."""
    return _process("process_file_with_rotation", positions, rotations, face_joint_indx, fid_l, fid_r, feet_thre, n_raw_offsets,
                    kinematic_chain)


def process_file(positions, face_joint_indx, fid_l, fid_r, feet_thre, n_raw_offsets, kinematic_chain):
    """The reference's `process_file`, positional signature: one clip [T, J, 3], numpy (numpy comes back) or a tensor.
    -> (data [T-1, 12J-1], global_positions [T, J, 3], positions [T, J, 3], l_velocity [T-1, 2]).  A zero-length bone in the raw offsets
    or the clip gives NaN in that joint's rotation columns, as in the reference."""
    return _process("process_file", positions, None, face_joint_indx, fid_l, fid_r, feet_thre, n_raw_offsets, kinematic_chain)


# ------------------------------------------------------------------------------------------ one skeleton for every clip
# Counterpart of `uniform_skeleton_basic` (data_loaders/humanml/scripts/motion_process.py:12-35; `uniform_skeleton` with its globals made
# arguments): one native launch for a batch, one workgroup per clip (k_retarget, csrc/mst_bvh.h).
def retarget_max_frames(joints):
    """Longest clip `retarget_joints` takes (mst_retarget_max_frames)."""
    n = int(N.lib().mst_retarget_max_frames(int(joints)))
    if n < 0:
        N.check(1)
    return n


def retarget_joints(positions, target_offset, raw_offsets, chains, l_idx, face_joint_indx, lengths=None):
    """Joint positions [B, T, J, 3] moved onto the skeleton with bone offsets `target_offset` [J, 3] -> [B, T, J, 3].  Per clip: the source
    offsets are frame 0's bone lengths along `raw_offsets` [J, 3]; the root is scaled by the ratio of leg lengths, each the sum over the two
    joints `l_idx` of the offset's largest absolute component (the reference's measure, not a norm); the chain IK (smooth_forward=False,
    frame 0's root quaternion the identity, every chain restarting from the root quaternion) gives the rotations and the forward kinematics
    with the target offsets the result.  lengths [B]: 1 <= len <= T; frames past a clip are exact zeros.  A joint no chain names comes
    back as zeros and a zero-length bone gives NaN, both as in the reference.  The input is not modified; one launch on the caller's
    current stream."""
    what = "retarget_joints"
    if not torch.is_tensor(positions):
        raise TypeError(f"{what}: positions is a tensor (uniform_skeleton_basic takes the reference's numpy clip)")
    if positions.dim() != 4 or positions.shape[-1] != 3:
        raise ValueError(f"{what}: positions of shape {tuple(positions.shape)}, expected [B, T, J, 3]")
    B, T, J, _ = positions.shape
    if J < 2 or J > 24:
        raise ValueError(f"{what}: {J} joints outside 2..24")
    if B < 1 or T < 1:
        raise ValueError(f"{what}: {B} clips of {T} frames")
    _, _, face, _, flat, starts, off = _encode_validate(what, (B, 2, J, 3), None, HML, chains, raw_offsets, face_joint_indx, (0, 0), (0, 0),
                                                        None, None, None)
    tgt = target_offset.detach().cpu().numpy() if torch.is_tensor(target_offset) else np.asarray(target_offset)
    tgt = np.ascontiguousarray(tgt, dtype=np.float32)
    if tgt.shape != (J, 3):
        raise ValueError(f"{what}: target offsets of shape {tgt.shape}, expected ({J}, 3)")
    legs = [int(i) for i in l_idx]
    if len(legs) != 2 or min(legs) < 1 or max(legs) >= J:
        raise ValueError(f"{what}: l_idx {list(l_idx)}: two joints of 1..{J - 1} are needed")
    host = None
    if lengths is not None:
        host = lengths.detach().cpu().numpy() if torch.is_tensor(lengths) else np.asarray(lengths)
        host = host.reshape(-1).astype(np.int64)
        if host.shape[0] != B:
            raise ValueError(f"{what}: {host.shape[0]} lengths for {B} clips")
        if host.min() < 1 or host.max() > T:
            raise ValueError(f"{what}: lengths {host.min()}..{host.max()} outside 1..{T}")
    if not positions.is_cuda or (torch.is_tensor(lengths) and not lengths.is_cuda):
        raise RuntimeError(_NO_CPU.format(what))
    limit = retarget_max_frames(J)
    if T > limit:
        raise RuntimeError(f"{what}: {T} frames > {limit}, the longest clip mst_retarget_joints takes (mst_retarget_max_frames({J}))")
    dev = positions.device
    pos = positions.detach().to(torch.float32).contiguous()
    ld = None if host is None else torch.from_numpy(host.astype(np.int32)).to(dev)
    out = torch.empty(B, T, J, 3, dtype=torch.float32, device=dev)
    ints = lambda v: (C.c_int32 * max(len(v), 1))(*v)
    floats = lambda a: (C.c_float * a.size)(*a.reshape(-1).tolist())
    with torch.cuda.device(dev):
        N.check(N.lib().mst_retarget_joints(N.ptr(pos), N.ptr(ld), B, T, J, ints(face), ints(flat), ints(starts), len(starts) - 1, floats(off),
                                            floats(tgt), ints(legs), N.ptr(out), N.stream_ptr(dev)))
    return out


def uniform_skeleton_basic(positions, target_offset, n_raw_offsets, kinematic_chain, l_idx, face_joint_indx):
    """The reference's `uniform_skeleton_basic`, positional signature: one clip [T, J, 3], numpy (numpy comes back) or a tensor."""
    as_numpy = not torch.is_tensor(positions)
    pos = torch.as_tensor(np.asarray(positions, dtype=np.float32)) if as_numpy else positions
    if pos.dim() != 3:
        raise ValueError(f"uniform_skeleton_basic: positions of shape {tuple(pos.shape)}, expected one clip [T, J, 3]")
    if not pos.is_cuda and as_numpy and torch.cuda.is_available():
        pos = pos.cuda()
    out = retarget_joints(pos[None], target_offset, n_raw_offsets, kinematic_chain, l_idx, face_joint_indx)[0]
    return out.cpu().numpy() if as_numpy else out
