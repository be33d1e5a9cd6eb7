"""Foot-skate cleanup on the GPU: counterparts of `remove_fs` (data_loaders/humanml/common/bvh_utils.py:1685-1809), its contact detectors
(`get_foot_contact_by_vel_acc` :1591-1639, `get_foot_contact_by_vel3` :1642-1682), its `Butterworth` low-pass (:1872-1916) and
`get_ee_id_by_names` (:1566-1573).  One native launch per pass, one workgroup per clip (csrc/mst_feet.h); `clean_joints` is what
sample/demo_style_transfer.py:310-313 does to a finished sample -- recover_from_ric, then two passes -- without the clip leaving the GPU.
Left out, as no caller uses them: `ref_height`, and `output_path`, which the reference ignores too."""
import ctypes as C

import numpy as np
import torch

from .. import _native as N
from .motion_process import recover_joints

_NO_CPU = "{} runs on the GPU only (no CPU fallback); move the motion to cuda"
MODES = ("vel_acc", "vel3")


def ee_ids_by_names(bonenames, ee_names=("RightToeBase", "LeftToeBase", "LeftFoot", "RightFoot")):
    """`get_ee_id_by_names`: indices of the end effectors in `bonenames`, a `prefix:` stripped from every bone name first -- on a copy
    (the reference rewrites the caller's list)."""
    names = [n.split(":")[1] if ":" in n else n for n in bonenames]
    ids = []
    for ee in ee_names:
        if ee not in names:
            raise ValueError(f"remove_fs: end effector {ee!r} is not among the bone names")
        ids.append(names.index(ee))
    return ids


def _check_ids(ee_ids, J):
    ids = [int(i) for i in ee_ids]
    if len(ids) != 4:
        raise ValueError(f"remove_fs: four end-effector ids are needed, got {len(ids)}")
    if len(set(ids)) != 4:
        raise ValueError(f"remove_fs: duplicate end-effector ids {ids}")
    if min(ids) < 0 or max(ids) >= J:
        raise ValueError(f"remove_fs: end-effector ids {ids} outside 0..{J - 1}")
    return ids


def max_frames(joints):
    """Longest clip `remove_fs` takes at this joint count (mst_remove_fs_max_frames)."""
    n = int(N.lib().mst_remove_fs_max_frames(int(joints)))
    if n < 0:
        N.check(1)
    return n


def _checked_lengths(lengths, B, T, device):
    """-> int32 device tensor [B], or None.  The values are checked here, on the host (a CUDA tensor is copied back once for it): the
    kernel trusts them."""
    if lengths is None:
        return None
    host = lengths.detach().cpu().numpy() if torch.is_tensor(lengths) else np.asarray(lengths)
    host = host.reshape(-1).astype(np.int64)
    if host.shape[0] != B:
        raise ValueError(f"remove_fs: {host.shape[0]} lengths for {B} clips")
    if host.min() < 2 or host.max() > T:
        raise ValueError(f"remove_fs: lengths {host.min()}..{host.max()} outside 2..{T}")
    if torch.is_tensor(lengths) and lengths.is_cuda and lengths.dtype == torch.int32 and lengths.is_contiguous():
        return lengths
    return torch.from_numpy(host.astype(np.int32)).to(device)


def _validate(what, shape, ref, ee_ids):
    """Everything that can be refused without a GPU: shapes, ids, frame count, the limit.  -> the four ids."""
    if len(shape) != 4 or shape[-1] != 3:
        raise ValueError(f"{what}: motion of shape {tuple(shape)}, expected [B, T, J, 3]")
    B, T, J, _ = shape
    if ref is not None and (ref.dim() != 4 or ref.shape[0] not in (1, B) or tuple(ref.shape[1:]) != (T, J, 3)):
        raise ValueError(f"{what}: reference motion of shape {tuple(ref.shape)}, expected [{B} or 1, {T}, {J}, 3]")
    ids = _check_ids(ee_ids, J)
    if T < 2:
        raise IndexError(f"{what}: a clip of {T} frame has no velocity; at least 2 frames are needed (the reference raises IndexError too)")
    limit = max_frames(J)
    if T > limit:
        raise RuntimeError(f"{what}: {T} frames > {limit}, the longest clip mst_remove_fs takes (mst_remove_fs_max_frames({J}))")
    return ids


def _need_cuda(what, *tensors):
    if any(t is not None and not t.is_cuda for t in tensors):
        raise RuntimeError(_NO_CPU.format(what))


def _launch(glb, ref, ids, lengths, *, use_vel3, thr, use_window=False, force_on_floor=False, interp_length=5, filter_before=False,
            filter_after=False, out=None, contacts=None, foot_vels=None, workspace=None):
    """One mst_remove_fs launch on the current stream of glb's device.  glb, ref, out: contiguous fp32 CUDA tensors, already validated."""
    B, T, J, _ = glb.shape
    if int(interp_length) < 0:
        raise ValueError(f"remove_fs: interp_length {interp_length} < 0")
    fid = (C.c_int32 * 4)(*ids)
    if out is not None and (filter_before or filter_after) and workspace is None:
        workspace = torch.empty(B * (T - 1) * J * 3, dtype=torch.float64, device=glb.device)
    with torch.cuda.device(glb.device):
        N.check(N.lib().mst_remove_fs(N.ptr(glb), N.ptr(ref), 0 if ref is None else ref.shape[0], N.ptr(lengths), B, T, J, fid,
                                      int(bool(use_vel3)), float(thr), int(bool(use_window)), int(bool(force_on_floor)), int(interp_length),
                                      int(bool(filter_before)), int(bool(filter_after)), N.ptr(out), N.ptr(contacts), N.ptr(foot_vels),
                                      N.ptr(workspace), 0 if workspace is None else workspace.numel() * 8, N.stream_ptr(glb.device)))
    return workspace


def _f32(t):
    return t.to(torch.float32).contiguous()


def _same_memory(a, b):
    return a is b or (a.data_ptr() == b.data_ptr() and a.shape == b.shape)


def foot_contacts(ref, ee_ids, mode="vel_acc", thr=0.003, use_window=False, lengths=None):
    """Contacts and the velocities they were decided on, alone.  ref: [B, T, J, 3] CUDA tensor; mode "vel_acc" (y-velocity against `thr`
    with the acceleration sign, OR a sign change; `use_window`: the window-3, 0.006 height refinement) or "vel3" (speed < thr).
    -> (contacts [B, T, 4] int32, foot_vels [B, T-1, 4]: speeds for vel3, y-velocities for vel_acc); zero from a clip's length on."""
    if mode not in MODES:
        raise ValueError(f"foot_contacts: mode {mode!r} is none of {MODES}")
    ids = _validate("foot_contacts", ref.shape, None, ee_ids)
    B, T = ref.shape[:2]
    ld = _checked_lengths(lengths, B, T, ref.device)
    _need_cuda("foot_contacts", ref)
    ref = _f32(ref)
    contacts = torch.empty(B, T, 4, dtype=torch.int32, device=ref.device)
    vels = torch.empty(B, T - 1, 4, dtype=torch.float32, device=ref.device)
    _launch(ref, None, ids, ld, use_vel3=mode == "vel3", thr=thr, use_window=use_window, contacts=contacts, foot_vels=vels)
    return contacts, vels


def _remove_fs_tensors(glb, ref, ids, ld, out=None, workspace=None, outputs=True, **kw):
    """glb [B, T, J, 3] fp32 contiguous CUDA; ref None or [B or 1, T, J, 3]; ld: checked lengths on the device or None; out None (a new
    tensor) or where to write (may be glb)."""
    B, T = glb.shape[:2]
    if out is None:
        out = torch.empty_like(glb)
    contacts = torch.empty(B, T, 4, dtype=torch.int32, device=glb.device) if outputs else None
    vels = torch.empty(B, T - 1, 4, dtype=torch.float32, device=glb.device) if outputs else None
    workspace = _launch(glb, ref, ids, ld, out=out, contacts=contacts, foot_vels=vels, workspace=workspace, **kw)
    return out, vels, contacts, workspace


def remove_fs(output_path, glb_motion, ref_motion, bonenames, ee_names, interp_length=5, force_on_floor=False, use_window=False,
              use_vel3=False, use_butterworth=False, vel3_thr=0.01, after_butterworth=False, *, lengths=None, out=None):
    """The reference's `remove_fs`, signature and defaults: floor shift, contact detection on `ref_motion` (vel_acc with threshold 0.003,
    or vel3 with `vel3_thr`), every contact run replaced by its mean (y = 0 under `force_on_floor`), the frames within `interp_length` of
    a run blended towards it, a Butterworth low-pass before (`use_butterworth`, cut-off 3) and after (`after_butterworth`, cut-off 2.5).
    -> (glb_motion, foot_vels, contacts, butter_motion); butter_motion is a copy of the reference motion, as in the reference (whose
    detectors leave the end-effector rows as they are).

    glb_motion: the reference's [T, J, 3] numpy array -- numpy comes back -- or a [B, T, J, 3] CUDA tensor -- tensors come back
    ([B, T, J, 3], [B, T-1, 4], [B, T, 4] int32, [B or 1, T, J, 3]).  ref_motion: the same kind, [B or 1, ...] for tensors, or None /
    glb_motion itself for the clip as it is on entry.  Tensor form only: `lengths` [B] (every stage sees frames 0 .. len-1 of a clip, as the
    demo's `[:length]` slice; later frames are returned as they came) and `out`, a tensor to write instead of a new one (glb_motion
    itself: in place).  Nothing is mutated otherwise: not the motions, not `bonenames`."""
    ids = ee_ids_by_names(bonenames, ee_names)
    as_numpy = not torch.is_tensor(glb_motion)
    if as_numpy:
        if lengths is not None or out is not None:
            raise ValueError("remove_fs: lengths= and out= belong to the tensor form; slice the numpy clip instead")
        g = np.asarray(glb_motion)
        if g.ndim != 3:
            raise ValueError(f"remove_fs: numpy motion of shape {g.shape}, expected [T, J, 3]")
        glb = torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32))[None]
        ref = None if ref_motion is None or ref_motion is glb_motion else \
            torch.from_numpy(np.ascontiguousarray(np.asarray(ref_motion), dtype=np.float32))[None]
    else:
        glb = glb_motion
        ref = None if ref_motion is None or _same_memory(ref_motion, glb_motion) else ref_motion
    _validate("remove_fs", glb.shape, ref, ids)
    ld = _checked_lengths(lengths, glb.shape[0], glb.shape[1], glb.device)
    if as_numpy and torch.cuda.is_available():
        glb, ref = glb.cuda(), None if ref is None else ref.cuda()
    _need_cuda("remove_fs", glb, ref, ld)
    glb = _f32(glb)
    ref = None if ref is None else _f32(ref)
    if out is not None and (not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.shape != glb.shape):
        raise ValueError("remove_fs: out= must be a contiguous fp32 CUDA tensor of the motion's shape")
    butter = (glb if ref is None else ref).clone()
    cleaned, vels, contacts, _ = _remove_fs_tensors(
        glb, ref, ids, ld, out=out, use_vel3=use_vel3, thr=vel3_thr if use_vel3 else 0.003, use_window=use_window,
        force_on_floor=force_on_floor, interp_length=interp_length, filter_before=use_butterworth, filter_after=after_butterworth)
    if as_numpy:
        return tuple(t[0].cpu().numpy() for t in (cleaned, vels, contacts, butter))
    return cleaned, vels, contacts, butter


def clean_joints(sample, mean, std, joints_num, ee_ids, ref_joints=None, lengths=None, passes=2, vel3_thr=0.05, interp_length=5,
                 force_on_floor=True, after_butterworth=True, *, _lengths_checked=False):
    """`recover_joints` followed by the demo's passes (sample/demo_style_transfer.py:310-313; the defaults are the demo's settings):
    pass 1 detects contacts on `ref_joints` ([B or 1, T, J, 3], the content motion; None: the clip itself), later passes on the clip
    itself.  sample: [B, F, 1, T] normalised hml_vec CUDA tensor; lengths: [B].  -> joints [B, T, J, 3].
    Every launch is enqueued on the caller's current stream, with no host copy or synchronisation between them (lengths are checked,
    and a host array of them uploaded, before the first; `_lengths_checked`: the caller, joint_fit.fit_clean_joints, has done that and
    passes the device tensor)."""
    if not sample.is_cuda:
        raise RuntimeError(_NO_CPU.format("clean_joints"))
    B, T = sample.shape[0], sample.shape[-1]
    if ref_joints is not None and ref_joints.dim() == 5:
        ref_joints = ref_joints[:, 0]                       # recover_joints's own layout
    ids = _validate("clean_joints", (B, T, joints_num, 3), ref_joints, ee_ids)
    ld = lengths if _lengths_checked else _checked_lengths(lengths, B, T, sample.device)
    _need_cuda("clean_joints", ref_joints)
    joints = recover_joints(sample, mean, std, joints_num)[:, 0]
    ref = None if ref_joints is None else _f32(ref_joints)
    ws = None
    for k in range(int(passes)):
        ws = _remove_fs_tensors(joints, ref if k == 0 else None, ids, ld, out=joints, workspace=ws,
                                outputs=False, use_vel3=True, thr=vel3_thr, force_on_floor=force_on_floor, interp_length=interp_length,
                                filter_after=after_butterworth)[3]
    return joints
