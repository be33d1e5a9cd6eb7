"""Drop-in names of the reference's utils/process_smpl_from_hybrik.py -- `downsample`, `joints_downsample`, `amass_to_pose`, `pos2hmlrep`
-- over utils/pose_track.py: numpy in, numpy out, the work on the GPU.

The reference loads two SMPL-H bodies, their DMPLs and an example clip from fixed relative paths when it is imported.  Nothing is loaded
here at import; `configure` sets what those files provided:

    from mst_amd.utils import process_smpl_from_hybrik as psh
    psh.configure(body=BodyJoints.from_npz("body_models/smplh/male/model.npz"),        # the reference poses every track with the male body
                  tgt_offsets=offsets_of_the_example_clip, raw_offsets=t2m_raw_offsets)  # [22, 3] each
    joints, est_joints = psh.amass_to_pose("track.pk", fps=30)
    rows = psh.pos2hmlrep(joints)                                                      # [T - 1, 263]

The deviations of utils/pose_track.py apply (the rate of a float through `limit_denominator(1000)`, the shorter arc and the closed-form
quaternion on matrix input, float32 results where the reference returns float64).  One more: the reference's `amass_to_pose` falls back
to the body model's joints inside a bare `except` when the estimator's joints cannot be resampled; here that fallback is taken exactly
when the file holds no such joints (`.pkl`), and every other error is raised."""
import numpy as np
import torch

from . import pose_track as pt

ex_fps = pt.MODEL_FPS
_state = {"body": None, "tgt_offsets": None, "raw_offsets": None, "chains": pt.T2M_CHAINS}


def configure(body=None, tgt_offsets=None, raw_offsets=None, chains=None):
    """body: a `BodyJoints`, an `SMPLBody` or the path of an SMPL / SMPL-H .npz (the reference's male_bm).  tgt_offsets [22, 3]: the bone
    offsets of the target skeleton (the reference takes them from frame 0 of HumanML3D's clip 001234 with `Skeleton.get_offsets_joints`).
    raw_offsets [22, 3]: HumanML3D's unit bone directions (t2m_raw_offsets).  chains: its kinematic chains (the default).  Arguments
    left None keep what was set before."""
    if body is not None:
        if isinstance(body, pt.BodyJoints):
            _state["body"] = body
        elif isinstance(body, (str, bytes)) or hasattr(body, "__fspath__"):
            _state["body"] = pt.BodyJoints.from_npz(body)
        elif hasattr(body, "J0") and hasattr(body, "Jdirs"):
            _state["body"] = pt.BodyJoints.from_body(body)
        else:
            raise TypeError(f"configure: body is a BodyJoints, an SMPLBody or an .npz path; got {type(body).__name__}")
    for name, v in (("tgt_offsets", tgt_offsets), ("raw_offsets", raw_offsets)):
        if v is not None:
            a = np.ascontiguousarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float32)
            if a.shape != (pt.CHAIN_JOINTS, 3):
                raise ValueError(f"configure: {name} of shape {a.shape}, expected ({pt.CHAIN_JOINTS}, 3)")
            _state[name] = a
    if chains is not None:
        _state["chains"] = [list(map(int, c)) for c in chains]


def _need(*names):
    missing = [n for n in names if _state[n] is None]
    if missing:
        raise RuntimeError(f"process_smpl_from_hybrik: {', '.join(missing)} not set; call configure(...) first (nothing is loaded from fixed "
                           "paths at import, unlike the reference)")


def _cuda(what, a):
    if not torch.cuda.is_available():
        raise RuntimeError(pt._NO_CPU.format(what))
    return torch.as_tensor(np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float32)).cuda()


def downsample(rotations, positions, downsample_rate):
    """rotations [T, J, 4], positions [T, 3] -> (rotations [K, J, 4], positions [K, 3]) float32 numpy, K = ceil((T - 1) * up / down):
    the reference's formula, the longer arc included when the signs of an interval's ends disagree."""
    q, p = _cuda("downsample", rotations), _cuda("downsample", positions)
    if q.dim() != 3 or p.dim() != 2:
        raise ValueError(f"downsample: rotations of shape {tuple(q.shape)} and positions of shape {tuple(p.shape)}, expected [T, J, 4] and [T, 3]")
    qo, po, _ = pt.resample_tracks(q[None], p[None, :, None], rate=pt.parse_rate(downsample_rate))
    return qo[0].cpu().numpy(), po[0, :, 0].cpu().numpy()


def joints_downsample(joints, downsample_rate):
    """joints [T, J, 3] -> [K, J, 3] float32 numpy."""
    p = _cuda("joints_downsample", joints)
    if p.dim() != 3:
        raise ValueError(f"joints_downsample: joints of shape {tuple(p.shape)}, expected [T, J, 3]")
    return pt.resample_tracks(None, p[None], rate=pt.parse_rate(downsample_rate))[1][0].cpu().numpy()


def amass_to_pose(src_path, fps=25, trans_path="", with_trans=False):
    """A pose estimator's file (`read_pose_track`: trusted input) -> (pose_seq [K, 22, 3], joints [K, 22, 3]) float32 numpy at 20 fps: the
    body model's joints and the estimator's own, both re-axed; the first twice where the file holds no joints of the estimator."""
    _need("body")
    track = pt.read_pose_track(src_path, trans_path)
    model, est, _ = pt.track_joints(track, _state["body"], fps, with_trans)
    model = model[0].cpu().numpy()
    return model, (model if est is None else est[0].cpu().numpy())


def pos2hmlrep(joints):
    """joints [T, 22, 3] -> the 263-feature rows [T - 1, 263] (numpy): `uniform_skeleton_basic` onto the configured target offsets, then
    `process_file` with feet threshold 0.002."""
    from .motion_process import process_file, uniform_skeleton_basic
    _need("tgt_offsets", "raw_offsets")
    raw, chains = _state["raw_offsets"], _state["chains"]
    moved = uniform_skeleton_basic(np.asarray(joints, np.float32), _state["tgt_offsets"], raw, chains, list(pt.T2M_LEGS), list(pt.T2M_FACE))
    return process_file(moved, list(pt.T2M_FACE), list(pt.T2M_FID_L), list(pt.T2M_FID_R), 0.002, raw, chains)[0]
