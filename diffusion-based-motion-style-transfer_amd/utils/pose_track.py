"""Style examples and content clips from a video pose estimator's track: the counterpart of utils/process_smpl_from_hybrik.py
(`downsample`, `joints_downsample`, `amass_to_pose`, `pos2hmlrep`).  The reference resamples with `qslerp` / `lerp`, converts to axis-angle
and runs a body model frame by frame in a Python loop; here a batch of tracks is one launch (csrc/mst_track.h):

  resample_tracks    quaternion tracks of any joint count and point tracks to a rational rate (k_track_resample); also what
                     `utils.bvh.read_bvh_resampled` uses for a fractional `downsample_rate`
  track_joints       rotations (quaternions or matrices), shape and translation -> the 22 joints at the model's 20 fps, re-axed as the
                     reference does, and the estimator's own joint track beside them (k_track_joints)
  track_to_features  track_joints + retarget_joints + encode_joints: normalised, padded sample tensors without leaving the device
  read_pose_track    the three file formats `amass_to_pose` reads; BodyJoints: the joint table of the user's own SMPL / SMPL-H file

Nothing here has a CPU path; rates, files and every argument check need no GPU.

The output frames.  The reference resamples intervals: (T - 1) * up up-sampled frames, then every down-th, so a clip of T frames gives
ceil((T - 1) * up / down) -- the source's last frame is dropped, even at rate 1.  That is kept.

Stated deviations from the reference:
  * the rate of a float.  The reference takes `Fraction(fps / 20)` exactly, which only works where the quotient is dyadic (25 and 30 fps):
    24 fps gives 5404319552844595/4503599627370496 and the up-sampling then tries to allocate that many frames.  Here a float goes
    through `Fraction(x).limit_denominator(1000)` (24 fps: 6/5); a `Fraction` or an (int, int) pair is taken as it is.
  * rotation matrices (`.pt`, `.pk`).  The reference's `rotm2q` takes the quaternion from `torch.linalg.eig`, so its sign is whatever
    LAPACK returns, and `qslerp` does not take the shorter arc: the reference's in-between frames depend on that sign.  Here the quaternion
    is the closed form of the same eigenvector and the shorter arc is always taken for matrix input (`shortest`, also offered for
    quaternion input); the frames whose parameter t is 0 equal the reference's.
  * arithmetic.  Rotations run in float32 throughout (the reference's theta = t * theta0 and its sine and cosine are float64 because its
    `t` is); points and translations are interpolated in double and stored as float32 (the reference returns them float64)."""
import ctypes as C
import pickle
from dataclasses import dataclass
from fractions import Fraction
from typing import Optional

import numpy as np
import torch

from .. import _native as N

_NO_CPU = "{} runs on the GPU only (no CPU fallback); move the track to cuda"
CHAIN_JOINTS = 22
NUM_BETAS = 10
MODEL_FPS = 20                               # the reference's ex_fps
MAX_RATE = 100000                            # up and down, each (mst_track_resample)
# HumanML3D's 22-joint skeleton as `pos2hmlrep` uses it: the kinematic chains, the face joints (r_hip, l_hip, sdr_r, sdr_l), the feet
# and the two leg joints whose offsets set the scale
T2M_CHAINS = [[0, 2, 5, 8, 11], [0, 1, 4, 7, 10], [0, 3, 6, 9, 12, 15], [9, 14, 17, 19, 21], [9, 13, 16, 18, 20]]
T2M_FACE, T2M_FID_L, T2M_FID_R, T2M_LEGS = (2, 1, 17, 16), (7, 10), (8, 11), (5, 8)


# ------------------------------------------------------------------------------------------ rates
def decimal_to_fraction(decimal_number):
    """The reference's `decimal_to_fraction` (bvh_utils.py:254-263): the number's own decimal text, digit by digit, then
    `limit_denominator()`.  A text without a '.' (an int, '3') is refused there by its `split`; here it is the integer."""
    text = str(decimal_number)
    if "." not in text:
        return Fraction(int(text))
    whole, digits = text.split(".")
    if "e" in digits.lower():
        raise ValueError(f"decimal_to_fraction: {text!r} is not written as whole.digits")
    den = 10 ** len(digits)
    return Fraction(int(digits) + int(whole) * den, den).limit_denominator()


def _fraction(what, x):
    if isinstance(x, Fraction):
        return x
    if isinstance(x, (tuple, list)):
        if len(x) != 2 or any(int(v) != v for v in x):
            raise ValueError(f"{what}: a rate pair is (numerator, denominator), two integers; got {x!r}")
        if int(x[1]) == 0:
            raise ValueError(f"{what}: denominator 0")
        return Fraction(int(x[0]), int(x[1]))
    if isinstance(x, (int, np.integer)):
        return Fraction(int(x))
    if isinstance(x, str):
        return decimal_to_fraction(x)
    x = float(x)
    if not np.isfinite(x):
        raise ValueError(f"{what}: {x}")
    return Fraction(x).limit_denominator(1000)


def parse_rate(rate=None, fps=None, target_fps=MODEL_FPS):
    """-> Fraction source frames per output frame.  rate: a Fraction, an (int, int) pair, an int, a float (through
    `limit_denominator(1000)`, see the module docstring) or a decimal string (`decimal_to_fraction`); or fps / target_fps, each read the
    same way.  24 fps -> 6/5, 1.25 -> 5/4."""
    what = "parse_rate"
    if (rate is None) == (fps is None):
        raise ValueError(f"{what}: give either rate or fps")
    r = _fraction(what, rate) if rate is not None else _fraction(what, fps) / _fraction(what, target_fps)
    if r <= 0:
        raise ValueError(f"{what}: rate {r} is not positive")
    if r.numerator > MAX_RATE or r.denominator > MAX_RATE:
        raise ValueError(f"{what}: rate {r}: numerator and denominator above {MAX_RATE} are not taken")
    return r


def up_down(rate):
    """The reference's lcm arithmetic for a rate num / den in lowest terms: up-sample by den, keep every num-th."""
    return rate.denominator, rate.numerator


def out_frames(frames, rate):
    """Output frames of a clip of `frames` source frames: ceil((frames - 1) * up / down); an int or an integer array."""
    up, down = up_down(rate)
    return np.maximum(-(-(np.asarray(frames, np.int64) - 1) * up // down), 0)


def max_frames(joints=CHAIN_JOINTS):
    """Longest source clip the kernels take (mst_track_max_frames)."""
    n = int(N.lib().mst_track_max_frames(int(joints)))
    if n < 0:
        N.check(1)
    return n


# ------------------------------------------------------------------------------------------ shared checks
def _host_lengths(what, lengths, B, T):
    """-> int64 numpy [B] or None, checked on the host: 2 <= len <= T (a clip of one frame has no interval)."""
    if lengths is None:
        return None
    host = lengths.detach().cpu().numpy() if torch.is_tensor(lengths) else np.asarray(lengths)
    host = host.reshape(-1).astype(np.int64)
    if host.shape[0] != B:
        raise ValueError(f"{what}: {host.shape[0]} lengths for {B} clips")
    if host.min() < 2 or host.max() > T:
        raise ValueError(f"{what}: lengths {host.min()}..{host.max()} outside 2..{T}")
    return host


def _f32(t, dev):
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


def _out_lengths(host, B, T, rate, dev):
    full = np.full(B, T, np.int64) if host is None else host
    return torch.from_numpy(out_frames(full, rate).astype(np.int32)).to(dev)


# ------------------------------------------------------------------------------------------ resampling
def resample_tracks(rotations=None, points=None, *, rate=None, fps=None, target_fps=MODEL_FPS, lengths=None, shortest=False):
    """Quaternion tracks [B, T, J, 4] (w first; need not be normalised) and point tracks [B, T, P, 3] (either may be None) resampled
    from `fps` to `target_fps`, or by `rate` source frames per output frame (`parse_rate`) -> (rotations [B, K, J, 4] or None, points
    [B, K, P, 3] or None, lengths int32 [B]) with K = ceil((T - 1) * up / down).  lengths [B]: a clip's own frames, 2 <= len <= T; a clip
    of L frames has ceil((L - 1) * up / down) output frames, every later row is exact zeros.
    Rotations follow the reference's `qslerp` in float32; shortest=True negates the relative quaternion of an interval when its w is
    negative, which makes the rotation independent of the sign of either end (the reference's formula takes the longer arc when the ends'
    signs disagree).  Points are p0 + t (p1 - p0) in double, stored as float32.  One launch on the caller's current stream; the inputs
    are not modified."""
    what = "resample_tracks"
    r = parse_rate(rate, fps, target_fps)
    if rotations is None and points is None:
        raise ValueError(f"{what}: neither rotations nor points")
    for name, t, last in (("rotations", rotations, 4), ("points", points, 3)):
        if t is None:
            continue
        if not torch.is_tensor(t):
            raise TypeError(f"{what}: {name} is a tensor")
        if t.dim() != 4 or t.shape[-1] != last or t.shape[2] < 1:
            raise ValueError(f"{what}: {name} of shape {tuple(t.shape)}, expected [B, T, {'J' if last == 4 else 'P'}, {last}]")
    first = rotations if rotations is not None else points
    B, T = first.shape[:2]
    if rotations is not None and points is not None and tuple(points.shape[:2]) != (B, T):
        raise ValueError(f"{what}: rotations of {B} clips x {T} frames but points of {tuple(points.shape[:2])}")
    if B < 1 or T < 2:
        raise ValueError(f"{what}: {B} clips of {T} frames; a track is resampled interval by interval, so 2 frames at least")
    host = _host_lengths(what, lengths, B, T)
    if any(t is not None and not t.is_cuda for t in (rotations, points)) or (torch.is_tensor(lengths) and not lengths.is_cuda):
        raise RuntimeError(_NO_CPU.format(what))
    J = 0 if rotations is None else rotations.shape[2]
    P = 0 if points is None else points.shape[2]
    limit = max_frames(max(J, P))
    if T > limit:
        raise RuntimeError(f"{what}: {T} frames > {limit}, the longest clip mst_track_resample takes (mst_track_max_frames)")
    dev = first.device
    up, down = up_down(r)
    K = int(out_frames(T, r))
    q = None if rotations is None else _f32(rotations, dev)
    p = None if points is None else _f32(points, dev)
    ld = None if host is None else torch.from_numpy(host.astype(np.int32)).to(dev)
    qo = None if q is None else torch.empty(B, K, J, 4, dtype=torch.float32, device=dev)
    po = None if p is None else torch.empty(B, K, P, 3, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        N.check(N.lib().mst_track_resample(N.ptr(q), N.ptr(p), N.ptr(ld), B, T, J, P, up, down, int(bool(shortest)), N.ptr(qo), N.ptr(po),
                                           N.stream_ptr(dev)))
    return qo, po, _out_lengths(host, B, T, r, dev)


# ------------------------------------------------------------------------------------------ the body's joint table
class BodyJoints:
    """What the video path needs of a body model: J = J0 + Jdirs beta for the first 22 joints and their parents.  J0 [22, 3] and Jdirs
    [22, 3, 10] are the joint regressor applied to the template and to the shape directions, formed in double as `SMPLBody` forms them.
    Only joints 0 .. 21 are kept and their parents all lie below 22, so an SMPL-H body of 52 joints and an SMPL body of 24 both serve.
    Built and validated on the host; the device copies are made on first use."""

    def __init__(self, v_template, shapedirs, J_regressor, parents, num_betas=NUM_BETAS):
        what = "BodyJoints"
        dense = lambda a: a.toarray() if hasattr(a, "toarray") else np.asarray(a)
        if not 1 <= int(num_betas) <= NUM_BETAS:
            raise ValueError(f"{what}: num_betas {num_betas} outside 1..{NUM_BETAS}")
        nb = int(num_betas)
        vt = np.ascontiguousarray(dense(v_template), dtype=np.float64)
        if vt.ndim != 2 or vt.shape[1] != 3 or vt.shape[0] < 1:
            raise ValueError(f"{what}: v_template of shape {vt.shape}, expected [V, 3]")
        V = vt.shape[0]
        sd = np.asarray(dense(shapedirs), dtype=np.float64)
        if sd.ndim != 3 or sd.shape[:2] != (V, 3) or sd.shape[2] < nb:
            raise ValueError(f"{what}: shapedirs of shape {sd.shape}, expected [{V}, 3, >= {nb}]")
        jr = np.asarray(dense(J_regressor), dtype=np.float64)
        if jr.ndim != 2 or jr.shape[1] != V or jr.shape[0] < CHAIN_JOINTS:
            raise ValueError(f"{what}: J_regressor of shape {jr.shape}, expected [>= {CHAIN_JOINTS}, {V}]")
        par = np.asarray(parents).astype(np.int64).reshape(-1)
        if par.shape[0] < CHAIN_JOINTS:
            raise ValueError(f"{what}: {par.shape[0]} parents, at least {CHAIN_JOINTS} are needed")
        par = par[:CHAIN_JOINTS].copy()
        if par[0] != -1:
            raise ValueError(f"{what}: parents[0] = {par[0]}, the root's is -1")
        for j in range(1, CHAIN_JOINTS):
            if not 0 <= par[j] < j:
                raise ValueError(f"{what}: parents[{j}] = {par[j]} is not an earlier joint")
        jr = jr[:CHAIN_JOINTS]
        for name, a in (("v_template", vt), ("shapedirs", sd), ("J_regressor", jr)):
            if not np.isfinite(a).all():
                raise ValueError(f"{what}: {name} is not finite")
        worst = float(np.abs(jr.sum(1) - 1).max())
        if not worst <= 1e-4:
            raise ValueError(f"{what}: a row of J_regressor sums to 1 {worst:+.3e}; every row must sum to 1 within 1e-4")
        self.num_betas = nb
        self.parents = par
        self.J0 = (jr @ vt).astype(np.float32)
        jd = np.zeros((CHAIN_JOINTS, 3, NUM_BETAS))
        jd[..., :nb] = np.einsum("jv,vci->jci", jr, sd[..., :nb])
        self.Jdirs = jd.astype(np.float32)
        self._dev = {}

    @classmethod
    def from_body(cls, body):
        """From an `SMPLBody` (model/smpl.py): its J0, Jdirs and parents, the first 22 joints."""
        self = cls.__new__(cls)
        self.num_betas = NUM_BETAS
        self.parents = np.asarray(body.parents).astype(np.int64)[:CHAIN_JOINTS].copy()
        self.J0 = np.ascontiguousarray(body.J0[:CHAIN_JOINTS], dtype=np.float32)
        self.Jdirs = np.ascontiguousarray(body.Jdirs[:CHAIN_JOINTS], dtype=np.float32)
        self._dev = {}
        return self

    @classmethod
    def from_npz(cls, path, num_betas=NUM_BETAS):
        """The user's own SMPL or SMPL-H .npz (the reference reads ./body_models/smplh/male/model.npz): `v_template`, `shapedirs` (the
        first `num_betas` directions), `J_regressor` and `kintree_table`."""
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in ("v_template", "shapedirs", "J_regressor", "kintree_table") if k not in z.files]
            if missing:
                raise KeyError(f"BodyJoints.from_npz: {missing} not in the file (keys: {sorted(z.files)[:20]})")
            parents = np.asarray(z["kintree_table"]).astype(np.int64)[0].copy()
            parents[0] = -1                               # the files store 2^32 - 1
            return cls(z["v_template"], z["shapedirs"], z["J_regressor"], parents, num_betas)

    def tables(self, device):
        """-> (J0, Jdirs) float32 tensors on `device`."""
        device = torch.device(device)
        if device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError(_NO_CPU.format("BodyJoints"))
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._dev:
            self._dev[device] = (torch.from_numpy(self.J0).to(device), torch.from_numpy(self.Jdirs).to(device))
        return self._dev[device]


# ------------------------------------------------------------------------------------------ tracks and their files
@dataclass
class PoseTrack:
    """One track of a pose estimator.  rotations [T, J, 4] (w first) or matrices [T, J, 3, 3] (exactly one of the two; J >= 22), transl
    [T, 3], betas [10] (the mean of the file's shape rows), joints [T, Je, 3] (the estimator's own joints; optional), fps (of the camera;
    None: not stated).  numpy arrays or tensors."""
    transl: object
    betas: object
    rotations: object = None
    matrices: object = None
    joints: object = None
    fps: Optional[float] = None

    @property
    def frames(self):
        return int((self.rotations if self.rotations is not None else self.matrices).shape[0])


def _np(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def read_pose_track(path, trans_path="", fps=None):
    """The files `amass_to_pose` reads, by the reference's suffix tests and key names -> PoseTrack:
      *pt   torch.load(path)[0]: `pred_theta_mats` (-> [T, 24, 3, 3]), `pred_shape`, `pred_xyz_jts_24_struct`, `transl`
      *pk   a pickle: `pred_thetas`, `pred_betas`, `pred_xyz_24_struct`, `transl`
      *pkl  pickle[0]: `smpl_pose_quat_wroot` ([T, J, 4] quaternions), `smpl_beta`, `root_trans`; no estimator joints
    betas is the mean of the shape rows.  trans_path: a pickle whose [0]['root_trans'] replaces the translation; track and translation are
    then cut to the shorter of the two, as in the reference.
    The files are unpickled as the reference unpickles them (`pickle.load`, `torch.load` without weights_only): unpickling runs code, so
    these are TRUSTED input -- open only files you made or trust."""
    path = str(path)
    rotations = matrices = joints = None
    if path[-2:] == "pt":
        d = torch.load(path, weights_only=False)[0]
        matrices = _np(d["pred_theta_mats"]).reshape(-1, 24, 3, 3)
        betas = _np(d["pred_shape"]).mean(0)
        joints = _np(d["pred_xyz_jts_24_struct"]).reshape(-1, 24, 3)
        transl = _np(d["transl"])
    elif path[-2:] == "pk":
        with open(path, "rb") as fh:
            d = pickle.load(fh)
        matrices = np.asarray(d["pred_thetas"]).reshape(-1, 24, 3, 3)
        betas = np.asarray(d["pred_betas"]).mean(0)
        joints = np.asarray(d["pred_xyz_24_struct"]).reshape(-1, 24, 3)
        transl = np.asarray(d["transl"])
    elif path[-3:] == "pkl":
        with open(path, "rb") as fh:
            d = pickle.load(fh)[0]
        rotations = np.asarray(d["smpl_pose_quat_wroot"])
        betas = np.asarray(d["smpl_beta"]).mean(0)
        transl = np.asarray(d["root_trans"])
    else:
        raise ValueError(f"read_pose_track: {path!r} ends in none of 'pt', 'pk', 'pkl'")
    rot = rotations if rotations is not None else matrices
    if trans_path:
        with open(trans_path, "rb") as fh:
            transl = np.asarray(pickle.load(fh)[0]["root_trans"])
        n = min(len(transl), len(rot))                    # the reference cuts by the joints' count, which is the rotations'
        transl, rot = transl[:n], rot[:n]
        joints = None if joints is None else joints[:n]
    transl = np.asarray(transl).reshape(-1, 3)
    if rotations is not None:
        return PoseTrack(transl, betas, rotations=rot, joints=joints, fps=fps)
    return PoseTrack(transl, betas, matrices=rot, joints=joints, fps=fps)


# ------------------------------------------------------------------------------------------ the fused video path
def track_joints_batch(rotations, transl, betas, body, *, rate, joints=None, with_trans=False, lengths=None, shortest=False):
    """The launch under `track_joints`, for tracks that already are one batch on the device.  rotations [B, T, J, 4] (w first) or
    [B, T, J, 3, 3] with J >= 22, transl [B, T, 3] (may be None without with_trans), betas [B, 10], joints [B, T, Je, 3] or None, rate
    a Fraction (`parse_rate`) -> (model joints [B, K, 22, 3], estimator joints [B, K, 22, 3] or None, lengths int32 [B])."""
    what = "track_joints"
    if not isinstance(body, BodyJoints):
        raise TypeError(f"{what}: body is a BodyJoints (BodyJoints.from_npz, .from_body); got {type(body).__name__}")
    if not isinstance(rate, Fraction):
        raise TypeError(f"{what}: rate is a Fraction (parse_rate)")
    for name, t in (("rotations", rotations), ("transl", transl), ("betas", betas), ("joints", joints)):
        if t is not None and not torch.is_tensor(t):
            raise TypeError(f"{what}: {name} is a tensor")
    is_mat = rotations.dim() == 5
    if not ((rotations.dim() == 4 and rotations.shape[-1] == 4) or (is_mat and tuple(rotations.shape[-2:]) == (3, 3))):
        raise ValueError(f"{what}: rotations of shape {tuple(rotations.shape)}, expected [B, T, J, 4] or [B, T, J, 3, 3]")
    B, T, Jr = rotations.shape[:3]
    if Jr < CHAIN_JOINTS:
        raise ValueError(f"{what}: {Jr} rotations a frame, the chain reads the first {CHAIN_JOINTS}")
    if B < 1 or T < 2:
        raise ValueError(f"{what}: {B} clips of {T} frames; a track is resampled interval by interval, so 2 frames at least")
    if transl is None and with_trans:
        raise ValueError(f"{what}: with_trans without a translation track")
    if transl is not None and tuple(transl.shape) != (B, T, 3):
        raise ValueError(f"{what}: transl of shape {tuple(transl.shape)}, expected [{B}, {T}, 3]")
    if tuple(betas.shape) != (B, NUM_BETAS):
        raise ValueError(f"{what}: betas of shape {tuple(betas.shape)}, expected [{B}, {NUM_BETAS}]")
    if joints is not None and (joints.dim() != 4 or tuple(joints.shape[:2]) != (B, T) or joints.shape[2] < CHAIN_JOINTS or joints.shape[3] != 3):
        raise ValueError(f"{what}: estimator joints of shape {tuple(joints.shape)}, expected [{B}, {T}, >= {CHAIN_JOINTS}, 3]")
    if rate <= 0 or rate.numerator > MAX_RATE or rate.denominator > MAX_RATE:
        raise ValueError(f"{what}: rate {rate}")
    host = _host_lengths(what, lengths, B, T)
    if any(t is not None and not t.is_cuda for t in (rotations, transl, betas, joints)) or (torch.is_tensor(lengths) and not lengths.is_cuda):
        raise RuntimeError(_NO_CPU.format(what))
    limit = max_frames(CHAIN_JOINTS)
    if T > limit:
        raise RuntimeError(f"{what}: {T} frames > {limit}, the longest clip mst_track_joints takes (mst_track_max_frames)")
    if B > 65535:
        raise ValueError(f"{what}: {B} clips > 65535 in one launch")
    dev = rotations.device
    up, down = up_down(rate)
    K = int(out_frames(T, rate))
    rot = _f32(rotations, dev)
    tr = None if transl is None else _f32(transl, dev)
    be = _f32(betas, dev)
    ej = None if joints is None else _f32(joints, dev)
    ld = None if host is None else torch.from_numpy(host.astype(np.int32)).to(dev)
    J0, Jd = body.tables(dev)
    out = torch.empty(B, K, CHAIN_JOINTS, 3, dtype=torch.float32, device=dev)
    eo = None if ej is None else torch.empty(B, K, CHAIN_JOINTS, 3, dtype=torch.float32, device=dev)
    parents = (C.c_int32 * CHAIN_JOINTS)(*[int(p) for p in body.parents])
    with torch.cuda.device(dev):
        N.check(N.lib().mst_track_joints(N.ptr(rot), int(is_mat), Jr, N.ptr(tr), N.ptr(be), N.ptr(ej), 0 if ej is None else ej.shape[2],
                                         N.ptr(ld), B, T, up, down, int(bool(shortest)), int(bool(with_trans)), N.ptr(J0), N.ptr(Jd),
                                         parents, N.ptr(out), N.ptr(eo), N.stream_ptr(dev)))
    return out, eo, _out_lengths(host, B, T, rate, dev)


def _collate(what, tracks, lengths, device):
    """PoseTracks -> padded device tensors (rotations, transl, betas, joints or None, lengths int64 numpy)."""
    if isinstance(tracks, PoseTrack):
        tracks = [tracks]
    tracks = list(tracks)
    if not tracks:
        raise ValueError(f"{what}: no tracks")
    for t in tracks:
        if not isinstance(t, PoseTrack):
            raise TypeError(f"{what}: tracks are PoseTrack objects (read_pose_track); got {type(t).__name__}")
        if (t.rotations is None) == (t.matrices is None):
            raise ValueError(f"{what}: a PoseTrack holds either rotations or matrices")
    is_mat = tracks[0].matrices is not None
    with_joints = tracks[0].joints is not None
    if any((t.matrices is not None) != is_mat or (t.joints is not None) != with_joints for t in tracks):
        raise ValueError(f"{what}: the tracks of a batch are all quaternions or all matrices, all with the estimator's joints or all without")
    rots = [np.asarray(_np(t.matrices if is_mat else t.rotations), np.float32) for t in tracks]
    tail = (3, 3) if is_mat else (4,)
    Jr = rots[0].shape[1] if rots[0].ndim >= 2 else 0
    for r in rots:
        if r.ndim != 2 + len(tail) or r.shape[2:] != tail or r.shape[1] != Jr or Jr < CHAIN_JOINTS:
            raise ValueError(f"{what}: a rotation track of shape {r.shape}, expected [T, {max(Jr, CHAIN_JOINTS)} (>= {CHAIN_JOINTS}), "
                             f"{', '.join(map(str, tail))}]")
    own = np.array([len(r) for r in rots], np.int64)
    if lengths is not None:
        given = np.asarray(_np(lengths)).reshape(-1).astype(np.int64)
        if given.shape[0] != len(tracks) or (given < 2).any() or (given > own).any():
            raise ValueError(f"{what}: lengths {given.tolist()} for tracks of {own.tolist()} frames (2 <= len <= the track's own)")
        own = given
    if own.min() < 2:
        raise ValueError(f"{what}: a track of {own.min()} frames; 2 at least")
    B, T = len(tracks), int(max(len(r) for r in rots))
    rot = np.zeros((B, T, Jr) + tail, np.float32)
    tr = np.zeros((B, T, 3), np.float32)
    be = np.zeros((B, NUM_BETAS), np.float32)
    ej, Je = None, 0
    if with_joints:
        Je = np.asarray(_np(tracks[0].joints)).shape[1]
        ej = np.zeros((B, T, Je, 3), np.float32)
    for b, t in enumerate(tracks):
        n = len(rots[b])
        rot[b, :n] = rots[b]
        x = np.asarray(_np(t.transl), np.float32).reshape(-1, 3)
        if len(x) < own[b]:
            raise ValueError(f"{what}: track {b}: {len(x)} translation rows for {own[b]} frames")
        m = min(len(x), n)
        tr[b, :m] = x[:m]
        s = np.asarray(_np(t.betas), np.float32).reshape(-1)
        if s.shape[0] < 1 or s.shape[0] > NUM_BETAS and np.any(s[NUM_BETAS:] != 0):
            raise ValueError(f"{what}: track {b}: {s.shape[0]} betas; the joint table takes {NUM_BETAS}")
        be[b, :min(len(s), NUM_BETAS)] = s[:NUM_BETAS]
        if with_joints:
            e = np.asarray(_np(t.joints), np.float32)
            if e.ndim != 3 or e.shape[1:] != (Je, 3) or Je < CHAIN_JOINTS or len(e) < own[b]:
                raise ValueError(f"{what}: track {b}: estimator joints of shape {e.shape}, expected [>= {own[b]}, {Je} (>= {CHAIN_JOINTS}), 3]")
            m = min(len(e), n)
            ej[b, :m] = e[:m]
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError(_NO_CPU.format(what))
    up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    return up(rot), up(tr), up(be), up(ej), own


def _track_fps(what, tracks, fps):
    if fps is not None:
        return fps
    stated = {t.fps for t in ([tracks] if isinstance(tracks, PoseTrack) else tracks) if getattr(t, "fps", None) is not None}
    if len(stated) > 1:
        raise ValueError(f"{what}: the tracks state different frame rates {sorted(stated)}; a launch has one rate")
    return stated.pop() if stated else 25


def track_joints(tracks, body, fps=None, with_trans=False, lengths=None, *, target_fps=MODEL_FPS, shortest=False, device="cuda"):
    """A PoseTrack or a list of them -> (model_joints [B, K, 22, 3], estimator_joints [B, K, 22, 3] or None, out_lengths int32 [B]) at
    `target_fps`, in one launch: what `amass_to_pose` returns per file.  fps: the camera's rate (None: the tracks' own `fps`, 25 -- the
    reference's default -- where they state none).  model_joints: the body's first 22 joints posed by the resampled rotations (plus the
    resampled translation under with_trans), x and z swapped and y negated.  estimator_joints: the tracks' own joints through the same
    lerp and re-axing, plus under with_trans the resampled translation re-axed the same way (the reference's `transl[:, [2, 1, 0]]`
    with y negated).  The tracks are padded to the longest; lengths [B]: fewer frames of a track than it holds.  Rows behind a clip's
    output length are exact zeros.  Matrix tracks always take the shorter arc; `shortest` offers it for quaternion tracks."""
    what = "track_joints"
    if not isinstance(body, BodyJoints):
        raise TypeError(f"{what}: body is a BodyJoints (BodyJoints.from_npz, .from_body); got {type(body).__name__}")
    rate = parse_rate(None, _track_fps(what, tracks, fps), target_fps)
    rot, tr, be, ej, own = _collate(what, tracks, lengths, device)
    return track_joints_batch(rot, tr, be, body, rate=rate, joints=ej, with_trans=with_trans, lengths=own, shortest=shortest)


def track_to_features(tracks, body, *, tgt_offsets, raw_offsets, chains=None, fps=None, with_trans=False, lengths=None,
                      source="model", l_idx=T2M_LEGS, face_joint_indx=T2M_FACE, fid_l=T2M_FID_L, fid_r=T2M_FID_R, feet_thre=0.002,
                      mean=None, std=None, frames_out=None, target_fps=MODEL_FPS, shortest=False, device="cuda"):
    """Tracks -> (sample [B, 263, 1, frames_out], lengths int32 [B]): `track_joints`, then `retarget_joints` onto the skeleton with bone
    offsets `tgt_offsets` [22, 3], then `encode_joints` in "hml" mode -- `pos2hmlrep` for a batch, normalised by mean / std [263] and
    zero-padded as the samplers read it, without leaving the device.  source: "model" (the body model's joints) or "estimator" (the
    tracks' own).  raw_offsets [22, 3]: HumanML3D's unit bone directions (the reference's t2m_raw_offsets); chains default to its
    kinematic chains.  Every clip needs at least 2 output frames."""
    from .motion_process import encode_joints, retarget_joints
    what = "track_to_features"
    if source not in ("model", "estimator"):
        raise ValueError(f"{what}: source {source!r} is neither 'model' nor 'estimator'")
    chains = T2M_CHAINS if chains is None else chains
    model, est, out_len = track_joints(tracks, body, fps, with_trans, lengths, target_fps=target_fps, shortest=shortest, device=device)
    if source == "estimator" and est is None:
        raise ValueError(f"{what}: source 'estimator' but the tracks hold no joints of the estimator")
    if int(out_len.min()) < 2:
        raise ValueError(f"{what}: a clip with {int(out_len.min())} output frames; encode_joints needs 2")
    joints = model if source == "model" else est
    if joints.shape[1] < 2:
        raise ValueError(f"{what}: {joints.shape[1]} output frames; encode_joints needs 2")
    moved = retarget_joints(joints, tgt_offsets, raw_offsets, chains, l_idx, face_joint_indx, lengths=out_len)
    return encode_joints(moved, chains=chains, raw_offsets=raw_offsets, face_joint_indx=face_joint_indx, fid_l=fid_l, fid_r=fid_r,
                         feet_thre=feet_thre, mode="hml", lengths=out_len, mean=mean, std=std, frames_out=frames_out)
