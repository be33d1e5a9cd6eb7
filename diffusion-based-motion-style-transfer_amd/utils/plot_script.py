"""Clips to video frames on the GPU: the counterpart of data_loaders/humanml/utils/plot_script.py (`plot_3d_motion`,
`explicit_plot_3d_motion`, :30-56 and :168-311).  The reference redraws a matplotlib 3-D axes per frame on one CPU thread and encodes
the animation; here a batch of clips becomes [B, T, H, W, 3] uint8 frames on the device in two launches (csrc/mst_render.h), without
matplotlib and without leaving the device.

  render_motion             joints -> frames (and the float image before quantisation when asked)
  frame_colors              the reference's per-frame palette names (`plot_3d_motion`, :37-55), a pure host function
  plot_3d_motion,           the reference's signatures: a numpy [T, J, 3] clip or a CUDA batch -> frames, saved when a path is given
  explicit_plot_3d_motion
  default_camera            matplotlib's projection for the reference's axes as a closed form: no matplotlib is imported
  title_overlay             the wrapped title as a coverage mask for `overlay=` (PIL's built-in font; None without PIL)
  save_frames               .npy, .gif / .png through PIL, .mp4 through an `ffmpeg` on PATH

The scene is the reference's: scale * joints, the floor at the clip's lowest point, everything re-centred on the root frame by frame,
the ground quad over the clip's extent, the first five kinematic chains (the reference's `zip` with a five-colour palette stops there,
so chains beyond the fifth were never drawn and are not drawn here), the root or joint traces the inpainting mask names.  The drawing
rules -- analytic coverage of quads and polylines, straight-alpha compositing -- are this package's and are stated in
include/mst_engine.h; matplotlib's Agg anti-aliasing is not matched pixel for pixel, its geometry is.

Stated deviations from the reference:
  * the camera distance.  The reference sets `ax.dist = 7.5`, which a current matplotlib no longer reads (its distance is 10): the
    default here is what a current matplotlib draws, `dist=7.5` is offered.
  * a non-square image uses the square image's map for min(W, H), centred.  matplotlib has no say here: the reference's figure is square.
  * `scale` multiplies both skeletons (the reference scales `joints2` for HumanML-like datasets only).
  * a trace names a joint by index, or by name through the `names=` list the caller passes (the reference's own table of HumanML3D
    joint names is not carried here).  `render_motion` refuses a feature that is neither; `plot_3d_motion` and
    `explicit_plot_3d_motion` pass over it, as the reference does with the mask names the demo hands it ('upper_body', '').
  * vis_mode 'upper_body'.  The reference's `colors = colors_orange; colors[0] = colors_blue[0]; colors[1] = colors_blue[1]` writes
    through to the 'orange' entry of its palette table, so its 'orange' frames are drawn in blue for the first two chains: the
    'upper_body' palette.  `explicit_plot_3d_motion` does the same; `frame_colors` returns the names the reference passes down.

Nothing here has a CPU path; `frame_colors`, `default_camera`, `title_overlay`, `save_frames` and every argument check need no GPU."""
import ctypes as C
import math
import os
import shutil
import subprocess
import warnings
from textwrap import wrap

import numpy as np
import torch

from .. import _native as N

_NO_CPU = "{} runs on the GPU only (no CPU fallback); move the joints to cuda"
PALETTE_NAMES = ("blue", "orange", "purple", "upper_body")
TRACE_ROOT_HORIZONTAL, TRACE_ROOT, TRACE_JOINT = 0, 1, 2
# the reference's per-dataset scale (:203-214); the second 'humanact12' / 'uestc' test there is never reached
DATASET_SCALE = {"kit": 0.003, "humanml": 1.3, "bandai-1_posrot": 1.3, "bandai-2_posrot": 1.3, "humanact12": -1.5, "uestc": -1.5,
                 "amass": -1.5, "babel": -1.3}
# matplotlib's constants: the 4:4:3 box aspect's normalisation (Axes3D.set_box_aspect) and the 2-D view limits of a 3-D axes
_BOX_NORM = 1.8294640721620434 * 25 / 24
_VIEW_MIN, _VIEW_MAX = -0.095, 0.09


class FfmpegNotFound(RuntimeError):
    """save_frames('.mp4') found no `ffmpeg` on PATH."""


# ------------------------------------------------------------------------------------------ the camera
def default_camera(width, height, radius=3.0, dist=10.0, elev=120.0, azim=-90.0, focal_length=1.0):
    """-> (proj [4, 4], affine [2, 3]) float64: what a current matplotlib's `Axes3D.get_proj()` and `transData` give for the
    reference's axes -- limits [-r/2, r/2], [0, r], [-r/3, 2r/3] scaled to the 4:4:3 box aspect, `view_init(elev, azim)`, roll 0,
    z vertical, perspective of the given focal length from distance `dist` -- filling a square figure of `width` pixels.  A pixel is
    affine (X / w, Y / w, 1) with (X, Y, ., w) = proj (x, y, z, 1), y up.  For width != height the square map of min(width, height)
    is centred in the image (this package's definition)."""
    r = float(radius)
    if not (r > 0 and dist > 0 and focal_length > 0 and math.isfinite(r * dist * focal_length)):
        raise ValueError("default_camera: radius, dist and focal_length are positive and finite")
    box = np.array([4.0, 4.0, 3.0])
    box = box * (_BOX_NORM / np.linalg.norm(box))
    lo = np.array([-r / 2, 0.0, -r / 3.0])
    span = np.array([r, r, r]) / box
    world = np.eye(4)
    world[[0, 1, 2], [0, 1, 2]] = 1.0 / span
    world[:3, 3] = -lo / span
    e, a = np.deg2rad(elev), np.deg2rad(azim)
    ps = np.array([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)])
    centre = 0.5 * box
    eye = centre + dist * ps * focal_length
    en = (elev + 180.0) % 360.0 - 180.0                               # art3d._norm_angle
    up = np.array([0.0, 0.0, -1.0 if abs(np.deg2rad(en)) > np.pi / 2 else 1.0])
    w = eye - centre
    w = w / np.linalg.norm(w)
    u = np.cross(up, w)
    u = u / np.linalg.norm(u)
    v = np.cross(w, u)
    view = np.eye(4)
    view[:3, :3] = [u, v, w]
    shift = np.eye(4)
    shift[:3, 3] = -eye
    persp = np.array([[focal_length, 0, 0, 0], [0, focal_length, 0, 0], [0, 0, 0.0, -dist], [0, 0, -1.0, 0]])
    proj = persp @ (view @ shift) @ world
    side = float(min(width, height))
    k = side / (_VIEW_MAX - _VIEW_MIN)
    affine = np.array([[k, 0.0, -_VIEW_MIN * k + (width - side) / 2.0], [0.0, k, -_VIEW_MIN * k + (height - side) / 2.0]])
    return proj, affine


# ------------------------------------------------------------------------------------------ frame colours
def frame_colors(frames_number, vis_mode="default", gt_frames=(), handshake_size=0, blend_size=0, step_sizes=(), lengths=()):
    """The palette name of every frame as the reference's `plot_3d_motion` forms it (:37-55): 'blue' for a frame in gt_frames and
    'orange' otherwise; 'unfold' and 'unfold_arb_len' lay out the purple hand-shakes of the long-sequence sampler ('unfold' returns
    its own count of names, longer than the clip, as the reference's does); 'gt' is all blue.  Frames behind the list are blue
    (`explicit_plot_3d_motion`, :267)."""
    gt = set(int(g) for g in gt_frames)
    colors = ["blue" if index in gt else "orange" for index in range(frames_number)]
    if vis_mode == "unfold":
        colors = ["purple"] * handshake_size + ["blue"] * blend_size + ["orange"] * (120 - handshake_size * 2 - blend_size * 2) + \
                 ["orange"] * blend_size
        colors = ["orange"] * (120 - handshake_size - blend_size) + ["orange"] * blend_size + colors * 1024
    elif vis_mode == "unfold_arb_len":
        for ii, step_size in enumerate(step_sizes):
            if ii == 0:
                colors = ["orange"] * (step_size - handshake_size - blend_size) + ["orange"] * blend_size + ["purple"] * (handshake_size // 2)
                continue
            if ii == len(step_sizes) - 1:
                colors += ["purple"] * (handshake_size // 2) + ["orange"] * blend_size + ["orange"] * (lengths[ii] - handshake_size - blend_size)
                continue
            colors += ["purple"] * (handshake_size // 2) + ["orange"] * blend_size + \
                      ["orange"] * (lengths[ii] - 2 * handshake_size - 2 * blend_size) + ["orange"] * blend_size + \
                      ["purple"] * (handshake_size // 2)
    elif vis_mode == "gt":
        colors = ["blue"] * frames_number
    return colors


def palette_indices(colors, frames_number, upper_body=False):
    """Names (or indices) per frame -> int32 [frames_number]: frames behind the list are blue; under `upper_body` an 'orange' frame
    reads the 'upper_body' palette (see the module docstring)."""
    out = np.zeros(frames_number, np.int32)
    for i in range(frames_number):
        if i < len(colors):
            c = colors[i]
            if isinstance(c, str):
                if c not in PALETTE_NAMES:
                    raise ValueError(f"palette: {c!r} is none of {PALETTE_NAMES}")
                c = PALETTE_NAMES.index(c)
            c = int(c)
            if not 0 <= c < len(PALETTE_NAMES):
                raise ValueError(f"palette: index {c} outside 0..{len(PALETTE_NAMES) - 1}")
            out[i] = 3 if (upper_body and c == 1) else c
    return out


# ------------------------------------------------------------------------------------------ rendering
def limits():
    """-> dict of the kernel's limits (mst_render_max_*): frames, joints, chains_drawn, traces, side, chunk."""
    lib = N.lib()
    return {"frames": lib.mst_render_max_frames(), "joints": lib.mst_render_max_joints(), "chains_drawn": lib.mst_render_chains_drawn(),
            "traces": lib.mst_render_max_traces(), "side": lib.mst_render_max_side(), "chunk": lib.mst_render_chunk()}


def _traces(what, painting_features, names, J):
    """The reference's order (:295-300): root_horizontal, root, then every named joint in the order given."""
    if isinstance(painting_features, str):
        painting_features = [painting_features]
    feats = [f for f in painting_features if not (isinstance(f, str) and f == "")]
    kinds, joints = [], []
    if "root_horizontal" in feats:
        kinds.append(TRACE_ROOT_HORIZONTAL)
        joints.append(0)
    if "root" in feats:
        kinds.append(TRACE_ROOT)
        joints.append(0)
    for f in feats:
        if isinstance(f, str) and f in ("root_horizontal", "root"):
            continue
        if isinstance(f, str):
            if names is None or f not in list(names):
                raise ValueError(f"{what}: trace {f!r} is neither 'root_horizontal', 'root', a joint index nor a name in names=")
            j = list(names).index(f)
        else:
            j = int(f)
        if not 0 <= j < J:
            raise ValueError(f"{what}: trace joint {j} outside 0..{J - 1}")
        kinds.append(TRACE_JOINT)
        joints.append(j)
    return kinds, joints


def _palette(what, palette, B, T):
    """None, a name, an index, a list of names per frame, or an integer array [T] or [B, T] -> int32 numpy [B, T]."""
    if palette is None:
        palette = "orange"
    if isinstance(palette, (str, int, np.integer)):
        return np.ascontiguousarray(np.broadcast_to(palette_indices([palette], 1)[0], (B, T)), dtype=np.int32)
    if torch.is_tensor(palette):
        palette = palette.detach().cpu().numpy()
    if isinstance(palette, (list, tuple)) and all(isinstance(c, str) for c in palette):
        return np.ascontiguousarray(np.broadcast_to(palette_indices(palette, T), (B, T)), dtype=np.int32)
    arr = np.asarray(palette)
    if arr.dtype.kind not in "iu" or arr.shape not in ((T,), (B, T)):
        raise ValueError(f"{what}: palette of shape {arr.shape} and type {arr.dtype}, expected integers [{T}] or [{B}, {T}]")
    if arr.size and (arr.min() < 0 or arr.max() >= len(PALETTE_NAMES)):
        raise ValueError(f"{what}: palette indices outside 0..{len(PALETTE_NAMES) - 1}")
    return np.ascontiguousarray(np.broadcast_to(arr, (B, T)), dtype=np.int32)            # a broadcast view keeps stride 0 through astype


def render_motion(joints, kinematic_tree, lengths=None, *, joints2=None, palette=None, painting_features=(), scale=1.3, radius=3,
                  size=300, dpi=100, camera=None, overlay=None, frames=None, float_image=False, layout="btjc", names=None, dist=10.0):
    """joints [B, T, J, 3] (layout='btjc') or [B, J, 3, T] (layout='bjct', as `recover_joints` lays it out; the layout is never
    guessed) on a CUDA device -> frames uint8 [B, t1 - t0, H, W, 3] on the same device, plus the float32 image before quantisation
    when float_image=True.  Two launches on the caller's current stream; the inputs are read in place through their strides.

    kinematic_tree: lists of joint indices; the first five are drawn.  lengths [B]: a clip's own frames, 1 <= len <= T; frames at and
    behind it are exact zeros.  joints2: a second skeleton of the same shape, drawn in the same colours and shifted by the first
    one's root.  palette: a name or index for every frame, a list of names per frame (`frame_colors`), or integers [T] / [B, T];
    default 'orange'.  painting_features: 'root_horizontal', 'root', joint indices, or joint names resolved through `names=`.
    size: the image side, or (H, W); each 16..1024.  dpi sets the line widths (4 pt and 2 pt).  camera: (proj [4, 4], affine [2, 3])
    instead of `default_camera(W, H, radius, dist)`.  overlay: uint8 [H, W], [1, H, W] or [B, H, W] coverage drawn last in black
    (`title_overlay`).  frames=(t0, t1) renders only those frames, bit-equal to the same frames of a full render."""
    what = "render_motion"
    if not torch.is_tensor(joints):
        raise TypeError(f"{what}: joints is a tensor")
    if layout not in ("btjc", "bjct"):
        raise ValueError(f"{what}: layout {layout!r} is neither 'btjc' ([B, T, J, 3]) nor 'bjct' ([B, J, 3, T])")
    axis = 3 if layout == "btjc" else 2
    if joints.dim() != 4 or joints.shape[axis] != 3:
        raise ValueError(f"{what}: joints of shape {tuple(joints.shape)}, expected {'[B, T, J, 3]' if layout == 'btjc' else '[B, J, 3, T]'}")
    B, T, J = (joints.shape[0], joints.shape[1], joints.shape[2]) if layout == "btjc" else (joints.shape[0], joints.shape[3], joints.shape[1])
    if B < 1 or T < 1 or J < 1:
        raise ValueError(f"{what}: {B} clips of {T} frames and {J} joints")
    if joints2 is not None and (not torch.is_tensor(joints2) or tuple(joints2.shape) != tuple(joints.shape)):
        raise ValueError(f"{what}: joints2 is a tensor of the shape of joints, {tuple(joints.shape)}")
    H, W = (int(size), int(size)) if isinstance(size, (int, np.integer)) else (int(size[0]), int(size[1]))
    if not (16 <= H <= 1024 and 16 <= W <= 1024):
        raise ValueError(f"{what}: image {H} x {W}: each side 16..1024")
    if not (math.isfinite(dpi) and dpi > 0) or not math.isfinite(scale):
        raise ValueError(f"{what}: dpi {dpi} must be positive and scale {scale} finite")
    chains = [[int(j) for j in c] for c in kinematic_tree]
    if len(chains) > 16:
        raise ValueError(f"{what}: {len(chains)} chains, at most 16 are taken")
    for c in chains:
        if any(not 0 <= j < J for j in c):
            raise ValueError(f"{what}: chain {c} names a joint outside 0..{J - 1}")
    if sum(len(c) for c in chains[:5]) > 128:
        raise ValueError(f"{what}: the five chains drawn hold more than 128 points")
    kinds, tjoints = _traces(what, painting_features, names, J)
    if len(kinds) > 8:
        raise ValueError(f"{what}: {len(kinds)} traces, at most 8")
    t0, t1 = (0, T) if frames is None else (int(frames[0]), int(frames[1]))
    if not 0 <= t0 < t1 <= T:
        raise ValueError(f"{what}: frames ({t0}, {t1}) is not 0 <= t0 < t1 <= {T}")
    host_len = None
    if lengths is not None:
        host_len = (lengths.detach().cpu().numpy() if torch.is_tensor(lengths) else np.asarray(lengths)).reshape(-1).astype(np.int64)
        if host_len.shape[0] != B or host_len.min() < 1 or host_len.max() > T:
            raise ValueError(f"{what}: lengths {host_len.tolist()[:8]} for {B} clips of {T} frames (1 <= len <= T)")
    pal = _palette(what, palette, B, T)
    if camera is None:
        proj, affine = default_camera(W, H, radius, dist)
    else:
        proj, affine = (np.asarray(camera[0], np.float64), np.asarray(camera[1], np.float64))
        if proj.shape != (4, 4) or affine.shape != (2, 3):
            raise ValueError(f"{what}: camera is (proj [4, 4], affine [2, 3]); got {proj.shape} and {affine.shape}")
    if overlay is not None:
        if not torch.is_tensor(overlay):
            overlay = torch.from_numpy(np.ascontiguousarray(overlay))
        if overlay.dim() == 2:
            overlay = overlay[None]
        if overlay.dtype != torch.uint8 or overlay.dim() != 3 or tuple(overlay.shape[1:]) != (H, W) or overlay.shape[0] not in (1, B):
            raise ValueError(f"{what}: overlay of shape {tuple(overlay.shape)} and type {overlay.dtype}, expected uint8 [1 or {B}, {H}, {W}]")
    if not joints.is_cuda or (joints2 is not None and not joints2.is_cuda):
        raise RuntimeError(_NO_CPU.format(what))
    lim = limits()
    if T > lim["frames"] or J > lim["joints"]:
        raise RuntimeError(f"{what}: {T} frames and {J} joints; the kernel takes {lim['frames']} and {lim['joints']}")
    dev = joints.device
    src = joints.detach()
    if src.dtype != torch.float32:
        src = src.float()
    src2 = None
    if joints2 is not None:
        src2 = joints2.detach().to(device=dev, dtype=torch.float32)
        if src2.stride() != src.stride():
            src, src2 = src.contiguous(), src2.contiguous()
    if any(s < 1 for s in src.stride()):
        src = src.contiguous()
        src2 = None if src2 is None else src2.contiguous()
    st = src.stride()
    sB, sT, sJ, sC = (st[0], st[1], st[2], st[3]) if layout == "btjc" else (st[0], st[3], st[1], st[2])
    ld = None if host_len is None else torch.from_numpy(host_len.astype(np.int32)).to(dev)
    pal_dev = torch.from_numpy(np.array(pal, dtype=np.int32, order="C")).to(dev)     # a copy: [B][T] rows, never a broadcast view
    ov = None if overlay is None else overlay.to(dev).contiguous()
    scene = N.MstRenderScene(src.data_ptr(), None if src2 is None else src2.data_ptr(), sB, sT, sJ, sC, None if ld is None else ld.data_ptr(),
                             B, T, J, float(scale))
    view = N.MstRenderView()
    offs = np.concatenate([[0], np.cumsum([len(c) for c in chains])]).astype(np.int32)
    flat = np.array([j for c in chains for j in c] or [0], np.int32)
    c_offs, c_flat = (C.c_int32 * len(offs))(*offs.tolist()), (C.c_int32 * len(flat))(*flat.tolist())
    c_kinds, c_tj = (C.c_int32 * max(len(kinds), 1))(*kinds), (C.c_int32 * max(len(kinds), 1))(*tjoints)
    view.n_chains, view.chain_offsets_host, view.chain_joints_host = len(chains), c_offs, c_flat
    view.n_traces, view.trace_kinds_host, view.trace_joints_host = len(kinds), c_kinds, c_tj
    view.palette_dev = pal_dev.data_ptr()
    view.proj = (C.c_float * 16)(*[float(x) for x in proj.reshape(-1)])
    view.affine = (C.c_float * 6)(*[float(x) for x in affine.reshape(-1)])
    view.width, view.height, view.dpi = W, H, float(dpi)
    view.overlay_dev, view.overlay_batch = (None, 0) if ov is None else (ov.data_ptr(), ov.shape[0])
    view.t0, view.t1 = t0, t1
    bounds = torch.empty(B, 8, dtype=torch.float32, device=dev)
    out = torch.empty(B, t1 - t0, H, W, 3, dtype=torch.uint8, device=dev)
    outf = torch.empty(B, t1 - t0, H, W, 3, dtype=torch.float32, device=dev) if float_image else None
    with torch.cuda.device(dev):
        stream = N.stream_ptr(dev)
        N.check(N.lib().mst_render_bounds(C.byref(scene), N.ptr(bounds), stream))
        N.check(N.lib().mst_render_frames(C.byref(scene), N.ptr(bounds), C.byref(view), N.ptr(out), N.ptr(outf), stream))
    return (out, outf) if float_image else out


# ------------------------------------------------------------------------------------------ the reference's entry points
def explicit_plot_3d_motion(save_path, kinematic_tree, joints, title, dataset, figsize=(3, 3), fps=120, radius=3, vis_mode="default",
                            frame_colors=(), joints2=None, painting_features=(), *, dpi=100, names=None, lengths=None, device="cuda"):
    """The reference's signature (:168).  joints: a numpy [T, J, 3] (or [T, J * 3]) clip, moved to `device`, or a CUDA batch
    [B, T, J, 3].  -> uint8 frames [T, H, W, 3] (a clip) or [B, T, H, W, 3] (a batch) on the device, H = figsize[1] * dpi and
    W = figsize[0] * dpi; written through `save_frames(save_path, frames, fps)` when save_path is given (a batch: one file per clip,
    '_<b>' before the extension).  title: a string, wrapped at 20 characters and drawn through `title_overlay`; a list of per-frame
    titles draws its first.  dataset picks the scale (DATASET_SCALE)."""
    what = "explicit_plot_3d_motion"
    if dataset not in DATASET_SCALE:
        raise ValueError(f"{what}: dataset {dataset!r} is none of {sorted(DATASET_SCALE)}")
    single = not torch.is_tensor(joints)

    def to_batch(a):
        if a is None:
            return None
        if torch.is_tensor(a):
            return a
        a = np.asarray(a, np.float32)
        return torch.from_numpy(np.ascontiguousarray(a.reshape(len(a), -1, 3)))[None].to(device)

    if single and not torch.cuda.is_available():
        raise RuntimeError(_NO_CPU.format(what))
    batch, batch2 = to_batch(joints), to_batch(joints2)
    T = batch.shape[1]
    W, H = int(round(figsize[0] * dpi)), int(round(figsize[1] * dpi))
    if isinstance(title, (list, tuple)):
        title = title[0] if len(title) else ""
    overlay = title_overlay(title, H, W) if title else None
    pal = palette_indices(list(frame_colors), T, upper_body=vis_mode == "upper_body")
    # the demo hands over its whole inpainting mask, split at commas ('upper_body', ''): what names no trace is passed over, as the
    # reference's `plot_feature` passes over what is not in its joint names
    if isinstance(painting_features, str):
        painting_features = [painting_features]
    feats = [f for f in painting_features if not isinstance(f, str) or f in ("root_horizontal", "root") or (names is not None and f in names)]
    frames = render_motion(batch, kinematic_tree, lengths, joints2=batch2, palette=pal, painting_features=feats,
                           scale=DATASET_SCALE[dataset], radius=radius, size=(H, W), dpi=dpi, overlay=overlay, names=names)
    if save_path:
        if single:
            save_frames(save_path, frames[0], fps)
        else:
            stem, ext = os.path.splitext(str(save_path))
            for b in range(frames.shape[0]):
                save_frames(f"{stem}_{b}{ext}", frames[b] if lengths is None else frames[b, :int(lengths[b])], fps)
    return frames[0] if single else frames


def plot_3d_motion(save_path, kinematic_tree, joints, title, dataset, figsize=(3, 3), fps=120, radius=3, vis_mode="default", gt_frames=(),
                   handshake_size=0, blend_size=0, step_sizes=(), lengths=(), joints2=None, painting_features=(), **kw):
    """The reference's signature (:30): `frame_colors` from gt_frames and vis_mode, then `explicit_plot_3d_motion`.  `lengths` is the
    reference's argument of that name (the windows of 'unfold_arb_len'), not the clips' lengths, which go through `clip_lengths=`."""
    frames_number = joints.shape[1] if torch.is_tensor(joints) else len(joints)
    colors = frame_colors(frames_number, vis_mode, gt_frames, handshake_size, blend_size, step_sizes, lengths)
    return explicit_plot_3d_motion(save_path, kinematic_tree, joints, title, dataset, figsize=figsize, fps=fps, radius=radius,
                                   vis_mode=vis_mode, frame_colors=colors, joints2=joints2, painting_features=painting_features,
                                   lengths=kw.pop("clip_lengths", None), **kw)


# ------------------------------------------------------------------------------------------ titles and files
_warned = set()


def _pil(what):
    try:
        import PIL.Image  # noqa: F401
        import PIL.ImageDraw  # noqa: F401
        import PIL.ImageFont  # noqa: F401
        return PIL
    except ImportError:
        if what not in _warned:
            _warned.add(what)
            warnings.warn(f"{what}: PIL is not importable")
        return None


def title_overlay(text, height, width):
    """The title wrapped at 20 characters as the reference wraps it (:174-177), drawn centred at the top in PIL's built-in font -> a
    uint8 [height, width] coverage mask for `overlay=`, confined to the top fifth of the image; None (with one warning) where PIL
    is not importable.  There is no font table in the kernel."""
    pil = _pil("title_overlay")
    if pil is None:
        return None
    lines = wrap(str(text), 20)
    strip = max(height // 5, 1)
    img = pil.Image.new("L", (width, strip), 0)
    draw = pil.ImageDraw.Draw(img)
    font = pil.ImageFont.load_default()
    y = 1
    for line in lines:
        x0, y0, x1, y1 = draw.textbbox((0, 0), line, font=font)
        if y + (y1 - y0) > strip:
            break
        draw.text(((width - (x1 - x0)) // 2 - x0, y - y0), line, fill=255, font=font)
        y += (y1 - y0) + 2
    mask = np.zeros((height, width), np.uint8)
    mask[:strip] = np.asarray(img, np.uint8)
    return mask


def _host_chunks(frames, chunk):
    """Frames to the host a chunk at a time: a device tensor is never copied whole."""
    for s in range(0, frames.shape[0], chunk):
        part = frames[s:s + chunk]
        yield part.detach().cpu().numpy() if torch.is_tensor(part) else np.asarray(part)


def render_to_file(path, joints, kinematic_tree, fps=20, chunk=32, **kw):
    """One clip ([1, T, J, 3], or [1, J, 3, T] with layout='bjct') rendered `chunk` frames at a time through `frames=` and handed to
    `save_frames` piece by piece: a 4096-frame clip never has its whole video resident on the device.  kw: `render_motion`'s."""
    if not torch.is_tensor(joints) or joints.dim() != 4 or joints.shape[0] != 1:
        raise ValueError("render_to_file: joints is one clip, a tensor [1, T, J, 3] or [1, J, 3, T]")
    if "frames" in kw or kw.get("float_image"):
        raise ValueError("render_to_file: frames= and float_image= are not taken")
    T = joints.shape[3] if kw.get("layout", "btjc") == "bjct" else joints.shape[1]
    if kw.get("lengths") is not None:
        T = int(np.asarray(kw["lengths"].cpu() if torch.is_tensor(kw["lengths"]) else kw["lengths"]).reshape(-1)[0])
    pieces = (render_motion(joints, kinematic_tree, frames=(s, min(s + chunk, T)), **kw)[0] for s in range(0, T, chunk))
    return save_frames(path, pieces, fps, chunk)


def save_frames(path, frames, fps=20, chunk=32):
    """frames uint8 [T, H, W, 3] (a tensor on any device, or numpy; [T, H, W, 4] RGBA too: .npy and .png keep the alpha channel,
    .gif and .mp4 drop it and write the colours as they are) -> a file chosen by the extension: .npy (always), .gif and .png
    (numbered files path_0000.png ...) through PIL, .mp4 as raw RGB piped to an `ffmpeg` found on PATH (FfmpegNotFound when there is
    none; nothing is bundled or fetched).  Frames come to the host `chunk` at a time.  To keep a long clip's video off the device
    altogether, render it through `render_motion(..., frames=(t0, t1))` and pass a generator of such pieces as `frames`."""
    what = "save_frames"
    path = str(path)
    ext = os.path.splitext(path)[1].lower()
    if ext not in (".npy", ".gif", ".png", ".mp4"):
        raise ValueError(f"{what}: {ext!r} is none of .npy, .gif, .png, .mp4")
    pieces = [frames] if (torch.is_tensor(frames) or isinstance(frames, np.ndarray)) else frames

    def host():
        for piece in pieces:
            if piece.ndim != 4 or piece.shape[-1] not in (3, 4) or (piece.dtype not in (torch.uint8, np.uint8)):
                raise ValueError(f"{what}: frames of shape {tuple(piece.shape)} and type {piece.dtype}, expected uint8 [T, H, W, 3 or 4]")
            for part in _host_chunks(piece, chunk):
                yield part[..., :3] if (part.shape[-1] == 4 and ext in (".gif", ".mp4")) else part

    if ext == ".npy":
        np.save(path, np.concatenate(list(host())))
        return path
    if ext == ".mp4":
        exe = shutil.which("ffmpeg")
        if exe is None:
            raise FfmpegNotFound(f"{what}: no `ffmpeg` on PATH to encode {path!r}; save .npy, .gif or .png instead, or install ffmpeg")
        proc = None
        for part in host():
            if proc is None:
                h, w = part.shape[1:3]
                proc = subprocess.Popen([exe, "-y", "-loglevel", "error", "-f", "rawvideo", "-pix_fmt", "rgb24", "-s", f"{w}x{h}", "-r",
                                         str(fps), "-i", "-", "-an", "-pix_fmt", "yuv420p", path], stdin=subprocess.PIPE)
            proc.stdin.write(np.ascontiguousarray(part).tobytes())
        if proc is not None:
            proc.stdin.close()
            if proc.wait() != 0:
                raise RuntimeError(f"{what}: ffmpeg exited with {proc.returncode}")
        return path
    pil = _pil(what)
    if pil is None:
        raise RuntimeError(f"{what}: {ext} needs PIL, which is not importable; .npy always works")
    images = [pil.Image.fromarray(f) for part in host() for f in part]
    if ext == ".gif":
        images[0].save(path, save_all=True, append_images=images[1:], duration=max(int(round(1000 / fps)), 1), loop=0)
    else:
        stem = os.path.splitext(path)[0]
        for i, im in enumerate(images):
            im.save(f"{stem}_{i:04d}.png")
    return path
