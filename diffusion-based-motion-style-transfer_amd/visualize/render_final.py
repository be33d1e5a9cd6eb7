"""The reference's visualize/render_final.py (`render`, :45-261) over the native chain: joints -> SMPLify (`joints2smpl`) ->
`Rotation2xyz(jointstype='vertices')` -> `render_meshes` (csrc/mst_mesh.h) -> PNGs and a GIF.  No `pyrender`, `trimesh`, `shapely`,
`imageio` or GL context: the frames are drawn on the device and written through PIL.

The reference loads ./body_models and the SMPLify prior files from fixed paths.  Here they are the user's: `configure(body=...,
pose_prior=..., mean_pose=..., mean_shape=...)` once, or the same keywords on `render`.  Everything else is the reference's: the
height offset subtracted from `motions` in place, the `<outdir><name>_pred.pt` / `_gt.pt` vertex cache, `joints2smpl` then
`Rotation2xyz(..., pose_rep='rot6d', translation=True, glob=True, jointstype='vertices', vertstrans=True)`, 960 x 960 RGBA frames,
every third frame as `<outdir><name>/<k>_pred.png` and `pred.gif` at 20 fps (pred=True), or `gt.gif` alone (pred=False).  What the
pictures look like inside the silhouette is this package's (visualize/mesh_render.py lists the deviations)."""
import os

import numpy as np
import torch

from ..model.rotation2xyz import Rotation2xyz
from . import mesh_render
from .simplify_loc2rot import joints2smpl

_CONFIG = {}


def configure(**kw):
    """Keep `body`, `pose_prior`, `mean_pose`, `mean_shape` (as `joints2smpl` takes them) and optionally `num_smplify_iters`, `width`,
    `height`, `samples` for later `render` calls.  configure() with nothing forgets them."""
    unknown = set(kw) - {"body", "pose_prior", "mean_pose", "mean_shape", "num_smplify_iters", "width", "height", "samples"}
    if unknown:
        raise TypeError(f"render_final.configure: unknown {sorted(unknown)}")
    if not kw:
        _CONFIG.clear()
    _CONFIG.update(kw)


class WeakPerspectiveCamera:
    """The reference's class (:21-43) without pyrender: `get_projection_matrix` is all this package reads."""

    def __init__(self, scale, translation, znear=0.05, zfar=None, name=None):
        self.scale, self.translation, self.znear, self.zfar, self.name = scale, translation, znear, zfar, name

    def get_projection_matrix(self, width=None, height=None):
        return mesh_render.weak_perspective_camera(self.scale, self.translation)


def render(motions, outdir='test_vis', device_id=0, name=None, pred=True, **kw):
    """motions [frames, njoints, 3] numpy (edited in place: y -= its minimum, as the reference) -> the files; returns the frames
    uint8 [T, 960, 960, 4] on the device.  kw overrides `configure`'s values."""
    cfg = dict(_CONFIG, **kw)
    if cfg.get("body") is None:
        raise RuntimeError("render_final.render: no SMPL body is configured; call render_final.configure(body=..., pose_prior=..., "
                           "mean_pose=..., mean_shape=...) or pass them here (no body model is bundled)")
    if not torch.cuda.is_available():
        raise RuntimeError("render_final.render runs on the GPU only (no CPU fallback)")
    frames, njoints, nfeats = motions.shape
    MINS = motions.min(axis=0).min(axis=0)
    height_offset = MINS[1]
    motions[:, :, 1] -= height_offset
    device = torch.device("cuda", device_id)
    rot2xyz = Rotation2xyz(device=device, body=cfg["body"])
    cache = outdir + name + ('_pred.pt' if pred else '_gt.pt')
    if not os.path.exists(cache):
        j2s = joints2smpl(num_frames=frames, device_id=device_id, cuda=True, num_smplify_iters=cfg.get("num_smplify_iters", 150),
                          body=cfg["body"], pose_prior=cfg.get("pose_prior"), mean_pose=cfg.get("mean_pose"), mean_shape=cfg.get("mean_shape"))
        motion_tensor, opt_dict = j2s.joint2smpl(motions)  # [nframes, njoints, 3]
        vertices = rot2xyz(motion_tensor.clone(), mask=None, pose_rep='rot6d', translation=True, glob=True, jointstype='vertices',
                           vertstrans=True)
        torch.save(vertices, cache)
    else:
        vertices = torch.load(cache, map_location=device)
        print(cache)
    out = mesh_render.render_meshes(vertices[:1], rot2xyz.smpl_model.body, width=cfg.get("width", 960), height=cfg.get("height", 960),
                                    samples=cfg.get("samples", 2))[0]
    os.makedirs(outdir + name, exist_ok=True)
    if pred:
        host = out.cpu().numpy()
        pil = mesh_render.ps._pil("render_final.render")
        if pil is None:
            raise RuntimeError("render_final.render: the PNGs and the GIF need PIL, which is not importable")
        for k in range(int(len(host) / 3)):
            pil.Image.fromarray(np.squeeze(host[k * 3])).save(outdir + name + '/' + str(k * 3) + '_pred.png')
        mesh_render.save_mesh_frames(outdir + name + '/' + 'pred.gif', host, fps=20)
    else:
        mesh_render.save_mesh_frames(outdir + name + '/' + 'gt.gif', out, fps=20)
    return out
