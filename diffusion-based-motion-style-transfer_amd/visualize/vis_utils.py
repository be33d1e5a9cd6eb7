"""The mesh output of the demo chain: the reference's visualize/vis_utils.py `npy2obj` (:10-70) over the native SMPL body.  A
`results.npy` of SMPL parameters (`nfeats == 6`: 24 6D rotations and one translation row per frame) becomes vertices in one chain of
launches (model/rotation2xyz.py) and OBJ / npy files.  `nfeats == 3` (joint positions) goes through SMPLify first, the reference's
`joints2smpl` fit (visualize/simplify_loc2rot.py), when the caller hands one over as `smplify=`: the fit needs the user's prior and
mean-parameter files, which nothing here can find on its own.  `joints2rotation` is the reference's helper of the same name;
`joints2bvh` is not covered.  OBJ files are written by this module's own writer, plain `v x y z` / `f a b c` lines with
1-based indices; `trimesh` is not used, and byte equality with its exporter is not claimed."""
import numpy as np
import torch

from ..model.rotation2xyz import Rotation2xyz
from ..model.smpl import _NO_CPU


def write_obj(path_or_file, vertices, faces):
    """vertices [V, 3] floats, faces [F, 3] 0-based ints -> `v` and `f` lines (1-based).  %.9g: nine significant digits, so a
    float32 vertex is read back (`read_obj`) as the same float32."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3) + 1
    text = "".join("v %.9g %.9g %.9g\n" % tuple(r) for r in v) + "".join("f %d %d %d\n" % tuple(r) for r in f)
    if hasattr(path_or_file, "write"):
        path_or_file.write(text)
    else:
        with open(path_or_file, "w") as fh:
            fh.write(text)


def read_obj(path):
    """-> (vertices [V, 3] float64, faces [F, 3] int64, 0-based) of a file `write_obj` wrote."""
    v, f = [], []
    with open(path) as fh:
        for line in fh:
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                v.append([float(a) for a in p[1:4]])
            elif p[0] == "f":
                f.append([int(a.split("/")[0]) - 1 for a in p[1:4]])
    return np.asarray(v, np.float64).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)


def _load_results(path):
    """The dict a sampling script saved with np.save (or np.savez, under 'arr_0')."""
    raw = np.load(path, allow_pickle=True)
    if str(path).endswith(".npz"):
        raw = raw["arr_0"]
    return raw.item() if isinstance(raw, np.ndarray) else dict(raw)


class npy2obj:
    """One clip of a `results.npy` as SMPL vertices.  Same arguments, attributes (`vertices` [1, V, 3, T] on the host, `faces`,
    `real_num_frames`, `motions`) and methods as the reference's class, plus `body`: a `model.smpl.SMPLBody` -- the user's SMPL file."""

    def __init__(self, npy_path, sample_idx, rep_idx, body=None, device=0, cuda=True, smplify=None):
        """smplify: a `joints2smpl` built for the clip's frame count, or a factory `num_frames -> joints2smpl`; needed only for
        nfeats == 3."""
        if not cuda or not torch.cuda.is_available():
            raise RuntimeError(_NO_CPU.format("npy2obj"))
        self.npy_path, self.sample_idx, self.rep_idx = npy_path, sample_idx, rep_idx
        self.motions = _load_results(npy_path)
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.rot2xyz = Rotation2xyz(device=self.device, body=body)
        self.faces = self.rot2xyz.smpl_model.faces
        everything = np.asarray(self.motions["motion"])
        self.total_num_samples = int(self.motions["num_samples"])
        self.absl_idx = rep_idx * self.total_num_samples + sample_idx          # repetitions are stacked along the batch
        nfeats = everything.shape[2]
        if nfeats == 3 and smplify is None:
            raise NotImplementedError("npy2obj: nfeats == 3 holds joint positions, which the reference fits with SMPLify (joints2smpl); "
                                      "that fit is not covered here -- pass a sample of SMPL parameters (nfeats == 6)")
        if nfeats not in (3, 6):
            raise ValueError(f"npy2obj: nfeats {nfeats}, expected 6 (24 6D rotations and a translation row)")
        if nfeats == 3:
            joints = np.ascontiguousarray(everything[self.absl_idx], dtype=np.float32).transpose(2, 0, 1)      # [nframes, njoints, 3]
            self.j2s = smplify if hasattr(smplify, "joint2smpl") else smplify(joints.shape[0])
            motion_tensor, self.opt_dict = self.j2s.joint2smpl(joints)
            clip = np.ascontiguousarray(motion_tensor.cpu().numpy(), dtype=np.float32)
        else:
            clip = np.ascontiguousarray(everything[self.absl_idx:self.absl_idx + 1], dtype=np.float32)
        self.motions["motion"] = clip
        self.bs, self.njoints, self.nfeats, self.nframes = clip.shape
        self.num_frames = self.nframes
        self.real_num_frames = int(np.asarray(self.motions["lengths"])[self.absl_idx])
        x = torch.from_numpy(clip).to(self.device)
        verts = self.rot2xyz(x, mask=None, pose_rep="rot6d", translation=True, glob=True, jointstype="vertices", vertstrans=True)
        # the reference adds the ABSOLUTE translation on top of vertstrans' relative one (visualize/vis_utils.py:42-43); kept
        self.root_loc = clip[:, -1, :3, :].reshape(1, 1, 3, -1)
        verts += x[:, -1, :3, :].reshape(1, 1, 3, -1)
        self.vertices = verts.cpu()

    def get_vertices(self, sample_i, frame_i):
        return self.vertices[sample_i, :, :, frame_i].tolist()

    def render_frames(self, **kw):
        """The clip as video frames: `mesh_render.render_meshes` over this object's own vertices -> uint8 [1, T, H, W, 4] on the
        device.  kw: `render_meshes`' (width, height, samples, camera, colors, frames, ...)."""
        from .mesh_render import render_meshes
        kw.setdefault("lengths", [self.real_num_frames])
        return render_meshes(self.vertices.to(self.device), self.rot2xyz.smpl_model.body, **kw)

    def save_obj(self, save_path, frame_i):
        write_obj(save_path, self.vertices[0, :, :, frame_i].numpy(), self.faces)
        return save_path

    def save_npy(self, save_path):
        """The reference's keys: motion, thetas, root_translation, faces, vertices, text, length -- cut to the clip's real length."""
        n, clip = self.real_num_frames, self.motions["motion"][0]
        np.save(save_path, {"motion": clip[..., :n], "thetas": clip[:-1, :, :n], "root_translation": clip[-1, :3, :n], "faces": self.faces,
                            "vertices": self.vertices[0, :, :, :n], "text": self.motions["text"][0], "length": n})


def joints2rotation(joints, num_smplify_iters=150, *, smplify):
    """The reference's joints2rotation (visualize/vis_utils.py:70-80): joints [T, 22, 3] -> the sample [1, 25, 6, T] of the fitted SMPL
    parameters.  As there, the clip's lowest y over all frames and joints is subtracted from `joints` IN PLACE first.  smplify: a
    `joints2smpl`, or a factory `(num_frames, num_smplify_iters) -> joints2smpl`."""
    frames, njoints, nfeats = joints.shape
    MINS = joints.min(axis=0).min(axis=0)
    height_offset = MINS[1]
    joints[:, :, 1] -= height_offset
    j2s = smplify if hasattr(smplify, "joint2smpl") else smplify(frames, num_smplify_iters)
    motion_tensor, opt_dict = j2s.joint2smpl(joints)  # [nframes, njoints, 3]
    return motion_tensor
