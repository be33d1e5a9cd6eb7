"""The SMPL body on the GPU: the counterpart of the reference's model/smpl.py (`SMPL`, an `smplx.SMPLLayer` with more joints) with
nothing of `smplx` underneath: the standard linear blend skinning is three HIP kernels (csrc/mst_smpl.h; `mst_smpl_pose`,
`mst_smpl_skin`, `mst_smpl_regress`), forward only, fp32.

`SMPLBody` holds the arrays of one body -- the user's file, as the CLIP checkpoint is; nothing is bundled.  `SMPL(body)` has the
reference's call surface: `forward(body_pose, global_orient, betas)` -> {'vertices', 'vibe', 'a2m', 'smpl', 'a2mpl'}, `.faces`,
`.maps`, `.num_betas`.  `model/rotation2xyz.py` is what the pipeline calls.

The list of 54 joints the maps index: the 24 posed joints, the vertices at `vertex_ids` (21: nose, eyes, ears, six feet points, the
finger tips of the left and of the right hand), then the 9 rows of `J_regressor_extra` over the vertices."""
import ctypes as C
import pickle

import numpy as np
import torch

from .. import _native as N

_NO_CPU = "{} runs on the GPU only (no CPU fallback); move the motion to cuda"
NUM_JOINTS = 24
NUM_BETAS = 10
NUM_VERTEX_IDS = 21
NUM_EXTRA = 9
POSE_REPS = {"rot6d": (0, 6), "rotmat": (1, 9), "rotquat": (2, 4), "rotvec": (3, 3)}

# SMPL's public kinematic tree
SMPL_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)

# ---- the joint lists, as indices into the list of 54 (held to the reference's `maps` and JOINTSTYPE_ROOT by tests/golden/smpl.npz)
_OPENPOSE_25 = (24, 12, 17, 19, 21, 16, 18, 20, 0, 2, 5, 8, 1, 4, 7) + tuple(range(25, 35))     # body 15, then eyes, ears, feet
_LSP_14 = (8, 5, 45, 46, 4, 7, 21, 19, 17, 16, 18, 20, 47, 48)                                  # ankle .. wrist right-left, neck, head top
_MPII_H36M_FACE = (49, 50, 51, 52, 53, 24, 26, 25, 28, 27)
VIBE_INDEXES = _OPENPOSE_25 + _LSP_14 + _MPII_H36M_FACE                                         # 49 joints
_A2M_OF_VIBE = (8, 1, 2, 3, 4, 5, 6, 7, 0, 9, 10, 11, 12, 13, 14, 21, 24, 38)                   # OpenPose body with nose and hip swapped, heel, ankle, head
A2M_INDEXES = tuple(VIBE_INDEXES[i] for i in _A2M_OF_VIBE)
SMPL_INDEXES = tuple(range(NUM_JOINTS))
A2MPL_INDEXES = tuple(sorted(set(SMPL_INDEXES) | set(A2M_INDEXES)))
JOINTSTYPE_ROOT = {"a2m": 0, "smpl": 0, "a2mpl": 0, "vibe": 8}
JOINTSTYPES = ["a2m", "a2mpl", "smpl", "vibe", "vertices"]


def joint_maps():
    """name -> int64 array, the reference's `SMPL.maps`."""
    return {"vibe": np.array(VIBE_INDEXES), "a2m": np.array(A2M_INDEXES), "smpl": np.array(SMPL_INDEXES), "a2mpl": np.array(A2MPL_INDEXES)}


# smplx's `vertex_ids['smplh']` as recalled, UNVERIFIED here (no SMPL file and no smplx on the authoring machine): check it against
# your smplx before relying on it.  Only meaningful on the 6890-vertex topology; no test depends on it.
SMPL_6890_VERTEX_IDS_UNVERIFIED = (332, 6260, 2800, 4071, 583, 3216, 3226, 3387, 6617, 6624, 6787,
                                   2746, 2319, 2445, 2556, 2673, 6191, 5782, 5905, 6016, 6133)


def _dense(a):
    return a.toarray() if hasattr(a, "toarray") else np.asarray(a)


class SMPLBody:
    """The arrays of one body.  Built on the host (validated there, no GPU needed); the device copies, the joint tables J0 / Jdirs
    (J_regressor applied to v_template and to shapedirs in double) and the packed skinning operand are made on first use on `device`.

    v_template [V, 3], shapedirs [V, 3, >= 10] (the first 10 are kept), posedirs [207, 3 V] or the files' [V, 3, 207], J_regressor
    [24, V], parents [24], lbs_weights [V, 24], faces [F, 3], J_regressor_extra [9, V], vertex_ids [21]."""

    def __init__(self, v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights, faces, J_regressor_extra, vertex_ids,
                 device="cuda"):
        what = "SMPLBody"
        vt = np.ascontiguousarray(_dense(v_template), dtype=np.float64)
        if vt.ndim != 2 or vt.shape[1] != 3 or vt.shape[0] < 1:
            raise ValueError(f"{what}: v_template of shape {vt.shape}, expected [V, 3]")
        V = vt.shape[0]
        sd = np.asarray(_dense(shapedirs), dtype=np.float64)
        if sd.ndim != 3 or sd.shape[:2] != (V, 3) or sd.shape[2] < NUM_BETAS:
            raise ValueError(f"{what}: shapedirs of shape {sd.shape}, expected [{V}, 3, >= {NUM_BETAS}]")
        sd = np.ascontiguousarray(sd[..., :NUM_BETAS])
        pd = np.asarray(_dense(posedirs), dtype=np.float64)
        K = 9 * (NUM_JOINTS - 1)
        if pd.shape == (V, 3, K):
            pd = pd.reshape(3 * V, K).T                   # smplx: posedirs.reshape(-1, 207).T
        if pd.shape != (K, 3 * V):
            raise ValueError(f"{what}: posedirs of shape {pd.shape}, expected [{K}, {3 * V}] or [{V}, 3, {K}]")
        jr = np.asarray(_dense(J_regressor), dtype=np.float64)
        if jr.shape != (NUM_JOINTS, V):
            raise ValueError(f"{what}: J_regressor of shape {jr.shape}, expected [{NUM_JOINTS}, {V}] (only bodies of {NUM_JOINTS} joints are built)")
        par = np.asarray(parents).astype(np.int64).reshape(-1)
        if par.shape[0] != NUM_JOINTS:
            raise ValueError(f"{what}: {par.shape[0]} parents, expected {NUM_JOINTS} (only bodies of {NUM_JOINTS} joints are built)")
        if par[0] != -1:
            raise ValueError(f"{what}: parents[0] = {par[0]}, the root's is -1")
        for j in range(1, NUM_JOINTS):
            if not 0 <= par[j] < j:
                raise ValueError(f"{what}: parents[{j}] = {par[j]} is not an earlier joint")
        w = np.asarray(_dense(lbs_weights), dtype=np.float64)
        if w.shape != (V, NUM_JOINTS):
            raise ValueError(f"{what}: lbs_weights of shape {w.shape}, expected [{V}, {NUM_JOINTS}]")
        for name, a in (("lbs_weights", w), ("J_regressor", jr)):
            worst = float(np.abs(a.sum(1) - 1).max())
            if not worst <= 1e-4:
                raise ValueError(f"{what}: a row of {name} sums to 1 {worst:+.3e}; every row must sum to 1 within 1e-4")
        f = np.asarray(_dense(faces)).astype(np.int64)
        if f.ndim != 2 or f.shape[1] != 3:
            raise ValueError(f"{what}: faces of shape {f.shape}, expected [F, 3]")
        if f.size and (f.min() < 0 or f.max() >= V):
            raise ValueError(f"{what}: faces name vertex {f.min() if f.min() < 0 else f.max()}, outside 0..{V - 1}")
        ex = np.asarray(_dense(J_regressor_extra), dtype=np.float64)
        if ex.shape != (NUM_EXTRA, V):
            raise ValueError(f"{what}: J_regressor_extra of shape {ex.shape}, expected [{NUM_EXTRA}, {V}]")
        ids = np.asarray(vertex_ids).astype(np.int64).reshape(-1)
        if ids.shape[0] != NUM_VERTEX_IDS:
            raise ValueError(f"{what}: {ids.shape[0]} vertex_ids, expected {NUM_VERTEX_IDS}")
        if ids.min() < 0 or ids.max() >= V:
            raise ValueError(f"{what}: vertex id {ids.min() if ids.min() < 0 else ids.max()} outside 0..{V - 1}")
        for name, a in (("v_template", vt), ("shapedirs", sd), ("posedirs", pd), ("J_regressor", jr), ("lbs_weights", w), ("J_regressor_extra", ex)):
            if not np.isfinite(a).all():
                raise ValueError(f"{what}: {name} is not finite")
        self.num_vertices = V
        self.v_template, self.shapedirs, self.posedirs = vt.astype(np.float32), sd.astype(np.float32), np.ascontiguousarray(pd, dtype=np.float32)
        self.J_regressor, self.lbs_weights, self.J_regressor_extra = jr.astype(np.float32), w.astype(np.float32), ex.astype(np.float32)
        self.parents, self.faces, self.vertex_ids = par, f, ids
        # J = J_regressor (v_template + shapedirs beta) = J0 + Jdirs beta, formed once in double
        self.J0 = (jr @ vt).astype(np.float32)                                      # [24, 3]
        self.Jdirs = np.einsum("jv,vci->jci", jr, sd).astype(np.float32)           # [24, 3, 10]
        self.device = torch.device(device)
        self._dev = {}                                    # device -> the uploaded arrays, made on first use there

    @property
    def topology(self):
        """The faces and their vertex -> faces adjacency as `visualize.mesh_render.render_meshes` reads them, built once."""
        if getattr(self, "_topology", None) is None:
            from ..visualize.mesh_render import MeshTopology
            self._topology = MeshTopology(self.faces, self.num_vertices)
        return self._topology

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_arrays(cls, *, v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights, faces, J_regressor_extra, vertex_ids,
                    device="cuda"):
        return cls(v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights, faces, J_regressor_extra, vertex_ids, device)

    @classmethod
    def _from_mapping(cls, what, d, J_regressor_extra, vertex_ids, device):
        def pick(*names):
            for n in names:
                if n in d:
                    return d[n]
            raise KeyError(f"{what}: none of {names} in the file (keys: {sorted(d)[:20]})")
        if "parents" in d:
            parents = np.asarray(d["parents"]).astype(np.int64)
        else:
            parents = np.asarray(pick("kintree_table")).astype(np.int64)[0].copy()
            parents[0] = -1                               # the files store 2^32 - 1
        if J_regressor_extra is None:
            J_regressor_extra = pick("J_regressor_extra")
        if vertex_ids is None:
            vertex_ids = pick("vertex_ids")
        return cls(pick("v_template"), pick("shapedirs"), pick("posedirs"), pick("J_regressor"), parents, pick("lbs_weights", "weights"),
                   pick("faces", "f"), J_regressor_extra, vertex_ids, device)

    @classmethod
    def from_npz(cls, path, J_regressor_extra=None, vertex_ids=None, device="cuda"):
        """An .npz with SMPL's key names (v_template, shapedirs, posedirs, J_regressor, kintree_table or parents, weights or
        lbs_weights, f or faces).  J_regressor_extra (an array or the .npy the reference's JOINT_REGRESSOR_TRAIN_EXTRA names) and
        vertex_ids come from the arguments or from keys of those names."""
        if isinstance(J_regressor_extra, str):
            J_regressor_extra = np.load(J_regressor_extra)
        with np.load(path, allow_pickle=False) as z:
            return cls._from_mapping("SMPLBody.from_npz", {k: z[k] for k in z.files}, J_regressor_extra, vertex_ids, device)

    @classmethod
    def from_pkl(cls, path, J_regressor_extra=None, vertex_ids=None, device="cuda"):
        """A pickle of numpy / scipy-sparse arrays under SMPL's key names, read with encoding='latin1' (what smplx does with
        SMPL_NEUTRAL.pkl).  The original SMPL pickles hold `chumpy` objects: when the file needs a module that is not installed the
        error says which, and the file has to be converted first (SMPL's own clean-up script writes plain numpy).  Unpickling runs
        code: only open files you trust.  NOT tried against a real SMPL file -- none was available when this was written; the
        tests use synthetic files."""
        if isinstance(J_regressor_extra, str):
            J_regressor_extra = np.load(J_regressor_extra)
        try:
            with open(path, "rb") as fh:
                d = pickle.load(fh, encoding="latin1")
        except ModuleNotFoundError as e:
            raise ImportError(f"SMPLBody.from_pkl: {path} needs the module {e.name!r}, which is not installed (the original SMPL "
                              "pickles hold chumpy arrays): install it, or convert the file to plain numpy arrays / an .npz first") from e
        if not isinstance(d, dict):
            raise ValueError(f"SMPLBody.from_pkl: {path} holds a {type(d).__name__}, expected a dict of arrays")
        return cls._from_mapping("SMPLBody.from_pkl", d, J_regressor_extra, vertex_ids, device)

    def to(self, device):
        """The device `run` uses when it is handed none.  Copies made on another device are kept."""
        self.device = torch.device(device)
        return self

    # ------------------------------------------------------------------ device state
    def _state(self, device):
        device = torch.device(device)
        if device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError(_NO_CPU.format("SMPLBody"))
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._dev:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
            V = self.num_vertices
            posedirs, shapedirs = up(self.posedirs), up(self.shapedirs)
            nbytes = int(N.lib().mst_smpl_packed_bytes(V))
            if nbytes < 0:
                N.check(1)
            packed = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
            with torch.cuda.device(device):
                N.check(N.lib().mst_smpl_pack_body(N.ptr(posedirs), N.ptr(shapedirs), V, N.ptr(packed), N.stream_ptr(device)))
                torch.cuda.current_stream(device).synchronize()            # posedirs / shapedirs are dropped below
            self._dev[device] = {"packed": packed, "v_template": up(self.v_template), "weights": up(self.lbs_weights), "J0": up(self.J0),
                         "Jdirs": up(self.Jdirs), "extra": up(self.J_regressor_extra)}
        return self._dev[device]

    def run(self, x, strides, frame_ids, live, batch, frames, sample_joints, pose_rep, glob, glob_rot, betas, beta, trans_joint,
            jointstype, joint_map=None, root=-1, layout="reference", rotations=False, out=None):
        """One chain of launches on the current stream of x's device.  x: the CUDA float32 storage that element (b, j, f, t) is
        read from through `strides` = (batch, joint, feature, frame).  -> (out, rotations [live, 24, 3, 3] or None, the workspace).  `out`
        is written for live frames only: [B, n, 3, T], or [B, T, V, 3] for vertices with layout='frames'.  jointstype 'smpl' stops after
        the pose kernel, 'vertices' adds the skinning kernel, anything else (a `joint_map` into the list of 54, `root` the output index
        that is subtracted or -1) skins into the workspace, whose last region then holds the vertices [live, V, 3], and regresses."""
        st = self._state(x.device)
        dev, V, lib = x.device, self.num_vertices, N.lib()
        need_verts = jointstype not in ("smpl", "vertices")
        nbytes = int(lib.mst_smpl_workspace_bytes(live, V, int(need_verts)))
        if nbytes < 0:
            N.check(1)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rot = torch.empty(live, NUM_JOINTS, 3, 3, dtype=torch.float32, device=dev) if rotations else None
        sb, sj, sf, stt = (int(s) for s in strides)
        trans_ptr = None if trans_joint < 0 else C.c_void_p(x.data_ptr() + 4 * trans_joint * sj)
        n_out = {"smpl": NUM_JOINTS, "vertices": V}.get(jointstype, None if joint_map is None else len(joint_map))
        if out is None:
            shape = (batch, frames, V, 3) if (jointstype == "vertices" and layout == "frames") else (batch, n_out, 3, frames)
            out = torch.empty(shape, dtype=torch.float32, device=dev)
        groot = None if glob_rot is None else (C.c_float * 3)(*[float(a) for a in glob_rot])
        par = (C.c_int32 * NUM_JOINTS)(*[int(a) for a in self.parents])
        stream = N.stream_ptr(dev)
        with torch.cuda.device(dev):
            N.check(lib.mst_smpl_pose(N.ptr(x), sb, sj, sf, stt, N.ptr(frame_ids), live, batch, frames, sample_joints, NUM_JOINTS, V,
                                      int(need_verts), POSE_REPS[pose_rep][0], int(bool(glob)), groot, N.ptr(betas), float(beta),
                                      N.ptr(st["J0"]), N.ptr(st["Jdirs"]), par, trans_joint if jointstype == "smpl" else -1, N.ptr(ws),
                                      N.ptr(rot), N.ptr(out) if jointstype == "smpl" else None, stream))
            if jointstype == "vertices":
                os_ = (frames * V * 3, 3 * V, 3, 1) if layout == "frames" else (V * 3 * frames, 1, 3 * frames, frames)
                N.check(lib.mst_smpl_skin(N.ptr(st["packed"]), N.ptr(st["v_template"]), N.ptr(st["weights"]), V, 0, N.ptr(frame_ids), live,
                                          batch, frames, N.ptr(ws), trans_ptr, sb, sf, stt, N.ptr(out), *os_, stream))
            elif need_verts:
                N.check(lib.mst_smpl_skin(N.ptr(st["packed"]), N.ptr(st["v_template"]), N.ptr(st["weights"]), V, 1, N.ptr(frame_ids), live,
                                          batch, frames, N.ptr(ws), None, 0, 0, 0, None, 0, 0, 0, 0, stream))
                ids = (C.c_int32 * NUM_VERTEX_IDS)(*[int(a) for a in self.vertex_ids])
                jm = (C.c_int32 * len(joint_map))(*[int(a) for a in joint_map])
                N.check(lib.mst_smpl_regress(N.ptr(ws), N.ptr(st["extra"]), ids, V, N.ptr(frame_ids), live, batch, frames, jm, len(joint_map),
                                             int(root), trans_ptr, sb, sf, stt, N.ptr(out), stream))
        return out, rot, ws


class SMPL:
    """The reference's `SMPL` on a `SMPLBody`: `forward(body_pose, global_orient, betas)` -> the dict of the reference ('vertices' [N, V, 3]
    and the four joint lists [N, n, 3], no root subtracted), `.faces`, `.maps`, `.num_betas`.  Not an nn.Module: there are no
    parameters and no gradients; `eval()` and `to(device)` are there for the reference's `SMPL().eval().to(device)`."""
    num_betas = NUM_BETAS

    def __init__(self, body):
        if not isinstance(body, SMPLBody):
            raise TypeError("SMPL: body is a SMPLBody (from_arrays / from_npz / from_pkl); no body model is bundled")
        self.body = body
        self.faces = body.faces
        self.maps = joint_maps()

    @property
    def topology(self):
        return self.body.topology

    def eval(self):
        return self

    def to(self, device):
        self.body.to(device)
        return self

    def forward(self, body_pose, global_orient, betas=None, **kwargs):
        what = "SMPL.forward"
        if kwargs:
            raise TypeError(f"{what}: unexpected arguments {sorted(kwargs)} (no transl, no pose2rot: rotation matrices in, as the reference calls it)")
        if not (torch.is_tensor(body_pose) and torch.is_tensor(global_orient)):
            raise TypeError(f"{what}: body_pose and global_orient are tensors")
        if not body_pose.is_cuda:
            raise RuntimeError(_NO_CPU.format(what))
        n = body_pose.shape[0]
        if tuple(body_pose.shape) != (n, NUM_JOINTS - 1, 3, 3):
            raise ValueError(f"{what}: body_pose of shape {tuple(body_pose.shape)}, expected [N, {NUM_JOINTS - 1}, 3, 3]")
        if global_orient.numel() != n * 9:
            raise ValueError(f"{what}: global_orient of shape {tuple(global_orient.shape)}, expected [N, 3, 3] or [N, 1, 3, 3]")
        rot = torch.cat([global_orient.reshape(n, 1, 9), body_pose.reshape(n, NUM_JOINTS - 1, 9)], 1).float().contiguous()
        if betas is not None:
            betas = _checked_betas(what, betas, n, rot.device)
        V = self.body.num_vertices
        if n == 0:
            out = {"vertices": rot.new_zeros(0, V, 3)}
            out.update({k: rot.new_zeros(0, len(m), 3) for k, m in self.maps.items()})
            return out
        every = list(range(NUM_JOINTS + NUM_VERTEX_IDS + NUM_EXTRA))
        joints, _, ws = self.body.run(rot, (0, 9, 1, NUM_JOINTS * 9), None, n, 1, n, NUM_JOINTS, "rotmat", True, None, betas, 0.0, -1, "all",
                                      joint_map=every, root=-1)
        verts = ws[ws.numel() - _up256(n * V * 12):][:n * V * 12].view(torch.float32).view(n, V, 3).clone()    # the workspace's last region
        joints = joints[0].permute(2, 0, 1)                                 # [54, 3, N] -> [N, 54, 3]
        out = {"vertices": verts}
        for name, idx in self.maps.items():
            out[name] = joints[:, torch.as_tensor(idx, device=joints.device)]
        return out

    __call__ = forward


def _up256(b):
    return (b + 255) // 256 * 256


def _checked_betas(what, betas, n, device):
    if not torch.is_tensor(betas):
        betas = torch.as_tensor(np.asarray(betas, dtype=np.float32))
    if tuple(betas.shape) != (n, NUM_BETAS):
        raise ValueError(f"{what}: betas of shape {tuple(betas.shape)}, expected [{n}, {NUM_BETAS}] (one row per live frame)")
    return betas.to(device=device, dtype=torch.float32).contiguous()
