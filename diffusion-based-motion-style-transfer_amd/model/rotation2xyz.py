"""`Rotation2xyz` on the GPU: the reference's model/rotation2xyz.py:11-92 over the native SMPL body (model/smpl.py, csrc/mst_smpl.h).
Rotations in, joints or vertices out, for a whole batch of clips: the sample is read where it lies (any strides, no permute, no
copy) and the result is written in the reference's [B, n, 3, T].  Forward only.

Kept from the reference: `pose_rep` 'xyz' returns x as it is; the 6D form is the reference's own (x normalised, z = x cross y_raw
normalised, y = z cross x, as columns, no epsilon); 'rotvec' goes through its axis_angle_to_quaternion (small-angle branch at 1e-6)
and quaternion_to_matrix (2 / |q|^2); `translation=True` takes row -1, features :3; `glob=False` takes one axis-angle `glob_rot` for
every frame; frames the mask rules out are never computed and are zero before the root subtraction and the translation; every list but
'vertices' has its root joint (JOINTSTYPE_ROOT) subtracted; `vertstrans` adds trans - trans[..., [0]] to every frame, dead ones
included; `betas=None` means zeros with betas[:, 1] = beta; `get_rotations_back` returns the matrices.

One synchronisation per call when a mask is given: the live frames are compacted on the device and counted on the host (the
reference's `x_rotations[mask]` does the same)."""
import numpy as np
import torch

from .smpl import JOINTSTYPE_ROOT, JOINTSTYPES, NUM_JOINTS, POSE_REPS, SMPL, SMPLBody, _NO_CPU, _checked_betas  # noqa: F401


class Rotation2xyz:
    def __init__(self, device, dataset='amass', body=None):
        """body: a `SMPLBody` (or an `SMPL` built on one).  The reference loads ./body_models/smpl itself; here the body is the
        caller's file and nothing is bundled."""
        if isinstance(body, SMPL):
            body = body.body
        if not isinstance(body, SMPLBody):
            raise TypeError("Rotation2xyz: body= is a SMPLBody (SMPLBody.from_npz / from_pkl / from_arrays); no body model is bundled")
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.dataset = dataset
        self.smpl_model = SMPL(body).eval().to(self.device)

    def __call__(self, x, mask, pose_rep, translation, glob, jointstype, vertstrans, betas=None, beta=0, glob_rot=None,
                 get_rotations_back=False, layout="reference", **kwargs):
        what = "Rotation2xyz"
        if pose_rep == "xyz":
            return x
        if not glob and glob_rot is None:
            raise TypeError("You must specify global rotation if glob is False")
        if jointstype not in JOINTSTYPES:
            raise NotImplementedError("This jointstype is not implemented.")
        if pose_rep not in POSE_REPS:
            raise NotImplementedError("No geometry for this one.")
        if layout not in ("reference", "frames") or (layout == "frames" and jointstype != "vertices"):
            raise ValueError(f"{what}: layout {layout!r}: 'reference' ([B, n, 3, T]) or, for vertices, 'frames' ([B, T, V, 3])")
        if not torch.is_tensor(x) or x.dim() != 4:
            raise TypeError(f"{what}: x is a tensor [B, joints, feats, T]")
        if not x.is_cuda or (mask is not None and torch.is_tensor(mask) and not mask.is_cuda):
            raise RuntimeError(_NO_CPU.format(what))
        body = self.smpl_model.body
        x = x.detach()
        if x.dtype != torch.float32:
            x = x.float()
        B, rows, feats, T = x.shape
        nrot = rows - 1 if translation else rows
        want = NUM_JOINTS if glob else NUM_JOINTS - 1
        if nrot != want:
            raise ValueError(f"{what}: {nrot} rotation rows (x has {rows}, translation={bool(translation)}), the body takes {want} with glob={bool(glob)}")
        nf = POSE_REPS[pose_rep][1]
        if feats != nf:
            raise ValueError(f"{what}: {feats} features, pose_rep {pose_rep!r} has {nf}")
        if B < 1 or T < 1:
            raise ValueError(f"{what}: {B} clips of {T} frames")
        if glob_rot is not None:
            glob_rot = np.asarray(glob_rot.detach().cpu() if torch.is_tensor(glob_rot) else glob_rot, dtype=np.float32).reshape(-1)
            if glob_rot.shape[0] != 3:
                raise ValueError(f"{what}: glob_rot is one axis-angle (3 values)")
        dev = x.device
        if mask is None:
            live = B * T
            ids = None if B == 1 else torch.arange(B * T, dtype=torch.int32, device=dev)
        else:
            mask = torch.as_tensor(mask, device=dev)
            if tuple(mask.shape) != (B, T):
                raise ValueError(f"{what}: mask of shape {tuple(mask.shape)}, expected [{B}, {T}]")
            ids = mask.reshape(-1).to(torch.bool).nonzero().reshape(-1).to(torch.int32)
            live = int(ids.numel())
        if betas is not None:
            betas = _checked_betas(what, betas, live, dev)
        trans = bool(translation and vertstrans)
        n_out = body.num_vertices if jointstype == "vertices" else len(self.smpl_model.maps[jointstype])
        shape = (B, T, n_out, 3) if layout == "frames" else (B, n_out, 3, T)
        if live == B * T:
            out = torch.empty(shape, dtype=torch.float32, device=dev)
        elif trans:                                       # dead frames: 0 + (trans - trans[..., [0]])
            d = x[:, -1, :3, :] - x[:, -1, :3, :1]
            d = d.permute(0, 2, 1)[:, :, None, :] if layout == "frames" else d[:, None, :, :]
            out = (torch.zeros(shape, dtype=torch.float32, device=dev) + d).contiguous()
        else:
            out = torch.zeros(shape, dtype=torch.float32, device=dev)
        rot = None
        if live:
            joint_map = None if jointstype in ("smpl", "vertices") else [int(i) for i in self.smpl_model.maps[jointstype]]
            out, rot, _ = body.run(x, x.stride(), ids, live, B, T, nrot, pose_rep, glob, glob_rot, betas, float(beta),
                                   rows - 1 if trans else -1, jointstype, joint_map=joint_map, root=JOINTSTYPE_ROOT.get(jointstype, -1),
                                   layout=layout, rotations=get_rotations_back, out=out)
        if get_rotations_back:
            if rot is None:
                rot = torch.zeros(0, NUM_JOINTS, 3, 3, dtype=torch.float32, device=dev)
            if glob:
                return out, rot[:, 1:], rot[:, 0]
            return out, rot[:, 1:], rot[:, :1]
        return out
