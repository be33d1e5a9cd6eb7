"""`joints2smpl`: the reference's visualize/simplify_loc2rot.py over the native fit (visualize/joints2smpl/src/smplify.py).  Joint positions
[T, 22, 3] of one clip become SMPL parameters in the sample layout [1, 25, 6, T]: 24 6D rotations and the root row.

The reference reads ./body_models, the GMM folder and neutral_smpl_mean_params.h5 from fixed paths.  Here they are the caller's:
`body` (an SMPLBody or SMPL), `pose_prior` (a MaxMixturePrior or the path of gmm_08.pkl) and the mean parameters, as arrays
(`mean_pose` [72], `mean_shape` [10]) or as a path in `mean_pose`: an .npz with 'pose' and 'shape', or the reference's .h5, which is
read only when h5py imports.  One clip per fit, as in the reference.

Kept from the reference: HumanML's 22 joints and joints_category 'AMASS'; confidence 1 for every joint; the 6D output through
axis_angle_to_matrix / matrix_to_rotation_6d (utils/rotation_conversions.py:448-500, :555-573); the root row cat(root, zeros); the odd
'pose' entry of the returned dict, `new_opt_joints[0, :24].flatten()` -- joints of frame 0, not a pose."""
import numpy as np
import torch

from ..model.smpl import SMPL, SMPLBody
from .joints2smpl.src.prior import MaxMixturePrior
from .joints2smpl.src.smplify import SMPLify3D


def load_mean_params(path):
    """-> (pose [72], shape [10]) float32 arrays from an .npz with 'pose' and 'shape', or the reference's .h5 when h5py imports."""
    path = str(path)
    if path.endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            return np.asarray(z["pose"], np.float32), np.asarray(z["shape"], np.float32)
    try:
        import h5py
    except ImportError as e:
        raise ImportError(f"joints2smpl: {path} needs the module 'h5py', which is not installed: install it, or hand the mean parameters "
                          "over as arrays (mean_pose=, mean_shape=) or as an .npz with 'pose' and 'shape'") from e
    with h5py.File(path, "r") as fh:
        return np.asarray(fh["pose"][:], np.float32), np.asarray(fh["shape"][:], np.float32)


def axis_angle_to_matrix(a):
    """The reference's axis_angle_to_matrix: axis_angle_to_quaternion (small-angle branch at 1e-6), then quaternion_to_matrix."""
    ang = torch.norm(a, p=2, dim=-1, keepdim=True)
    half = 0.5 * ang
    small = ang.abs() < 1e-6
    s = torch.where(small, 0.5 - (ang * ang) / 48, torch.sin(half) / torch.where(small, torch.ones_like(ang), ang))
    q = torch.cat([torch.cos(half), a * s], dim=-1)
    r, i, j, k = torch.unbind(q, -1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(q.shape[:-1] + (3, 3))


def matrix_to_rotation_6d(m):
    """The reference's own form (utils/rotation_conversions.py:570-573): the first two COLUMNS, the inverse of its
    rotation_6d_to_matrix -- not the first two rows of the function it was derived from."""
    return torch.cat([m[..., 0], m[..., 1]], dim=-1)


class joints2smpl:

    def __init__(self, num_frames, device_id, cuda=True, num_smplify_iters=150, *, body, pose_prior, mean_pose, mean_shape=None):
        what = "joints2smpl"
        if isinstance(body, SMPLBody):
            body = SMPL(body)
        if not isinstance(body, SMPL):
            raise TypeError(f"{what}: body= is an SMPLBody or the package's SMPL; no body model is bundled")
        if isinstance(pose_prior, str):
            pose_prior = MaxMixturePrior.from_pkl(pose_prior)
        if not isinstance(pose_prior, MaxMixturePrior):
            raise TypeError(f"{what}: pose_prior= is a MaxMixturePrior or the path of gmm_08.pkl; no prior file is bundled")
        if isinstance(mean_pose, str):
            mean_pose, mean_shape = load_mean_params(mean_pose)
        if mean_pose is None or mean_shape is None:
            raise TypeError(f"{what}: mean_pose= and mean_shape= are arrays of 72 and 10 values, or mean_pose= is the path of the mean-parameter file")
        mean_pose, mean_shape = np.asarray(mean_pose, np.float32).reshape(-1), np.asarray(mean_shape, np.float32).reshape(-1)
        if mean_pose.shape[0] != 72 or mean_shape.shape[0] != 10:
            raise ValueError(f"{what}: mean_pose of {mean_pose.shape[0]} values and mean_shape of {mean_shape.shape[0]}, expected 72 and 10")
        if int(num_frames) < 1:
            raise ValueError(f"{what}: {num_frames} frames")
        if not cuda or not torch.cuda.is_available():
            raise RuntimeError(f"{what} runs on the GPU only (no CPU fallback)")
        self.device = torch.device("cuda:" + str(device_id)) if isinstance(device_id, int) else torch.device(device_id)
        self.batch_size = int(num_frames)
        self.num_joints = 22  # for HumanML3D
        self.joint_category = "AMASS"
        self.num_smplify_iters = num_smplify_iters
        self.fix_foot = False
        self.init_mean_pose = torch.from_numpy(mean_pose).unsqueeze(0).repeat(self.batch_size, 1).float().to(self.device)
        self.init_mean_shape = torch.from_numpy(mean_shape).unsqueeze(0).repeat(self.batch_size, 1).float().to(self.device)
        self.cam_trans_zero = torch.Tensor([0.0, 0.0, 0.0]).unsqueeze(0).to(self.device)
        self.smplify = SMPLify3D(smplxmodel=body, batch_size=self.batch_size, joints_category=self.joint_category,
                                 num_iters=self.num_smplify_iters, device=self.device, pose_prior=pose_prior)

    def npy2smpl(self, npy_path):
        """Every sample of a results file fitted, saved beside it as *_rot.npy; -> the path.  (The reference ends the process here.)"""
        out_path = npy_path.replace('.npy', '_rot.npy')
        motions = np.load(npy_path, allow_pickle=True)[None][0]
        all_thetas = []
        for sample_i in range(motions['motion'].shape[0]):
            thetas, _ = self.joint2smpl(motions['motion'][sample_i].transpose(2, 0, 1))  # [nframes, njoints, 3]
            all_thetas.append(thetas.cpu().numpy())
        motions['motion'] = np.concatenate(all_thetas, axis=0)
        np.save(out_path, motions)
        return out_path

    def joint2smpl(self, input_joints, init_params=None):
        """input_joints [T, 22, 3] -> (thetas [1, 25, 6, T], {'pose', 'betas', 'cam'})."""
        keypoints_3d = torch.as_tensor(np.asarray(input_joints.detach().cpu() if torch.is_tensor(input_joints) else input_joints),
                                       dtype=torch.float32).to(self.device)
        if keypoints_3d.dim() != 3 or tuple(keypoints_3d.shape[1:]) != (self.num_joints, 3) or keypoints_3d.shape[0] != self.batch_size:
            raise ValueError(f"joints2smpl: joints of shape {tuple(keypoints_3d.shape)}, expected [{self.batch_size}, {self.num_joints}, 3]")
        if init_params is None:
            pred_betas, pred_pose, pred_cam_t = self.init_mean_shape, self.init_mean_pose, self.cam_trans_zero
        else:
            pred_betas, pred_pose, pred_cam_t = init_params['betas'], init_params['pose'], init_params['cam']
        confidence_input = torch.ones(self.num_joints)
        if self.fix_foot:
            confidence_input[[7, 8, 10, 11]] = 1.5
        new_opt_vertices, new_opt_joints, new_opt_pose, new_opt_betas, new_opt_cam_t, new_opt_joint_loss = self.smplify(
            pred_pose.detach(), pred_betas.detach(), pred_cam_t.detach(), keypoints_3d, conf_3d=confidence_input.to(self.device))
        thetas = new_opt_pose.reshape(self.batch_size, 24, 3)
        thetas = matrix_to_rotation_6d(axis_angle_to_matrix(thetas))  # [bs, 24, 6]
        root_loc = keypoints_3d[:, 0]  # [bs, 3]
        root_loc = torch.cat([root_loc, torch.zeros_like(root_loc)], dim=-1).unsqueeze(1)  # [bs, 1, 6]
        thetas = torch.cat([thetas, root_loc], dim=1).unsqueeze(0).permute(0, 2, 3, 1)  # [1, 25, 6, T]
        return thetas.clone().detach(), {'pose': new_opt_joints[0, :24].flatten().clone().detach(), 'betas': new_opt_betas.clone().detach(),
                                         'cam': new_opt_cam_t.clone().detach()}
