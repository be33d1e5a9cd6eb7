"""Guides for the `cond_fn` argument of p_sample / ddim_sample and their loops (reference gaussian_diffusion.py:454-506).

A cond_fn returns grad log p(y | x_t).  Any callable works: the samplers evaluate it on x_t in front of each step and hand the
tensor to the step kernel (MST_GUIDE_GRADIENT, one step per engine call).  A `TargetGuide` is the one guide the step kernel
computes itself (MST_GUIDE_TARGET): its operands are constant over the loop, so a guided loop stays one native call.

A `JointGuide` is a cond_fn of the OTHER kind, the with-grad one of p_sample_with_grad / ddim_sample_with_grad and the loops under
cond_fn_with_grad=True (reference gaussian_diffusion.py:469-482, :508-530): cond_fn(x, t, p_mean_var, **model_kwargs), evaluated on the
denoised clip p_mean_var["pred_xstart"], which is in x's graph."""
import numpy as np
import torch as th


class TargetGuide:
    """g = weight[b] * mask * (a_t * target - x_t): the gradient of a Gaussian log-likelihood that pulls the masked entries of x_t
    towards a_t * target -- soft keyframes, a root trajectory, contact terms on top of the inpainting mask.

    target: [B,F,1,T] (or broadcastable to x), mask: the same or None for all ones, weight: a scalar or one value per clip.
    alphas_cumprod None: a_t = 1.  Otherwise a_t = sqrt(alphas_cumprod[t]): the target follows the schedule, as q_sample's mean does.
    It is the ORIGINAL process's table, indexed by the timesteps a cond_fn receives -- under SpacedDiffusion those are
    timestep_map[t], not the respaced indices.  Rescaled (float) timesteps cannot index it and are refused."""

    def __init__(self, target, mask=None, weight=1.0, alphas_cumprod=None):
        self.target = th.as_tensor(target, dtype=th.float32)
        self.mask = None if mask is None else th.as_tensor(mask, dtype=th.float32)
        self.weight = th.as_tensor(weight, dtype=th.float32).reshape(-1)
        self.alphas_cumprod = None if alphas_cumprod is None else np.asarray(alphas_cumprod, dtype=np.float64)

    def __call__(self, x, t, **model_kwargs):
        """The gradient in plain torch, on x's device: what the step kernel computes for MST_GUIDE_TARGET."""
        if th.is_floating_point(t):
            raise ValueError("TargetGuide: rescaled (float) timesteps cannot index alphas_cumprod; use rescale_timesteps=False")
        B = x.shape[0]
        view = (B,) + (1,) * (x.dim() - 1)
        y = self.target.to(device=x.device)
        w = self.weight.to(device=x.device)
        w = (w.expand(B) if w.numel() == 1 else w).view(view)
        if self.alphas_cumprod is None:
            d = y - x.float()
        else:
            a = th.from_numpy(np.sqrt(self.alphas_cumprod)).to(device=x.device)[t.long()].float().view(view)
            d = a * y - x.float()
        if self.mask is None:
            return w * d
        return (w * self.mask.to(device=x.device)) * d


class JointGuide:
    """A with-grad cond_fn (reference gaussian_diffusion.py:469-482, :508-530) that constrains world-space JOINTS of the denoised clip:
    log p = -1/2 scale sum_{t < len, j, c} weight (recover_from_ric(x0-hat * std + mean, n_joints) - target)^2, a wrist at a point in
    frame 40, a root on a floor path, a foot that stays put.  The likelihood and its gradient with respect to x0-hat are ONE native launch
    (engine.joint_guide); from there the gradient travels to x_t through the step's graph -- the inpainting blend, the clamp and the native
    training node, whose backward is the input-gradient-only pass (the samplers run the model inside `native_stack.input_grad_only()`).

    target, weight: [B,T,n_joints,3]; weight >= 0 per axis, 0 = unconstrained.  mean, std: [F] of the dataset.  scale: one value or one
    per clip.  lengths: [B], or None: model_kwargs['y']['lengths'] when the call carries them, else every clip is T long.
    Use with p_sample_with_grad / ddim_sample_with_grad, or the loops with cond_fn_with_grad=True."""

    def __init__(self, target, weight, mean, std, n_joints, scale=1.0, lengths=None):
        self.target = th.as_tensor(target, dtype=th.float32)
        self.weight = th.as_tensor(weight, dtype=th.float32)
        self.n_joints = int(n_joints)
        if self.target.dim() != 4 or self.target.shape[2:] != (self.n_joints, 3):
            raise ValueError(f"JointGuide: target must be [B, T, {self.n_joints}, 3], got {tuple(self.target.shape)}")
        if self.weight.shape != self.target.shape:
            raise ValueError(f"JointGuide: weight {tuple(self.weight.shape)} is not target's shape {tuple(self.target.shape)}")
        if bool((self.weight < 0).any()):
            raise ValueError("JointGuide: weight must be >= 0 (0 = unconstrained)")
        self.mean = th.as_tensor(mean, dtype=th.float32).reshape(-1)
        self.std = th.as_tensor(std, dtype=th.float32).reshape(-1)
        if self.mean.numel() != self.std.numel() or self.mean.numel() < 4 + 3 * (self.n_joints - 1) or self.n_joints < 1:
            raise ValueError(f"JointGuide: {self.mean.numel()} / {self.std.numel()} mean / std values cannot hold {self.n_joints} joints "
                             "(4 + 3 (J - 1) position channels)")
        self.scale = th.as_tensor(scale, dtype=th.float32).reshape(-1)
        B, T = self.target.shape[:2]
        if self.scale.numel() not in (1, B):
            raise ValueError(f"JointGuide: {self.scale.numel()} scale values for {B} clips (one value, or one per clip)")
        self.lengths = None if lengths is None else self._check_lengths(lengths, B, T)
        self._dev = {}

    @staticmethod
    def _check_lengths(lengths, B, T):
        n = th.as_tensor(lengths).reshape(-1)
        if n.numel() != B:
            raise ValueError(f"JointGuide: {n.numel()} lengths for {B} clips")
        # values: checked where they are on the host; a device tensor (y['lengths'] of a running loop) is not read back every step --
        # the kernel clamps what it reads into 0..T
        if not n.is_cuda and (bool((n < 0).any()) or bool((n > T).any())):
            raise ValueError(f"JointGuide: lengths must be in 0..{T}, got {n.tolist()}")
        return n.to(th.int32)

    def _operands(self, device):
        """The constant operands on `device`, moved once."""
        ops = self._dev.get(device)
        if ops is None:
            ops = self._dev[device] = tuple(v.to(device).contiguous() for v in (self.target, self.weight, self.mean, self.std, self.scale))
        return ops

    def log_prob_grad(self, x0, lengths=None):
        """(logp [B], d logp / d x0 [B,F,1,T]) of x0 [B,F,1,T], a float32 GPU tensor: the kernel."""
        from .. import engine as _eng
        B, T = self.target.shape[:2]
        if x0.dim() != 4 or x0.shape[0] != B or x0.shape[2] != 1 or x0.shape[3] != T or x0.shape[1] != self.mean.numel():
            raise ValueError(f"JointGuide: x0 {tuple(x0.shape)} is not [{B}, {self.mean.numel()}, 1, {T}] (the guide's clips, features and frames)")
        if T > _eng.joint_guide_max_frames():
            raise ValueError(f"JointGuide: {T} frames > {_eng.joint_guide_max_frames()} (engine.joint_guide_max_frames)")
        if lengths is None:
            lengths = self.lengths
        elif lengths is not self.lengths:
            lengths = self._check_lengths(lengths, B, T)
        target, weight, mean, std, scale = self._operands(x0.device)
        return _eng.joint_guide(x0, mean, std, self.n_joints, target, weight, scale, lengths=lengths)

    def __call__(self, x, t, p_mean_var, **model_kwargs):
        """grad log p(y | x_t): g0 from the kernel on the detached x0-hat, then through the step's graph to x."""
        pred = p_mean_var["pred_xstart"]
        lengths = self.lengths
        if lengths is None:
            lengths = (model_kwargs.get("y") or {}).get("lengths")
        _, g0 = self.log_prob_grad(pred.detach(), lengths)
        return th.autograd.grad(pred, x, grad_outputs=g0)[0]

    # ---- dense operands from sparse input, on the host
    @staticmethod
    def keyframes(shape, joints, frames, positions, weight=1.0, clips=None):
        """(target, weight) [B,T,J,3] from K keyframes: joint joints[k] of clip clips[k] (None: every clip) at frame frames[k] is asked
        to be at positions[k] ([K,3]) with weight[k] (a scalar, [K] or [K,3] per axis).  shape: (B, T, J)."""
        B, T, J = (int(v) for v in shape)
        joints = np.asarray(joints, dtype=np.int64).reshape(-1)
        frames = np.asarray(frames, dtype=np.int64).reshape(-1)
        K = joints.size
        positions = np.asarray(positions, dtype=np.float32).reshape(K, 3)
        w = np.asarray(weight, dtype=np.float32)
        w = np.broadcast_to(w.reshape(-1, 1) if w.ndim <= 1 else w, (K, 3))
        if frames.size != K or (clips is not None and np.asarray(clips).size != K):
            raise ValueError(f"JointGuide.keyframes: {K} joints, {frames.size} frames: one of each per keyframe")
        if K and (joints.min() < 0 or joints.max() >= J or frames.min() < 0 or frames.max() >= T):
            raise ValueError(f"JointGuide.keyframes: a joint outside 0..{J - 1} or a frame outside 0..{T - 1}")
        if (w < 0).any():
            raise ValueError("JointGuide.keyframes: weight must be >= 0")
        target, weights = np.zeros((B, T, J, 3), np.float32), np.zeros((B, T, J, 3), np.float32)
        for k in range(K):
            which = slice(None) if clips is None else int(np.asarray(clips).reshape(-1)[k])
            if clips is not None and not 0 <= which < B:
                raise ValueError(f"JointGuide.keyframes: clip {which} outside 0..{B - 1}")
            target[which, frames[k], joints[k]] = positions[k]
            weights[which, frames[k], joints[k]] = w[k]
        return th.from_numpy(target), th.from_numpy(weights)

    @staticmethod
    def root_path(shape, xz, weight=1.0, lengths=None):
        """(target, weight) [B,T,J,3] that ask the root (joint 0) to follow a floor path: xz [T,2] or [B,T,2], its x and z per frame;
        the height and every other joint stay unconstrained.  weight: a scalar, [T] or [B,T]; frames from lengths[b] on get 0."""
        B, T, J = (int(v) for v in shape)
        xz = np.asarray(xz, dtype=np.float32)
        if xz.shape not in ((T, 2), (B, T, 2)):
            raise ValueError(f"JointGuide.root_path: xz must be [{T}, 2] or [{B}, {T}, 2], got {xz.shape}")
        w = np.broadcast_to(np.asarray(weight, dtype=np.float32), (B, T)).copy()
        if (w < 0).any():
            raise ValueError("JointGuide.root_path: weight must be >= 0")
        if lengths is not None:
            n = np.asarray(lengths, dtype=np.int64).reshape(B)
            w[np.arange(T)[None, :] >= n[:, None]] = 0.0
        target, weights = np.zeros((B, T, J, 3), np.float32), np.zeros((B, T, J, 3), np.float32)
        target[:, :, 0, 0::2] = np.broadcast_to(xz, (B, T, 2))
        weights[:, :, 0, 0] = w
        weights[:, :, 0, 2] = w
        return th.from_numpy(target), th.from_numpy(weights)
