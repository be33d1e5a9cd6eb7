"""Guides for the `cond_fn` argument of p_sample / ddim_sample and their loops (reference gaussian_diffusion.py:454-506).

A cond_fn returns grad log p(y | x_t).  Any callable works: the samplers evaluate it on x_t in front of each step and hand the
tensor to the step kernel (MST_GUIDE_GRADIENT, one step per engine call).  A `TargetGuide` is the one guide the step kernel
computes itself (MST_GUIDE_TARGET): its operands are constant over the loop, so a guided loop stays one native call."""
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
