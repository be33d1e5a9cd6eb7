"""The joint-space likelihood of diffusion.guidance.JointGuide restated in torch, for the tests alone (the package has no torch-op
evaluation of it): `recover_from_ric` (reference data_loaders/humanml/scripts/motion_process.py:389-410, :444-461) out of place, the
likelihood  logp[b] = -1/2 scale[b] sum_{t < len_b, j, c} w (p - y)^2  and its gradient with respect to the normalised rows by
torch.autograd, in whatever dtype the inputs carry.  float64: the yardstick (pinned to the reference's own functions by
tests/golden/joint_guide.npz); float32 on the CPU: what the reference's arithmetic gives, the measure of the GPU test's bar.

Inputs are seeded (mst_amd.synthetic): rows ~ N(0, 1), std in [0.05, 0.5], mean in [-0.2, 0.2] -- the yaw angle of a 257-frame clip
then wanders a few radians, the root a few units -- targets ~ N(0, 1), weights in [0, 1) by pattern, scale in [0.5, 2)."""
import os

import numpy as np
import torch

from mst_amd import synthetic as syn

SEED = 20261020
PATTERNS = ("dense", "root_xz", "late_joint", "zero")
# (J, F): two joints in the smallest row that holds them, the 9 J + 1 position-rotation row at 21 joints, the HumanML row at 22
SKELETONS = ((2, 7), (21, 190), (22, 263))
FRAMES = (1, 2, 63, 64, 65, 196, 257)
GOLDEN_CASES = ((2, 7, 5, 1, "dense"), (21, 190, 9, 3, "dense"), (22, 263, 12, 3, "root_xz"), (22, 263, 7, 3, "late_joint"))


def lengths_of(T, B):
    return [T, 1, (T + 1) // 2][:B]


def qrot(q, v):
    """quaternion.py:88-99 (the reference's qrot), out of place."""
    qvec = q[..., 1:]
    uv = torch.cross(qvec, v, dim=-1)
    uuv = torch.cross(qvec, uv, dim=-1)
    return v + 2 * (q[..., :1] * uv + uuv)


def recover_from_ric(data, J):
    """data [..., T, F] denormalised -> [..., T, J, 3]; the reference's statements in its order, without the in-place writes."""
    rot_vel = data[..., 0]
    ang = torch.cumsum(torch.cat([torch.zeros_like(rot_vel[..., :1]), rot_vel[..., :-1]], dim=-1), dim=-1)
    zero = torch.zeros_like(ang)
    quat = torch.stack([torch.cos(ang), zero, torch.sin(ang), zero], dim=-1)
    vel = torch.cat([torch.zeros_like(data[..., :1, 1:3]), data[..., :-1, 1:3]], dim=-2)
    r_pos = torch.stack([vel[..., 0], zero, vel[..., 1]], dim=-1)
    r_pos = torch.cumsum(qrot(quat, r_pos), dim=-2)
    r_pos = torch.stack([r_pos[..., 0], data[..., 3], r_pos[..., 2]], dim=-1)
    local = data[..., 4:4 + 3 * (J - 1)]
    local = local.reshape(local.shape[:-1] + (J - 1, 3))
    pos = qrot(quat[..., None, :].expand(local.shape[:-1] + (4,)), local)
    pos = torch.stack([pos[..., 0] + r_pos[..., 0:1], pos[..., 1], pos[..., 2] + r_pos[..., 2:3]], dim=-1)
    return torch.cat([r_pos.unsqueeze(-2), pos], dim=-2)


def positions(x0, mean, std, J):
    """x0 [B,F,1,T] normalised -> [B,T,J,3]."""
    rows = x0[:, :, 0, :].permute(0, 2, 1) * std + mean
    return recover_from_ric(rows, J)


def log_prob(x0, mean, std, J, target, weight, scale, lengths=None):
    """(logp [B], positions [B,T,J,3]); differentiable in x0."""
    p = positions(x0, mean, std, J)
    B, T = p.shape[:2]
    w = weight
    if lengths is not None:
        live = (torch.arange(T, device=p.device)[None, :] < torch.as_tensor(lengths).to(p.device).reshape(B, 1)).to(p.dtype)
        w = w * live[:, :, None, None]
    return -0.5 * scale.reshape(B) * (w * (p - target) ** 2).sum(dim=(1, 2, 3)), p


def make_case(J, F, T, B, pattern, seed=SEED):
    """dict of float32 numpy inputs of one seeded case."""
    tag = f"jg/{J}/{F}/{T}/{B}"
    lengths = lengths_of(T, B)
    w = np.zeros((B, T, J, 3), np.float32)
    full = syn.uniform(seed, tag + "/w", (B, T, J, 3), 0.0, 1.0)
    if pattern == "dense":
        w = full
    elif pattern == "root_xz":
        w[:, :, 0, 0::2] = full[:, :, 0, 0::2]
    elif pattern == "late_joint":                      # one joint, in the last valid frame of every clip
        for b, n in enumerate(lengths):
            w[b, n - 1, J - 1] = 0.5 + 0.5 * full[b, n - 1, J - 1]
    else:
        assert pattern == "zero", pattern
    return dict(x0=syn.normal(seed, tag + "/x0", (B, F, 1, T)), mean=syn.uniform(seed, tag + "/mean", (F,), -0.2, 0.2),
                std=syn.uniform(seed, tag + "/std", (F,), 0.05, 0.5), target=syn.normal(seed, tag + "/y", (B, T, J, 3)), weight=w,
                scale=syn.uniform(seed, tag + "/scale", (B,), 0.5, 2.0), lengths=np.asarray(lengths, np.int32), J=J)


def evaluate(case, dtype, lengths="case"):
    """The fixture on the CPU in `dtype`: dict(logp [B], grad [B,F,1,T], pos [B,T,J,3]) as numpy arrays of that dtype."""
    t = {k: torch.from_numpy(np.asarray(case[k])).to(dtype) for k in ("x0", "mean", "std", "target", "weight", "scale")}
    x0 = t["x0"].clone().requires_grad_()
    n = case["lengths"] if isinstance(lengths, str) else lengths
    logp, pos = log_prob(x0, t["mean"], t["std"], case["J"], t["target"], t["weight"], t["scale"], n)
    grad, = torch.autograd.grad(logp.sum(), x0)
    return dict(logp=logp.detach().numpy(), grad=grad.numpy(), pos=pos.detach().numpy())


def distance(a, b):
    """max |a - b| over the largest magnitude of b (1 where b is all zero: the distance is then absolute)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = float(np.abs(b).max()) if b.size else 0.0
    return float(np.abs(a - b).max()) / (scale if scale > 0 else 1.0) if b.size else 0.0


def golden():
    from conftest import GOLDEN
    return np.load(os.path.join(GOLDEN, "joint_guide.npz"))
