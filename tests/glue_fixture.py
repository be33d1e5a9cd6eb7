"""Float64 numpy closed forms of the glue around the transformer kernels, and the fp32 torch-op formulas they are measured against.

What each closed form restates (the reference lines are the ones csrc/mst_elem.h cites beside the kernel):
  masked_l2(a, b, mask)          gaussian_diffusion.py:223-235      sum_{f,t} (a - b)^2 mask[t] / (sum_t mask[t] * F) per sample
  text_cosine(f, m)              gaussian_diffusion.py:1384-1388    mean_b (1 - <f_b, m_b> / (|f_b| |m_b|))
  step_d_out(...)                inpainting_gaussian_diffusion.py:66-123, :179-239 -- both outputs of the with-grad step are affine in
                                 the model output: pred = out (1 - mask) + motion mask (clamped to [-1, 1] under clip_denoised),
                                 sample = c1 pred + c2 x + ... (ancestral) or sqrt(abar_prev) pred + dir (srac x - pred) / srm1ac + ...
  recover_from_ric(...)          motion_process.py:389-410, :444-461 with the yaw rotation of quaternion.py:88-99 written out

Everything is evaluated in float64 from the float32 INPUTS (and the float64 schedule tables): the closed forms carry no fp32 rounding of
their own, so the distance of an fp32 evaluation from them is that evaluation's error.  `bar()` is the rule the GPU tests hold the kernels
to: four times the distance of the reference's own fp32 torch formula on the same inputs, and not below 1e-6."""
import numpy as np
import torch

FLOOR = 1e-6


def f64(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def rel(a, b):
    a, b = f64(a), f64(b)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def bar(ref_deviation):
    """4 x what the reference's fp32 formula is off by (two fp32 evaluations differ in summation order), floor 1e-6."""
    return max(4.0 * float(ref_deviation), FLOOR)


# ------------------------------------------------------------------------------------------ masked_l2
def masked_l2(a, b, mask):
    """a [n or 1, F, 1, T], b [n, F, 1, T], mask [n or 1, 1, 1, T] -> loss [n]."""
    a, b, mask = f64(a), f64(b), f64(mask)
    n, F = b.shape[0], b.shape[1] * b.shape[2]
    a, mask = np.broadcast_to(a, b.shape), np.broadcast_to(mask, (n, 1, 1, b.shape[3]))
    return ((a - b) ** 2 * mask).reshape(n, -1).sum(1) / (mask.reshape(n, -1).sum(1) * F)


def masked_l2_grad_b(a, b, mask, g):
    """d (sum_n g[n] loss[n]) / d b; the gradient to a per-sample `a` is its negative."""
    a, b, mask, g = f64(a), f64(b), f64(mask), f64(g)
    n, F = b.shape[0], b.shape[1] * b.shape[2]
    a, mask = np.broadcast_to(a, b.shape), np.broadcast_to(mask, (n, 1, 1, b.shape[3]))
    k = g / (mask.reshape(n, -1).sum(1) * F)
    return -2.0 * (a - b) * mask * k.reshape(n, 1, 1, 1)


def masked_l2_torch(a, b, mask):
    """The reference's formula, torch ops in fp32 (as tests/test_gpu_fused_ops.py writes it)."""
    F = b.shape[1] * b.shape[2]
    return (((a - b) ** 2) * mask.float()).flatten(1).sum(1) / (mask.float().flatten(1).sum(1) * F)


# ------------------------------------------------------------------------------------------ text cosine
def text_cosine(f, m):
    f, m = f64(f), f64(m)
    c = (f * m).sum(1) / (np.linalg.norm(f, axis=1) * np.linalg.norm(m, axis=1))
    return float((1.0 - c).mean())


def text_cosine_grad_m(f, m, g=1.0):
    f, m = f64(f), f64(m)
    nf, nm = np.linalg.norm(f, axis=1, keepdims=True), np.linalg.norm(m, axis=1, keepdims=True)
    c = (f * m).sum(1, keepdims=True) / (nf * nm)
    return -(float(g) / f.shape[0]) * (f / (nf * nm) - c * m / nm ** 2)


def text_cosine_torch(f, m):
    fn = f / f.norm(dim=-1, keepdim=True)
    mn = m / m.norm(dim=-1, keepdim=True)
    return (1 - torch.nn.functional.cosine_similarity(fn, mn, dim=1, eps=1e-6)).mean()


# ------------------------------------------------------------------------------------------ the with-grad step
def step_dsdp(tab, t, ddim, eta):
    """d sample / d pred per clip, float64 tables."""
    t = np.asarray(t, dtype=np.int64)
    if not ddim:
        return tab["posterior_mean_coef1"][t]
    ab, abp = tab["alphas_cumprod"][t], tab["alphas_cumprod_prev"][t]
    sigma = eta * np.sqrt((1 - abp) / (1 - ab)) * np.sqrt(1 - ab / abp)
    return np.sqrt(abp) - np.sqrt(1 - abp - sigma ** 2) / tab["sqrt_recipm1_alphas_cumprod"][t]


def step_d_out(tab, t, ddim, eta, g_sample, g_pred, mask=None, pred_clipped=None):
    """d L / d model_output given d L / d sample and d L / d pred (either may be None).  mask: the inpainting mask of a blend (None:
    no blend).  pred_clipped: the forward's clamped x0-hat under clip_denoised -- an element at +-1 passes no gradient."""
    ref = g_pred if g_pred is not None else g_sample
    g = np.zeros(ref.shape, np.float64) if g_pred is None else f64(g_pred).copy()
    if g_sample is not None:
        g = g + f64(g_sample) * step_dsdp(tab, t, ddim, eta).reshape(-1, *([1] * (g.ndim - 1)))
    if mask is not None:
        g = g * (1.0 - f64(mask))
    if pred_clipped is not None:
        g = np.where(np.abs(f64(pred_clipped)) < 1.0, g, 0.0)
    return g


def step_torch(tab, t, ddim, eta, out, x, noise, mask, motion, clip, mask_noise=True, dtype=torch.float32):
    """(sample, pred) by the reference's torch ops, differentiable in `out`: fp32 tables as `_extract_into_tensor` casts them
    (gaussian_diffusion.py:1605-1618), or -- dtype float64, with float64 operands -- the same algebra without any fp32 rounding."""
    def ex(name):
        return torch.from_numpy(np.asarray(tab[name]))[t].to(dtype).view(-1, 1, 1, 1)
    pred = out if motion is None else out * (1 - mask) + motion * mask
    if clip:
        pred = pred.clamp(-1, 1)
    nz = noise * (1 - mask) if (mask is not None and mask_noise) else noise
    nonzero = (t != 0).float().view(-1, 1, 1, 1)
    if not ddim:
        mean = ex("posterior_mean_coef1") * pred + ex("posterior_mean_coef2") * x
        return mean + nonzero * torch.exp(0.5 * ex("posterior_log_variance_clipped")) * nz, pred
    eps = (ex("sqrt_recip_alphas_cumprod") * x - pred) / ex("sqrt_recipm1_alphas_cumprod")
    ab, abp = ex("alphas_cumprod"), ex("alphas_cumprod_prev")
    sigma = eta * torch.sqrt((1 - abp) / (1 - ab)) * torch.sqrt(1 - ab / abp)
    return pred * torch.sqrt(abp) + torch.sqrt(1 - abp - sigma ** 2) * eps + nonzero * sigma * nz, pred


# ------------------------------------------------------------------------------------------ recover_from_ric
def recover_joints(sample, mean, std, joints):
    """sample [B, F, 1, T] normalised hml_vec -> joint positions [B, 1, T, J, 3].
    yaw a_t = sum_{s<t} w_s (w = feature 0); root XZ_t = sum_{1<=s<=t} R(a_s) (vx, vz)_{s-1} (features 1, 2); root Y = feature 3;
    joint j >= 1 = R(a_t) (features 4 + 3 (j - 1) ...) + root XZ.  R(a) is the rotation by the unit quaternion-like (cos a, 0, sin a, 0)
    with the FULL angle: x' = x + 2 (c s z - s^2 x), z' = z - 2 (c s x + s^2 z)."""
    x = f64(sample)[:, :, 0, :].transpose(0, 2, 1) * f64(std) + f64(mean)              # [B, T, F]
    B, T, _ = x.shape
    ang = np.concatenate([np.zeros((B, 1)), np.cumsum(x[:, :-1, 0], axis=1)], axis=1)    # exclusive running sum
    c, s = np.cos(ang), np.sin(ang)

    def rot(vx, vz, c, s):
        return vx + 2.0 * (c * s * vz - s * s * vx), vz - 2.0 * (c * s * vx + s * s * vz)
    vx = np.concatenate([np.zeros((B, 1)), x[:, :-1, 1]], axis=1)
    vz = np.concatenate([np.zeros((B, 1)), x[:, :-1, 2]], axis=1)
    rx, rz = rot(vx, vz, c, s)
    px, pz = np.cumsum(rx, axis=1), np.cumsum(rz, axis=1)
    out = np.empty((B, 1, T, joints, 3))
    out[:, 0, :, 0, 0], out[:, 0, :, 0, 1], out[:, 0, :, 0, 2] = px, x[:, :, 3], pz
    loc = x[:, :, 4:4 + 3 * (joints - 1)].reshape(B, T, joints - 1, 3)
    jx, jz = rot(loc[..., 0], loc[..., 2], c[..., None], s[..., None])
    out[:, 0, :, 1:, 0], out[:, 0, :, 1:, 1], out[:, 0, :, 1:, 2] = jx + px[..., None], loc[..., 1], jz + pz[..., None]
    return out
