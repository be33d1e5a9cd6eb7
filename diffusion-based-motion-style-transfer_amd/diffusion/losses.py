"""Drop-in counterpart of the reference's `diffusion/losses.py` (:12-77): the three likelihood helpers `_vb_terms_bpd` and `_prior_bpd`
are written in, as plain torch functions on whatever device their arguments live.

They are the names a reference checkout imports.  `GaussianDiffusion.calc_bpd_loop` does not call them: its terms are one HIP launch
per row batch (csrc/mst_vb.h), which evaluates the decoder term in double because `cdf_plus - cdf_min` below cancels in float32."""
import math

import torch as th


def normal_kl(mean1, logvar1, mean2, logvar2):
    """KL(N(mean1, exp(logvar1)) || N(mean2, exp(logvar2))) per element, broadcasting; at least one argument is a tensor
    (reference :12-39)."""
    like = next((v for v in (mean1, logvar1, mean2, logvar2) if isinstance(v, th.Tensor)), None)
    assert like is not None, "at least one argument must be a Tensor"
    # th.exp needs tensors: scalars take the dtype and device of the first tensor argument
    logvar1, logvar2 = (v if isinstance(v, th.Tensor) else th.tensor(v).to(like) for v in (logvar1, logvar2))
    return 0.5 * (-1.0 + logvar2 - logvar1 + th.exp(logvar1 - logvar2) + ((mean1 - mean2) ** 2) * th.exp(-logvar2))


def approx_standard_normal_cdf(x):
    """The tanh approximation of the standard normal CDF (reference :42-47)."""
    return 0.5 * (1.0 + th.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * th.pow(x, 3))))


def discretized_gaussian_log_likelihood(x, *, means, log_scales):
    """log-probability (nats) of x under a Gaussian discretised to bins of width 2/255 on [-1, 1], open-ended beyond +-0.999
    (reference :50-77; an image-codebase leftover, reproduced as it is)."""
    assert x.shape == means.shape == log_scales.shape
    centered = x - means
    inv_stdv = th.exp(-log_scales)
    cdf_plus = approx_standard_normal_cdf(inv_stdv * (centered + 1.0 / 255.0))
    cdf_min = approx_standard_normal_cdf(inv_stdv * (centered - 1.0 / 255.0))
    log_cdf_plus = th.log(cdf_plus.clamp(min=1e-12))
    log_one_minus_cdf_min = th.log((1.0 - cdf_min).clamp(min=1e-12))
    log_delta = th.log((cdf_plus - cdf_min).clamp(min=1e-12))
    out = th.where(x < -0.999, log_cdf_plus, th.where(x > 0.999, log_one_minus_cdf_min, log_delta))
    assert out.shape == x.shape
    return out
