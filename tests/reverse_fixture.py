"""The float64 statement of the DDIM reverse step (reference diffusion/gaussian_diffusion.py:910-946, `ddim_reverse_sample`) for the
reverse tests (tests/test_reverse_cpu.py, tests/test_gpu_reverse.py): the oracle package stays as it is, so this lives here.

    eps    = (sqrt_recip_alphas_cumprod[t] * x - pred) / sqrt_recipm1_alphas_cumprod[t]
    sample = pred * sqrt(acn) + sqrt(1 - acn) * eps,        acn = alphas_cumprod_next[t] = alphas_cumprod[t + 1], 0 at the last index

which is linear in both inputs: sample = a(t) * pred + b(t) * x.  The reference reads every table entry through
`_extract_into_tensor(...).float()` (:1605-1618), i.e. ROUNDED TO FLOAT32, and `1 - acn` is formed from the rounded entry: at the
first indices of the full schedule acn is within 1e-4 of 1, so that rounding moves sqrt(1 - acn) by up to 1.5e-4 relative -- it is
part of what the reference computes, not an arithmetic error.  `coefs` therefore takes the float32-rounded entries and does all
arithmetic behind them in float64; what is left between it and the reference (or the kernels) is fp32 operation rounding alone.

What an elementwise bar is relative to.  The step is evaluated as THREE products, not two:

    sample = sqrt(acn) pred  -  (sqrt(1 - acn) / srm1ac) pred  +  (sqrt(1 - acn) srac / srm1ac) x

and away from the ends of a schedule the two pred terms nearly cancel (full schedule, index 500: coefficients 0.70 and 0.70, a = 0.002).
Each product carries a few roundings of 2^-24 relative to ITSELF, in the reference's fp32 as in the kernels', so the rounding of the sum
is relative to the sum of the three magnitudes, `scale` = A |pred| + b |x| with A = sqrt(acn) + sqrt(1 - acn) / srm1ac >= |a|.  Relative
to |a pred| + |b x| alone, the reference's own fp32 output misses 1e-6 wherever x is near zero at such an index (measured here: 1.0e-5
at index 500 of the full schedule); relative to `scale` it holds 1e-6 everywhere.

`g(t)` = |a(t)| is the factor by which an error in x0-hat reaches the sample (exact: the map is linear in x0-hat); it comes from the
unrounded float64 tables, as a property of the schedule."""
import os

import numpy as np

import mst_amd.synthetic as syn
from conftest import GOLDEN, SEED
from oracle import schedule

PROMPT = "a person walks proudly"
SHAPES = {"xia": (181, 76), "hml": (263, 196)}
STRIDE = {"xia": 7, "hml": 17}                    # frames the golden keeps of a single step's outputs (make_golden_reverse.py)
INDICES = {"": (0, 500, 999), "100": (0, 50, 99), "ddim20": (0, 10, 19)}
RESPACINGS = {"xia": ("", "100", "ddim20"), "hml": ("ddim20",)}

_TAB = {}


def tables(respacing):
    if respacing not in _TAB:
        _TAB[respacing] = schedule.make("cosine", 1000, respacing)
    return _TAB[respacing]


def acn_of(tab, t):
    """alphas_cumprod_next[t] WITHOUT the table of that name: alphas_cumprod[t + 1], exactly 0 at the last index (:193)."""
    ac = np.asarray(tab["alphas_cumprod"], dtype=np.float64)
    t = np.asarray(t)
    return np.where(t + 1 < len(ac), ac[np.minimum(t + 1, len(ac) - 1)], 0.0)


def _f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def coefs(tab, t):
    """(a, b) per clip, float64 [B]: sample = a * pred + b * x.  Table entries as float32 (the reference's `.float()`), arithmetic in float64."""
    t = np.asarray(t).reshape(-1)
    srac = _f32(np.asarray(tab["sqrt_recip_alphas_cumprod"])[t])
    srm1 = _f32(np.asarray(tab["sqrt_recipm1_alphas_cumprod"])[t])
    acn = _f32(acn_of(tab, t))
    s1 = np.sqrt(1.0 - acn)
    return np.sqrt(acn) - s1 / srm1, s1 * srac / srm1


def _bc(v, like):
    return np.asarray(v, dtype=np.float64).reshape((-1,) + (1,) * (np.ndim(like) - 1))


def closed_form(tab, pred, x, t):
    """(sample, scale) in float64: the reverse step from x0-hat and x in the reference's operation order, and A |pred| + b |x|, the
    magnitudes of the three products whose (partly cancelling) sum the sample is -- what an elementwise bar is relative to (see above)."""
    pred, x = np.asarray(pred, dtype=np.float64), np.asarray(x, dtype=np.float64)
    t = np.asarray(t).reshape(-1)
    srac = _bc(_f32(np.asarray(tab["sqrt_recip_alphas_cumprod"])[t]), x)
    srm1 = _bc(_f32(np.asarray(tab["sqrt_recipm1_alphas_cumprod"])[t]), x)
    acn = _bc(_f32(acn_of(tab, t)), x)
    eps = (srac * x - pred) / srm1
    sample = pred * np.sqrt(acn) + np.sqrt(1.0 - acn) * eps
    A, b = np.sqrt(acn) + np.sqrt(1.0 - acn) / srm1, np.sqrt(1.0 - acn) * srac / srm1
    return sample, A * np.abs(pred) + b * np.abs(x)


def eps_of(tab, pred, x, t):
    x = np.asarray(x, dtype=np.float64)
    t = np.asarray(t).reshape(-1)
    srac = _bc(_f32(np.asarray(tab["sqrt_recip_alphas_cumprod"])[t]), x)
    srm1 = _bc(_f32(np.asarray(tab["sqrt_recipm1_alphas_cumprod"])[t]), x)
    return (srac * x - np.asarray(pred, dtype=np.float64)) / srm1


def g(tab, t):
    """|sqrt(acn) - sqrt(1 - acn) sqrt(ac) / sqrt(1 - ac)| from the float64 tables."""
    ac = np.asarray(tab["alphas_cumprod"], dtype=np.float64)[t]
    acn = acn_of(tab, t)
    return np.abs(np.sqrt(acn) - np.sqrt(1.0 - acn) * np.sqrt(ac) / np.sqrt(1.0 - ac))


def blend(out, mask, motion):
    """The inpainting blend on the raw model output (:341-349), in the input's precision."""
    return out * (1 - mask) + motion * mask


def reverse_loop(forward, tab, tmap, x, t0, n, mask=None, motion=None):
    """Ascending loop over an fp32 model `forward(x, original timesteps) -> x0-hat` (oracle.denoiser.forward behind a lambda): indices
    t0 .. t0 + n - 1.  Returns (x at index t0 + n, [x0-hat per step], [x per step: the step's INPUT]) as float32 arrays."""
    import torch
    x = np.asarray(x, dtype=np.float32)
    preds, xs = [], []
    for t in range(t0, t0 + n):
        tt = np.full((x.shape[0],), t)
        out = np.asarray(forward(torch.from_numpy(x), torch.from_numpy(np.asarray(tmap)[tt])), dtype=np.float32)
        if mask is not None:
            out = blend(out, mask, motion).astype(np.float32)
        xs.append(x)
        preds.append(out)
        x = closed_form(tab, out, x, tt)[0].astype(np.float32)
    return x, preds, xs


# ------------------------------------------------------------------------------ the golden's inputs, from their seeds
def golden():
    return np.load(os.path.join(GOLDEN, "reverse.npz"))


def golden_inputs(tag):
    F, T = SHAPES[tag]
    shp = (1, F, 1, T)
    return dict(F=F, T=T, x=syn.normal(SEED, f"rev/{tag}/x", shp), mask=syn.root_horizontal_mask(1, F, T),
                motion=syn.normal(SEED, f"rev/{tag}/motion", shp), txt=syn.normal(SEED, "text/" + PROMPT, (1, 512)))


def golden_content():
    F, T = SHAPES["xia"]
    return syn.normal(SEED, "rev/xia/content", (1, F, 1, T))


def single_step_cases():
    return [(tag, resp, t, pair) for tag in SHAPES for resp in RESPACINGS[tag] for t in INDICES[resp] for pair in (0, 1)]
