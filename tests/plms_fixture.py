"""The float64 statement of the PLMS step (reference diffusion/gaussian_diffusion.py:1084-1166, `plms_sample`) for the PLMS tests
(tests/test_plms_cpu.py, tests/test_gpu_plms.py): the oracle package stays as it is, so this lives here.

    eps   = (srac[t] x - pred) / srm1ac[t]                                  pred = x0-hat (blend / conversion / clip already applied)
    eps'  = sum_i COEF[cur_order][i] e_i,   e_0 = eps, e_1 .. the history NEWEST FIRST
    pred' = srac[t] x - srm1ac[t] eps'                                      (not clipped)
    mean  = pred' sqrt(abar_prev[t]) + sqrt(1 - abar_prev[t]) eps'
    sample = t != 0 ? mean : pred

and the two halves of the Pseudo Improved Euler step that opens a chain of order > 1:

    x_mid = pred sqrt(abar_prev[t]) + sqrt(1 - abar_prev[t]) eps            (from pred itself, not pred')
    eps2  = (srac[t-1] x_mid - pred2) / srm1ac[t-1],  eps' = (eps + eps2) / 2,  pred', mean as above with the tables at t and the ORIGINAL x.

The reference reads every table entry through `_extract_into_tensor(...).float()` (:1605-1618), i.e. ROUNDED TO FLOAT32; every function
here takes the float32-rounded entries and does all arithmetic behind them in float64, so what is left between it and the reference
(or the kernels) is fp32 operation rounding alone.

What an elementwise bar is relative to.  The sample is a sum of products that partly cancel (pred' = srac x - srm1ac eps' undoes most of
eps' = (srac x - pred) / srm1ac, and the order-4 coefficients sum to 160/24 in magnitude), and each product carries a few roundings of
2^-24 relative to ITSELF.  `scale` is therefore the sum of the magnitudes of every product the sample is built from:

    |eps|   <= (srac |x| + |pred|) / srm1ac                      =: E0
    |eps'|  <= sum_i |COEF_i| |e_i|  (E0 for i = 0)              =: EP
    scale    = sqrt(abar_prev) (srac |x| + srm1ac EP) + sqrt(1 - abar_prev) EP          (t != 0;  |pred| at t == 0)

Against this closed form the reference's own fp32 step stays within 2.6e-7 of `scale` (ddim20, "100" and the full schedule; indices
0, 1, 2, mid, n - 2, n - 1; orders 1-4), so the project's stand-alone-step bar 2e-5 (tests/test_gpu_parity.py) is the elementwise bar."""
import os

import numpy as np

import mst_amd.synthetic as syn
from conftest import GOLDEN, SEED
from oracle import schedule

PROMPT = "a person walks proudly"
SHAPES = {"xia": (181, 76), "hml": (263, 196)}
STRIDE = {"xia": 19, "hml": 49}                   # frames the golden keeps of a single step's outputs (make_golden_plms.py)
INDICES = {"": (0, 500, 999), "100": (0, 50, 99), "ddim20": (0, 10, 19)}
RESPACINGS = {"xia": ("", "100", "ddim20"), "hml": ("ddim20",)}
EULER_INDICES = (10, 19)
BAR_STEP = 2e-5                                   # tests/test_gpu_parity.py: the stand-alone step's constant, relative to `scale`

# eps' = sum COEF[cur_order][i] * e_i, e_0 this step's eps, e_1 the newest earlier one (reference :1147-1154)
COEF = {1: (1.0,), 2: (3 / 2, -1 / 2), 3: (23 / 12, -16 / 12, 5 / 12), 4: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}
# A_r = sum |COEF[r]|: by how much a per-step x0-hat error can reach eps' (the whole-loop bar of tests/test_gpu_plms.py)
A = {r: sum(abs(c) for c in COEF[r]) for r in COEF}

_TAB = {}


def tables(respacing):
    if respacing not in _TAB:
        _TAB[respacing] = schedule.make("cosine", 1000, respacing)
    return _TAB[respacing]


def _f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def _bc(v, like):
    return np.asarray(v, dtype=np.float64).reshape((-1,) + (1,) * (np.ndim(like) - 1))


def _entries(tab, t, like):
    """(srac, srm1ac, abar_prev) at index t per clip: float32-rounded entries, broadcast over a clip."""
    t = np.asarray(t).reshape(-1)
    return tuple(_bc(_f32(np.asarray(tab[k])[t]), like) for k in
                 ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "alphas_cumprod_prev"))


def eps_of(tab, pred, x, t):
    x = np.asarray(x, dtype=np.float64)
    srac, srm1, _ = _entries(tab, t, x)
    return (srac * x - np.asarray(pred, dtype=np.float64)) / srm1


def cur_order(order, held):
    """min(order, len(old_eps)) after this step's eps was appended to a history of `held` entries (reference :1146)."""
    return min(int(order), 1 + int(held))


def closed_form(tab, pred, x, t, hist=()):
    """(sample, scale, eps) in float64 of the multistep step with cur_order = 1 + len(hist); hist: the history NEWEST FIRST."""
    pred, x = np.asarray(pred, dtype=np.float64), np.asarray(x, dtype=np.float64)
    t = np.asarray(t).reshape(-1)
    c = COEF[1 + len(hist)]
    srac, srm1, abp = _entries(tab, t, x)
    eps = (srac * x - pred) / srm1
    es = [eps] + [np.asarray(h, dtype=np.float64) for h in hist]
    ep = sum(ci * ei for ci, ei in zip(c, es))
    pp = srac * x - srm1 * ep
    mean = pp * np.sqrt(abp) + np.sqrt(1.0 - abp) * ep
    nz = _bc(t != 0, x)
    E0 = (srac * np.abs(x) + np.abs(pred)) / srm1
    EP = sum(abs(ci) * ai for ci, ai in zip(c, [E0] + [np.abs(e) for e in es[1:]]))
    scale = np.sqrt(abp) * (srac * np.abs(x) + srm1 * EP) + np.sqrt(1.0 - abp) * EP
    return np.where(nz, mean, pred), np.where(nz, scale, np.abs(pred) + 1e-30), eps


def euler_first(tab, pred, x, t):
    """(x_mid, scale, eps): the first half of the Euler step, x_mid from pred ITSELF."""
    pred, x = np.asarray(pred, dtype=np.float64), np.asarray(x, dtype=np.float64)
    srac, srm1, abp = _entries(tab, t, x)
    eps = (srac * x - pred) / srm1
    x_mid = pred * np.sqrt(abp) + np.sqrt(1.0 - abp) * eps
    scale = np.sqrt(abp) * np.abs(pred) + np.sqrt(1.0 - abp) * (srac * np.abs(x) + np.abs(pred)) / srm1
    return x_mid, scale, eps


def euler_second(tab, pred2, x_mid, x, eps, t):
    """(sample, scale): the second half -- pred2 is x0-hat of the model at (x_mid, t - 1); tables at t - 1 for eps2, at t behind it."""
    pred2, x_mid, x, eps = (np.asarray(v, dtype=np.float64) for v in (pred2, x_mid, x, eps))
    t = np.asarray(t).reshape(-1)
    assert (t >= 1).all()
    srac, srm1, abp = _entries(tab, t, x)
    srac1, srm11, _ = _entries(tab, t - 1, x)
    eps2 = (srac1 * x_mid - pred2) / srm11
    ep = (eps + eps2) / 2
    pp = srac * x - srm1 * ep
    sample = pp * np.sqrt(abp) + np.sqrt(1.0 - abp) * ep
    EP = (np.abs(eps) + (srac1 * np.abs(x_mid) + np.abs(pred2)) / srm11) / 2
    return sample, np.sqrt(abp) * (srac * np.abs(x) + srm1 * EP) + np.sqrt(1.0 - abp) * EP


def euler_gain(tab, t, like):
    """d sample / d pred2 of the second half (the map is linear in pred2): (srm1ac[t] sqrt(abar_prev[t]) - sqrt(1 - abar_prev[t])) / (2 srm1ac[t - 1])."""
    t = np.asarray(t).reshape(-1)
    _, srm1, abp = _entries(tab, t, like)
    _, srm11, _ = _entries(tab, t - 1, like)
    return (srm1 * np.sqrt(abp) - np.sqrt(1.0 - abp)) / (2 * srm11)


def blend(out, mask, motion):
    """The inpainting blend on the raw model output (:341-349), in the input's precision."""
    return out * (1 - mask) + motion * mask


class HostSchedule:
    """`Schedule.plms_step` / `plms_euler` on the host, float64 behind float32 tensors: stands in for the device schedule so that the
    Python side of `plms_sample` (history bookkeeping, refusals, call order) runs without a GPU."""

    def __init__(self, tab):
        self.tab = tab
        self.calls = []

    def plms_step(self, model_output, x, t, history=(), order=None, mask=None, motion=None, clip_denoised=False, mean_type=0,
                  first_half=False, eps_out=None):
        import torch
        assert mean_type == 0
        out = model_output.double().numpy()
        if mask is not None:
            out = blend(out, mask.double().numpy(), motion.double().numpy())
        if clip_denoised:
            out = np.clip(out, -1, 1)
        tt = t.numpy()
        if first_half:
            s, _, eps = euler_first(self.tab, out, x.numpy(), tt)
            cur = 0
        else:
            cur = 1 + len(history) if order is None else cur_order(order, len(history))
            hist = [h.double().numpy() for h in list(history)[::-1][:cur - 1]]
            s, _, eps = closed_form(self.tab, out, x.numpy(), tt, hist)
        self.calls.append(("step", cur, int(tt[0])))
        f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
        return f(s), f(out), f(eps)

    def plms_euler(self, model_output, x_mid, x, eps, t, mask=None, motion=None, clip_denoised=False, mean_type=0):
        import torch
        out = model_output.double().numpy()
        if mask is not None:
            out = blend(out, mask.double().numpy(), motion.double().numpy())
        if clip_denoised:
            out = np.clip(out, -1, 1)
        s, _ = euler_second(self.tab, out, x_mid.numpy(), x.numpy(), eps.numpy(), t.numpy())
        self.calls.append(("euler", 0, int(t.numpy()[0])))
        return torch.from_numpy(s.astype(np.float32))


# ------------------------------------------------------------------------------ the golden's inputs, from their seeds
def golden():
    return np.load(os.path.join(GOLDEN, "plms.npz"))


def golden_inputs(tag):
    F, T = SHAPES[tag]
    shp = (1, F, 1, T)
    return dict(F=F, T=T, x=syn.normal(SEED, f"plms/{tag}/x", shp), mask=syn.root_horizontal_mask(1, F, T),
                motion=syn.normal(SEED, f"plms/{tag}/motion", shp), txt=syn.normal(SEED, "text/" + PROMPT, (1, 512)),
                hist=[syn.normal(SEED, f"plms/{tag}/h{k}", shp) for k in (1, 2, 3)])          # h1 newest .. h3 oldest


def golden_noise():
    F, T = SHAPES["xia"]
    return syn.normal(SEED, "plms/xia/noise", (1, F, 1, T))


def single_step_cases():
    return [(tag, resp, t, pair) for tag in SHAPES for resp in RESPACINGS[tag] for t in INDICES[resp] for pair in (0, 1)]


def euler_cases():
    return [(tag, t, pair) for tag in SHAPES for t in EULER_INDICES for pair in (0, 1)]
