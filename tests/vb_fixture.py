"""The float64 statement of the variational-bound evaluation (reference diffusion/gaussian_diffusion.py:1281-1314 `_vb_terms_bpd`,
:1529-1545 `_prior_bpd`, :1586-1588 the loop's two MSEs; diffusion/losses.py:12-77) for tests/test_vb_cpu.py and tests/test_gpu_vb.py:
the oracle package stays as it is, so this lives here.

A ROW is one (clip, timestep) pair; every function takes operands already gathered to rows ([R, ...]) and returns [R, 4] =
(vb term in bits, mean (x0hat - x0)^2, mean (eps - z)^2, rms x0hat):

    out'  = out (1 - m) + motion m                     the inpainting blend on the RAW output (:341-349)
    x0hat = out' | srac x_t - srm1ac out' | out' / c1 - (c2 / c1) x_t        by mean type 0 | 1 | 2 (:398-412), then clamp(-1, 1)
    eps   = (srac x_t - x0hat) / srm1ac
    t != 0:  vb = mean(normal_kl(true_mean, true_logvar, model_mean, model_logvar)) / ln 2
             true_mean - model_mean = c1 (x0 - x0hat) for mean types 0 and 1 (the c2 x_t terms cancel exactly);
             model_mean = out' for mean type 2
    t == 0:  vb = mean(-discretized_gaussian_log_likelihood(x0, means = model_mean, log_scales = model_logvar / 2)) / ln 2

The reference reads every table entry through `_extract_into_tensor(...).float()` (:1605-1618), ROUNDED TO FLOAT32; `terms64` takes the
float32-rounded entries and does all arithmetic behind them in float64 (as tests/plms_fixture.py does, for the same reason).
`terms32` is the same in float32 torch ops IN THE REFERENCE'S OWN ORDER (it subtracts the two posterior means as the reference does):
the yardstick.  Its distance from `terms64` is what the reference's own precision is, and the kernel's bars derive from it.

THE BARS (measured on the CPU by tests/test_vb_cpu.py::test_bars_are_the_fp32_restatements_distance, before any GPU run, over
`kernel_cases()` -- the very inputs tests/test_gpu_vb.py feeds the kernel; distance = |v32 - v64| / max(|v64|, DEN_FLOOR) per row).
d32 is taken PER per_clip CLASS (the table D32 below): a one-element row has nothing to average a rounding out, a 13756-element row
does, and one bar for both would let a large row's error of several per cent pass.  The rows that give the largest figures:

    vb  (t != 0) 4.30e-2   per_clip 1, full schedule, t = 999, FIXED_LARGE: -1 + lv2 - lv1 + exp(lv1 - lv2) cancels to 1.4e-7 bits in fp32
                           (the same at mean type 2, where the reference's true_mean - model_mean cancels at coef1 = 5e-5);
                           1.3e-6 at per_clip 13756 and 51548
    vb0 (t == 0) 2.91e-2   per_clip 256, full schedule, mean type 1: cdf_plus - cdf_min in fp32; 6.6e-3 at per_clip 13756
    xstart_mse   4.87e-4   per_clip 1, full schedule, mean type 2, t = 500: x0hat = out / c1 - (c2 / c1) x_t cancels; 1.3e-7 at 13756
    mse          2.07e-3   per_clip 1, full schedule, mean type 1, t = 999: eps - z cancels to 2e-5; 1.5e-7 at 13756
    rms          2.37e-5   per_clip 1, as xstart_mse; 8e-8 at 13756
    prior        4.12e-5   per_clip 1, "ddim20": -1 - lv + exp(lv) + mean1^2 in fp32: terms of size 1 for a sum of 1e-3

    KERNEL BAR of a column at a per_clip = max(4 * D32[per_clip][column], 1e-6): the multiplier of the evaluator and joint-guide tests --
    the reference's own precision with headroom for another summation order.  The t == 0 rows have their own d32 ("vb0"): the
    kernel evaluates that branch in double, so it should sit far inside.

`HostSchedule` stands in for `Schedule.vb_diffuse / vb_terms / vb_prior` so that the Python loop runs without a GPU."""
import os

import numpy as np

import mst_amd.synthetic as syn
from conftest import GOLDEN, SEED
from oracle import schedule

LN2 = float(np.log(2.0))
# A distance is relative to the row's own value, with a floor under the denominator.  The vb column's floor is the resolution of the
# reference's own float32 expression: normal_kl adds terms of magnitude up to 1 + |logvar| <= 12 (-1, logvar2, logvar1, the exp), so
# one element's KL is resolved to about 12 * 2^-24 nats ~ 1e-6 bits whatever its size -- and at the last index of the full schedule
# coef1 ~ 5e-5 makes the whole term ~ 1e-9 bits.  The other three columns are means of squares of O(1) numbers: their floor only keeps
# a division finite.
DEN_FLOOR = np.array([1e-6, 1e-9, 1e-9, 1e-9])
BAR_FLOOR = 1e-6          # no bar below this, relative
COLS = ("vb", "xstart_mse", "mse", "rms")

# measured by test_bars_are_the_fp32_restatements_distance over kernel_cases(), per per_clip class (the worst row of every column;
# "vb" over rows with t != 0, "vb0" over rows with t == 0 -- per_clip 1 has none --, "prior" over every case's clips).  The test
# re-measures and fails if a value here is not what it finds, within a factor of two either way (another libm's exp and tanh move
# single elements of the small rows).
_D32_COLS = ("vb", "vb0", "xstart_mse", "mse", "rms", "prior")
D32 = {per: dict(zip(_D32_COLS, v)) for per, v in {
    1: (4.30e-2, 0.0, 4.87e-4, 2.07e-3, 2.37e-5, 4.12e-5),
    3: (2.52e-2, 2.57e-6, 3.14e-6, 8.86e-4, 3.96e-7, 2.09e-5),
    255: (3.17e-2, 1.21e-2, 4.05e-7, 2.63e-4, 1.13e-7, 9.11e-6),
    256: (4.55e-6, 2.91e-2, 2.34e-6, 2.28e-6, 8.65e-7, 7.64e-6),
    257: (3.10e-2, 2.11e-2, 3.22e-6, 1.90e-4, 3.80e-7, 7.74e-6),
    181 * 76: (1.34e-6, 6.57e-3, 1.33e-7, 1.46e-7, 7.98e-8, 7.52e-6),
    263 * 196: (1.45e-6, 5.57e-3, 9.53e-8, 1.34e-7, 5.13e-8, 7.55e-6)}.items()}

PROMPTS = ["a person walks proudly", "an old man jumps"]
F, T = 181, 76
LENGTHS = (76, 40)
STRIDE = 19
X_SCALE = 0.6
# case -> (respacing, sigma_small, clips, clip_denoised): tests/golden/make_golden_vb.py
CASES = {"ddim20|c1": ("ddim20", True, 2, True), "ddim20|c0": ("ddim20", True, 2, False), "full|c0": ("", True, 1, False),
         "large|c0": ("ddim20", False, 2, False)}

_TAB = {}


def tables(respacing):
    if respacing not in _TAB:
        _TAB[respacing] = schedule.make("cosine", 1000, respacing)
    return _TAB[respacing]


def model_logvar(tab, large):
    """The model's log-variance row (:368-379): posterior_log_variance_clipped, or under FIXED_LARGE log(append(pv[1], betas[1:]))."""
    if large:
        return np.log(np.append(tab["posterior_variance"][1], tab["betas"][1:]))
    return tab["posterior_log_variance_clipped"]


def model_variance(tab, large):
    return np.append(tab["posterior_variance"][1], tab["betas"][1:]) if large else tab["posterior_variance"]


def _f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def _bc(v, like):
    return np.asarray(v, dtype=np.float64).reshape((-1,) + (1,) * (np.ndim(like) - 1))


def _mean_flat(a):
    return a.reshape(a.shape[0], -1).mean(axis=1)


# ------------------------------------------------------------------------------ the three helpers, float64
def normal_kl(mean1, logvar1, mean2, logvar2):
    return 0.5 * (-1.0 + logvar2 - logvar1 + np.exp(logvar1 - logvar2) + (mean1 - mean2) ** 2 * np.exp(-logvar2))


def approx_standard_normal_cdf(x):
    return 0.5 * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))


def discretized_gaussian_log_likelihood(x, means, log_scales):
    centered = x - means
    inv_stdv = np.exp(-log_scales)
    cdf_plus = approx_standard_normal_cdf(inv_stdv * (centered + 1.0 / 255.0))
    cdf_min = approx_standard_normal_cdf(inv_stdv * (centered - 1.0 / 255.0))
    return np.where(x < -0.999, np.log(np.maximum(cdf_plus, 1e-12)),
                    np.where(x > 0.999, np.log(np.maximum(1.0 - cdf_min, 1e-12)), np.log(np.maximum(cdf_plus - cdf_min, 1e-12))))


# ------------------------------------------------------------------------------ the terms, float64
def xstart64(tab, out, x_t, t, mean_type=0, clip_denoised=True, mask=None, motion=None):
    """(x0hat, blended raw output) in float64 behind float32-rounded entries."""
    out, x_t = np.asarray(out, np.float64), np.asarray(x_t, np.float64)
    t = np.asarray(t).reshape(-1)
    if mask is not None:
        out = out * (1 - np.asarray(mask, np.float64)) + np.asarray(motion, np.float64) * mask
    raw = out
    e = lambda k: _bc(_f32(np.asarray(tab[k])[t]), x_t)
    if mean_type == 1:
        out = e("sqrt_recip_alphas_cumprod") * x_t - e("sqrt_recipm1_alphas_cumprod") * out
    if mean_type == 2:
        c1, c2 = e("posterior_mean_coef1"), e("posterior_mean_coef2")
        out = (1.0 / c1) * out - (c2 / c1) * x_t
    return (np.clip(out, -1, 1) if clip_denoised else out), raw


def terms64(tab, x0, x_t, out, z, t, mean_type=0, clip_denoised=True, mask=None, motion=None, large=False, pred=None):
    """[R, 4] float64.  pred: x0-hat given (the golden's own pred_xstart) instead of derived from `out`."""
    x0, x_t, z = (np.asarray(v, np.float64) for v in (x0, x_t, z))
    t = np.asarray(t).reshape(-1)
    if pred is None:
        pred, raw = xstart64(tab, out, x_t, t, mean_type, clip_denoised, mask, motion)
    else:
        assert mean_type != 2
        pred, raw = np.asarray(pred, np.float64), None
    e = lambda k: _bc(_f32(np.asarray(tab[k])[t]), x_t)
    c1, c2 = e("posterior_mean_coef1"), e("posterior_mean_coef2")
    lv1 = _bc(_f32(tab["posterior_log_variance_clipped"][t]), x_t)
    lv2 = _bc(_f32(model_logvar(tab, large)[t]), x_t)
    if mean_type == 2:
        model_mean = raw
        dm = (c1 * x0 + c2 * x_t) - raw
    else:
        model_mean = c1 * pred + c2 * x_t
        dm = c1 * (x0 - pred)
    kl = _mean_flat(normal_kl(dm, lv1, 0.0, lv2) + 0 * x_t) / LN2
    nll = _mean_flat(-discretized_gaussian_log_likelihood(x0, model_mean, 0.5 * lv2 + 0 * x_t)) / LN2
    eps = (e("sqrt_recip_alphas_cumprod") * x_t - pred) / e("sqrt_recipm1_alphas_cumprod")
    return np.stack([np.where(t == 0, nll, kl), _mean_flat((pred - x0) ** 2), _mean_flat((eps - z) ** 2),
                     np.sqrt(_mean_flat(pred ** 2))], axis=1)


def prior64(tab, x0):
    x0 = np.asarray(x0, np.float64)
    a, lv = _f32(tab["sqrt_alphas_cumprod"][-1]), _f32(tab["log_one_minus_alphas_cumprod"][-1])
    return _mean_flat(normal_kl(a * x0, lv, 0.0, 0.0)) / LN2


# ------------------------------------------------------------------------------ the same in float32 torch ops, the reference's order
def terms32(tab, x0, x_t, out, z, t, mean_type=0, clip_denoised=True, mask=None, motion=None, large=False):
    """[R, 4] float32 numpy: `_vb_terms_bpd` + the loop's MSEs as the reference writes them (p_mean_variance :341-412,
    q_posterior_mean_variance :287-309, losses.py), on float32 tensors."""
    import torch as th
    f = lambda a: th.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32)))
    x0, x_t, out, z = f(x0), f(x_t), f(out), f(z)
    tt = th.from_numpy(np.asarray(t).reshape(-1).astype(np.int64))
    ex = lambda arr: th.from_numpy(np.asarray(arr, np.float64))[tt].float().view(-1, *([1] * (x_t.dim() - 1))).expand(x_t.shape)
    if mask is not None:
        m = th.ones_like(f(mask)) * f(mask)
        out = (out * (1 - m)) + (f(motion) * m)
    c1, c2 = ex(tab["posterior_mean_coef1"]), ex(tab["posterior_mean_coef2"])
    proc = (lambda v: v.clamp(-1, 1)) if clip_denoised else (lambda v: v)
    if mean_type == 2:
        pred = proc(ex(1.0 / tab["posterior_mean_coef1"]) * out - ex(tab["posterior_mean_coef2"] / tab["posterior_mean_coef1"]) * x_t)
        model_mean = out
    else:
        if mean_type == 1:
            out = ex(tab["sqrt_recip_alphas_cumprod"]) * x_t - ex(tab["sqrt_recipm1_alphas_cumprod"]) * out
        pred = proc(out)
        model_mean = c1 * pred + c2 * x_t
    true_mean = c1 * x0 + c2 * x_t
    lv1, lv2 = ex(tab["posterior_log_variance_clipped"]), ex(model_logvar(tab, large))
    mf = lambda a: a.mean(dim=list(range(1, a.dim())))
    kl = 0.5 * (-1.0 + lv2 - lv1 + th.exp(lv1 - lv2) + ((true_mean - model_mean) ** 2) * th.exp(-lv2))
    kl = mf(kl) / np.log(2.0)
    ls = 0.5 * lv2
    centered = x0 - model_mean
    inv = th.exp(-ls)
    cdf = lambda v: 0.5 * (1.0 + th.tanh(np.sqrt(2.0 / np.pi) * (v + 0.044715 * th.pow(v, 3))))
    cp, cm = cdf(inv * (centered + 1.0 / 255.0)), cdf(inv * (centered - 1.0 / 255.0))
    lp = th.where(x0 < -0.999, th.log(cp.clamp(min=1e-12)),
                  th.where(x0 > 0.999, th.log((1.0 - cm).clamp(min=1e-12)), th.log((cp - cm).clamp(min=1e-12))))
    nll = mf(-lp) / np.log(2.0)
    vb = th.where(tt == 0, nll, kl)
    eps = (ex(tab["sqrt_recip_alphas_cumprod"]) * x_t - pred) / ex(tab["sqrt_recipm1_alphas_cumprod"])
    return th.stack([vb, mf((pred - x0) ** 2), mf((eps - z) ** 2), mf(pred ** 2).sqrt()], dim=1).numpy()


def prior32(tab, x0):
    import torch as th
    x0 = th.from_numpy(np.ascontiguousarray(np.asarray(x0, np.float32)))
    a = float(np.float32(tab["sqrt_alphas_cumprod"][-1]))
    lv = th.tensor(float(np.float32(tab["log_one_minus_alphas_cumprod"][-1])))
    kl = 0.5 * (-1.0 + 0.0 - lv + th.exp(lv - 0.0) + ((a * x0 - 0.0) ** 2) * 1.0)
    return (kl.mean(dim=list(range(1, x0.dim()))) / np.log(2.0)).numpy()


def distance(got, want):
    """|got - want| / max(|want|, DEN_FLOOR) per row and column ([R, 4]; [R]: the vb column's floor, for the prior)."""
    want = np.asarray(want, np.float64)
    return np.abs(np.asarray(got, np.float64) - want) / np.maximum(np.abs(want), DEN_FLOOR if want.ndim == 2 else DEN_FLOOR[0])


def bar(col, per=F * T):
    """The kernel's bar for a column of COLS (or "vb0", "prior") at rows of `per` elements (default: the golden's Xia clips): 4 x the
    fp32 restatement's distance in that per_clip class, at least BAR_FLOOR."""
    return max(4.0 * D32[per][col], BAR_FLOOR)


def row_bars(t, per):
    """[R, 4] bars for rows of `per` elements with timestep indices t: the vb column takes "vb0" where t == 0."""
    t = np.asarray(t).reshape(-1)
    b = np.tile(np.array([bar(c, per) for c in COLS]), (t.size, 1))
    b[t == 0, 0] = bar("vb0", per)
    return b


# ------------------------------------------------------------------------------ the kernel test's cases (CPU: the bars; GPU: the kernel)
SHAPES = {1: (1, 1), 3: (1, 3), 255: (5, 51), 256: (16, 16), 257: (257, 1), 181 * 76: (181, 76), 263 * 196: (263, 196)}


def kernel_cases():
    """(id, per_clip, R, respacing, mean_type, clip_denoised, pair, large, draw).  The small sizes take the full cross product of the
    switches at R = 3; R = 1 and R = 65 and the two clip sizes take a covering handful each (every switch both ways)."""
    cases = []
    for per in (1, 3, 255, 256, 257):
        for resp in ("", "ddim20"):
            for mean in (0, 1, 2):
                for clip in (0, 1):
                    for pair in ((0, 1) if mean == 0 else (0,)):      # the reference asserts START_X with the pair (:343)
                        for large in (0, 1):
                            for draw in (0, 1):
                                cases.append((per, 3, resp, mean, clip, pair, large, draw))
    for per in (255, 257):
        for R in (1, 65):
            cases += [(per, R, "", 0, 1, 1, 0, 0), (per, R, "ddim20", 1, 0, 0, 1, 1), (per, R, "ddim20", 2, 1, 0, 0, 1)]
    for per in (181 * 76, 263 * 196):
        cases += [(per, 3, "ddim20", 0, 1, 1, 0, 1), (per, 3, "", 0, 0, 0, 1, 0), (per, 1, "", 1, 1, 0, 0, 1), (per, 3, "ddim20", 2, 0, 0, 1, 0)]
    cases.append((181 * 76, 65, "ddim20", 0, 1, 0, 0, 1))
    return [("-".join(str(v) if v != "" else "full" for v in c),) + c for c in cases]


def case_rows(R, nsteps, per):
    """(clip, t) of a case's rows over N = min(R, 3) clips: t cycles through 0, 1, an interior index and the last (starting where the
    size says, so that the three-row cases between them meet all four); clips cycle out of order."""
    pool = [0, 1, nsteps // 2, nsteps - 1]
    t = np.array([pool[(r + per) % 4] for r in range(R)], dtype=np.int64)
    clip = np.array([(r * 2 + 1) % min(R, 3) for r in range(R)], dtype=np.int64)
    return clip, t


def case_inputs(case, z_of=None):
    """Per-clip x0 / mask / motion [N, F, 1, T] and per-row model output / noise [R, F, 1, T] of a kernel case, from seeds; x_t is the
    float32 q_sample of them (unmasked: what x_t is does not matter to the terms).  z_of(clip, t, F, T, seed): the counter draw's
    noise for draw cases (the GPU test passes the engine's `philox_normal`); None: seeded normals stand in (the CPU measurement)."""
    cid, per, R, resp, mean, clip_d, pair, large, draw = case
    Fc, Tc = SHAPES[per]
    tab, _ = tables(resp)
    n = len(tab["betas"])
    clip, t = case_rows(R, n, per)
    N = min(R, 3)
    x0 = (X_SCALE * syn.normal(SEED, f"vbk/{per}/x0", (N, Fc, 1, Tc))).astype(np.float32)
    out = syn.normal(SEED, f"vbk/{per}/{R}/out", (R, Fc, 1, Tc)).astype(np.float32)
    seed = 1000 + per % 997
    if draw and z_of is not None:
        z = np.stack([z_of(int(c), int(tt), Fc, Tc, seed, N) for c, tt in zip(clip, t)]).astype(np.float32)
    else:
        z = syn.normal(SEED, f"vbk/{per}/{R}/z", (R, Fc, 1, Tc)).astype(np.float32)
    a = np.asarray(tab["sqrt_alphas_cumprod"])[t].astype(np.float32).reshape(-1, 1, 1, 1)
    b = np.asarray(tab["sqrt_one_minus_alphas_cumprod"])[t].astype(np.float32).reshape(-1, 1, 1, 1)
    x_t = (a * x0[clip] + b * z).astype(np.float32)
    if mean == 2:                  # a previous-x model's output lives near the posterior mean, not near x0
        c1 = np.asarray(tab["posterior_mean_coef1"])[t].astype(np.float32).reshape(-1, 1, 1, 1)
        c2 = np.asarray(tab["posterior_mean_coef2"])[t].astype(np.float32).reshape(-1, 1, 1, 1)
        out = (c1 * (0.7 * out) + c2 * x_t).astype(np.float32)
    mask = motion = None
    if pair:
        mask = (syn.uniform(SEED, f"vbk/{per}/mask", (N, Fc, 1, Tc), 0.0, 1.0) < 0.3).astype(np.float32)
        motion = (X_SCALE * syn.normal(SEED, f"vbk/{per}/motion", (N, Fc, 1, Tc))).astype(np.float32)
    return dict(tab=tab, nsteps=n, clip=clip, t=t, N=N, F=Fc, T=Tc, x0=x0, out=out, z=z, x_t=x_t, mask=mask, motion=motion, seed=seed,
                mean=mean, clip_denoised=bool(clip_d), large=bool(large), draw=bool(draw))


def case_terms(v, fn):
    """`fn` (terms64 / terms32) on a case's gathered operands."""
    g = lambda a: None if a is None else a[v["clip"]]
    return fn(v["tab"], v["x0"][v["clip"]], v["x_t"], v["out"], v["z"], v["t"], mean_type=v["mean"], clip_denoised=v["clip_denoised"],
              mask=g(v["mask"]), motion=g(v["motion"]), large=v["large"])


# ------------------------------------------------------------------------------ host stand-in for the device schedule
class HostSchedule:
    """`Schedule.vb_diffuse / vb_terms / vb_prior` on the host, float64 behind float32 tensors, recording its calls: the Python side of
    `calc_bpd_loop` (row plan, kwargs gathering, noise indexing, reassembly) runs without a GPU.  A drawn noise is a seeded stand-in
    keyed by (seed, clip, t) alone, as the kernel's is."""

    def __init__(self, tab, large=False):
        self.tab, self.large, self.calls = tab, large, []

    @staticmethod
    def draw(seed, clip, t, shape):
        return syn.normal(int(seed), f"host/{int(clip)}/{int(t)}", tuple(shape)).astype(np.float32)

    def _z(self, noise, seed, clip, t, shape):
        if noise is not None:
            return noise.numpy()
        return np.stack([self.draw(seed, c, tt, shape) for c, tt in zip(clip, t)])

    def vb_diffuse(self, x_start, clip, t, noise=None, seed=0, mask=None):
        import torch
        clip, t = clip.numpy(), t.numpy()
        x0 = x_start.numpy()
        z = self._z(noise, seed, clip, t, x0.shape[1:])
        if mask is not None:
            z = z * (1.0 - np.broadcast_to(mask.float().numpy(), x0.shape)[clip])
        a = _bc(_f32(self.tab["sqrt_alphas_cumprod"][t]), z)
        b = _bc(_f32(self.tab["sqrt_one_minus_alphas_cumprod"][t]), z)
        self.calls.append(("diffuse", clip.tolist(), t.tolist()))
        return torch.from_numpy((a * x0[clip] + b * z).astype(np.float32))

    def vb_terms(self, true_log_variance, x_start, x_t, model_output, clip, t, noise=None, seed=0, mask=None, motion=None,
                 clip_denoised=True, mean_type=0, want_xstart=False):
        import torch
        clip, t = clip.numpy(), t.numpy()
        x0 = x_start.numpy()
        assert np.array_equal(true_log_variance.numpy(), self.tab["posterior_log_variance_clipped"].astype(np.float32))
        z = self._z(noise, seed, clip, t, x0.shape[1:])
        g = lambda a: None if a is None else a.float().numpy()[clip]
        r = terms64(self.tab, x0[clip], x_t.numpy(), model_output.numpy(), z, t, mean_type, clip_denoised, g(mask), g(motion), self.large)
        self.calls.append(("terms", clip.tolist(), t.tolist()))
        xs = None
        if want_xstart:
            xs = torch.from_numpy(xstart64(self.tab, model_output.numpy(), x_t.numpy(), t, mean_type, clip_denoised, g(mask),
                                           g(motion))[0].astype(np.float32))
        return torch.from_numpy(r.astype(np.float32)), xs

    def vb_prior(self, x_start, sqrt_ac_last, log_1m_ac_last):
        import torch
        assert float(sqrt_ac_last) == float(self.tab["sqrt_alphas_cumprod"][-1])
        self.calls.append(("prior",))
        return torch.from_numpy(prior64(self.tab, x_start.numpy()).astype(np.float32))


# ------------------------------------------------------------------------------ the golden's inputs, from their seeds
def golden():
    return np.load(os.path.join(GOLDEN, "vb.npz"))


def golden_inputs(case):
    resp, small, n, clip = CASES[case]
    lengths = np.array(LENGTHS[:n])
    return dict(resp=resp, large=not small, n=n, clip_denoised=clip, lengths=lengths,
                x=(X_SCALE * syn.normal(SEED, "vb/x", (2, F, 1, T))[:n]).astype(np.float32), prompts=PROMPTS[:n],
                mask=(np.arange(T)[None] < lengths[:, None]).reshape(n, 1, 1, T))


def golden_noise(case, t, nsteps):
    """The noise the reference's loop drew at timestep index t: its k-th randn_like, k = nsteps - 1 - t."""
    n = CASES[case][2]
    return syn.normal(SEED, f"vb/{case}/noise/{nsteps - 1 - t}", (n, F, 1, T)).astype(np.float32)
