"""The variational-bound evaluation without a GPU: the float64 statement (tests/vb_fixture.py) against the reference's own
`calc_bpd_loop` outputs (tests/golden/vb.npz, made by tests/golden/make_golden_vb.py); the kernel's bars, measured here from the fp32
restatement; the row plan; the Python loop over a host stand-in for the device schedule; `diffusion.losses`; the ABI's refusals."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
import vb_fixture as vf

# the reference's parameter names, recorded from diffusion/gaussian_diffusion.py:1281-1283, :1529, :1547
REF_VB_TERMS = ["self", "model", "x_start", "x_t", "t", "clip_denoised", "model_kwargs"]
REF_PRIOR = ["self", "x_start"]
REF_LOOP = ["self", "model", "x_start", "clip_denoised", "model_kwargs"]


def diffusion(resp="ddim20", inpainting=False, large=False, var=None):
    from mst_amd.diffusion import gaussian_diffusion as gd
    from mst_amd.diffusion.inpainting_gaussian_diffusion import InpaintingGaussianDiffusion
    from mst_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    cls = InpaintingGaussianDiffusion if inpainting else SpacedDiffusion
    var = var or (gd.ModelVarType.FIXED_LARGE if large else gd.ModelVarType.FIXED_SMALL)
    return cls(use_timesteps=space_timesteps(1000, resp or [1000]), betas=gd.get_named_beta_schedule("cosine", 1000),
               model_mean_type=gd.ModelMeanType.START_X, model_var_type=var, loss_type=gd.LossType.MSE)


def on_host(d, resp="ddim20", large=False):
    """`d` with the device schedule replaced by the float64 host stand-in."""
    h = vf.HostSchedule(vf.tables(resp)[0], large)
    d._schedule = lambda device: h
    return h


def affine_vb(tab, large, t):
    """(c_t, const_t) with vb = c_t * xstart_mse + const_t in bits for t != 0, mean types 0 and 1, from float32-rounded entries."""
    c1 = vf._f32(tab["posterior_mean_coef1"][t])
    lv1, lv2 = vf._f32(tab["posterior_log_variance_clipped"][t]), vf._f32(vf.model_logvar(tab, large)[t])
    return 0.5 * c1 ** 2 * np.exp(-lv2) / vf.LN2, 0.5 * (-1.0 + lv2 - lv1 + np.exp(lv1 - lv2)) / vf.LN2


def reference_fp32_vb_error(tab, large, x0, xstart_mse, t):
    """By how much the REFERENCE's own fp32 vb (t != 0) can be off the float64 affine map of its xstart_mse, in bits, [N, T].  Two
    roundings that float64 -- and the kernel, which keeps the row's scalars in double and forms the means' difference as
    c1 (x0 - x0hat) -- does not have; the GPU tests do not use this.
      * the constant: -1 + lv2 - lv1 + exp(lv1 - lv2) is summed per element from terms of size 1, |lv2|, |lv1|, 1: three roundings of
        2^-24 (1 + |lv1| + |lv2|), halved by normal_kl's 0.5.  Under FIXED_SMALL the exact sum is 0 and fp32 leaves one ulp of 1 + |lv|:
        8.6e-8 bits at t = 992 of the full schedule, where the whole term is 1.8e-5 bits -- the 4.7e-3 this golden shows.
      * the means: both are c1 (.) + c2 x_t, of magnitude M = c1 rms(x0) + c2 rms(x_t), each with 2 * 2^-24 M of rounding; their
        difference is c1 sqrt(xstart_mse) in the mean and vb is quadratic in it: relative 8 * 2^-24 M / (c1 sqrt(xstart_mse))."""
    c1, c2 = vf._f32(tab["posterior_mean_coef1"][t])[None], vf._f32(tab["posterior_mean_coef2"][t])[None]
    lv1, lv2 = np.abs(tab["posterior_log_variance_clipped"][t])[None], np.abs(vf.model_logvar(tab, large)[t])[None]
    ac = np.asarray(tab["alphas_cumprod"])[t][None]
    ms0 = (np.asarray(x0, np.float64) ** 2).reshape(len(x0), -1).mean(1)[:, None]
    xs = np.asarray(xstart_mse, np.float64)
    M = c1 * np.sqrt(ms0) + c2 * np.sqrt(ac * ms0 + (1 - ac))
    c, _ = affine_vb(tab, large, t)
    return 0.5 * 3 * 2.0 ** -24 * (1 + lv1 + lv2) / vf.LN2 + c[None] * xs * 8 * 2.0 ** -24 * M / (c1 * np.sqrt(xs))


# ------------------------------------------------------------------------------ 1. the fixture against the reference
@pytest.mark.parametrize("case", list(vf.CASES))
def test_float64_statement_reproduces_the_reference_loop(case):
    """Every array of the golden: vb at t != 0 is the float64 affine map of the golden's own xstart_mse; prior_bpd is the float64 prior
    of the seeded clips; total_bpd is the sum of its parts; rms and the stored pred_xstart respect clip_denoised and each other; the
    t = 0 column lies where the clamps allow.  All within the fp32 restatement's distance D32 (the golden IS fp32 arithmetic)."""
    g, v = vf.golden(), vf.golden_inputs(case)
    tab, _ = vf.tables(v["resp"])
    n, T = v["n"], len(tab["betas"])
    vb, xs, mse, rms, prior, total = (g[f"{case}|{k}"] for k in ("vb", "xstart_mse", "mse", "rms", "prior_bpd", "total_bpd"))
    assert vb.shape == xs.shape == mse.shape == rms.shape == (n, T) and prior.shape == total.shape == (n,)
    t = np.arange(T)[::-1]                                             # column j is t = T - 1 - j
    c, const = affine_vb(tab, v["large"], t)
    want = c[None] * xs.astype(np.float64) + const[None]
    den = np.maximum(np.abs(want), vf.DEN_FLOOR[0])
    d = np.abs(vb - want) / den
    bound = vf.bar("vb") + reference_fp32_vb_error(tab, v["large"], v["x"], xs, t) / den
    j = np.unravel_index((d / bound)[:, :-1].argmax(), (n, T - 1))
    print(f"\n{case}: the golden's vb against the float64 affine map of its xstart_mse: worst distance {d[:, :-1].max():.2e}; worst "
          f"fraction of the reference's own fp32 bound {(d / bound)[j]:.3f} at t = {t[j[1]]} (distance {d[j]:.2e}, bound {bound[j]:.2e})")
    assert (d <= bound)[:, :-1].all()
    if not v["large"]:
        assert np.all(const[:-1] == 0.0)                                  # FIXED_SMALL: the two log-variances are one row
    # t = 0: a mean of -log(max(p, 1e-12)) / ln 2 over elements, p <= 1
    assert np.all(vb[:, -1] >= 0) and np.all(vb[:, -1] <= -np.log(1e-12) / vf.LN2 * (1 + 1e-6))
    dp = vf.distance(prior, vf.prior64(tab, v["x"]))
    assert dp.max() <= vf.bar("prior"), dp
    assert np.allclose(total, vb.astype(np.float64).sum(1) + prior, rtol=1e-6, atol=0)     # (an fp32 sum of T terms)
    for tt in (0, T // 2, T - 1):
        p = g[f"{case}|pred|{tt}"]
        assert p.shape == (n, vf.F, 1, len(range(0, vf.T, vf.STRIDE)))
        if v["clip_denoised"]:
            assert np.abs(p).max() <= 1.0
    if v["clip_denoised"]:
        assert rms.max() <= 1.0
    # |sqrt(xstart_mse) - rms(x0)| <= rms(x0hat) <= sqrt(xstart_mse) + rms(x0): the triangle inequality ties the two stored columns
    r0 = np.sqrt((v["x"].astype(np.float64) ** 2).reshape(n, -1).mean(1))[:, None]
    assert np.all(rms <= (np.sqrt(xs) + r0) * (1 + 1e-5)) and np.all(rms >= np.abs(np.sqrt(xs) - r0) * (1 - 1e-5))
    assert np.all(mse > 0) and np.all(np.isfinite(mse))


ORACLE_T = {"ddim20": (0, 1, 7, 10, 18, 19), "": (0, 1, 250, 500, 992, 999)}


@pytest.mark.parametrize("case", list(vf.CASES))
def test_float64_terms_of_the_oracle_forward_reproduce_the_golden_columns(case):
    """xstart_mse, mse, rms and vb of the golden at six timesteps per case, from the float64 statement fed the CPU oracle's forward
    (oracle/denoiser.py, pinned to the reference's own forward at TOL = 2e-5 relative L2 by tests/test_oracle_golden.py) on x_t
    rebuilt from the seeds.  The forward is the only difference, so the columns are held at that bar propagated per (clip, t) by
    the triangle inequality: |sqrt(xstart_mse) - sqrt(ref)| and |rms - ref| <= B rms_ref, |sqrt(mse) - sqrt(ref)| <= B rms_ref /
    sqrt_recipm1_ac[t], vb (t != 0) through c_t, plus the reference's own fp32 roundings of vb; the stored pred_xstart at B."""
    from conftest import SEED, rel_l2
    from oracle import denoiser
    from test_oracle_golden import TOL as B
    import mst_amd.synthetic as syn
    g, v = vf.golden(), vf.golden_inputs(case)
    tab, tmap = vf.tables(v["resp"])
    n, T = v["n"], len(tab["betas"])
    w, pe = syn.denoiser_state(SEED, vf.F), syn.positional_table(5000, 512)
    txt = np.stack([syn.normal(SEED, "text/" + p, (512,)) for p in v["prompts"]])
    worst = np.zeros(4)
    for ti in ORACLE_T[v["resp"]]:
        ti = min(ti, T - 1)
        t = np.full(n, ti)
        z = vf.golden_noise(case, ti, T)
        a, b = np.float32(tab["sqrt_alphas_cumprod"][ti]), np.float32(tab["sqrt_one_minus_alphas_cumprod"][ti])
        x_t = (a * v["x"] + b * z).astype(np.float32)                      # q_sample as the reference computes it (:281-285)
        out = denoiser.forward(w, pe, x_t, np.asarray(tmap)[t], txt).numpy()
        got = vf.terms64(tab, v["x"], x_t, out, z, t, clip_denoised=v["clip_denoised"], large=v["large"])
        j = T - 1 - ti
        ref = {k: g[f"{case}|{k}"][:, j].astype(np.float64) for k in ("vb", "xstart_mse", "mse", "rms")}
        bn = B * ref["rms"]
        f = [np.abs(np.sqrt(got[:, 1]) - np.sqrt(ref["xstart_mse"])) / bn,
             np.abs(np.sqrt(got[:, 2]) - np.sqrt(ref["mse"])) / (bn / vf._f32(tab["sqrt_recipm1_alphas_cumprod"][ti])),
             np.abs(got[:, 3] - ref["rms"]) / bn]
        if ti != 0:
            c, _ = affine_vb(tab, v["large"], t)
            bound = c * ((np.sqrt(ref["xstart_mse"]) + bn) ** 2 - ref["xstart_mse"]) + \
                reference_fp32_vb_error(tab, v["large"], v["x"], ref["xstart_mse"][:, None], np.array([ti]))[:, 0]
            f.append(np.abs(got[:, 0] - ref["vb"]) / bound)
        else:
            f.append(np.zeros(n))
        worst = np.maximum(worst, [x.max() for x in f])
        key = f"{case}|pred|{ti}"
        if key in g.files:
            pred, _ = vf.xstart64(tab, out, x_t, t, 0, v["clip_denoised"])
            for i in range(n):
                assert rel_l2(pred[i:i + 1, ..., ::vf.STRIDE], g[key][i:i + 1]) <= B, (ti, i)
    print(f"\n{case}: worst fraction of the propagated forward bar -- sqrt(xstart_mse) {worst[0]:.3f}, sqrt(mse) {worst[1]:.3f}, "
          f"rms {worst[2]:.3f}, vb {worst[3]:.3f}")
    assert (worst <= 1.0).all(), worst


def test_golden_cases_differ_where_they_should():
    g = vf.golden()
    assert not np.array_equal(g["ddim20|c1|xstart_mse"], g["ddim20|c0|xstart_mse"])          # clip_denoised acts
    assert np.array_equal(g["ddim20|c0|prior_bpd"], g["large|c0|prior_bpd"])                # the prior knows no variance type
    assert not np.allclose(g["ddim20|c0|vb"][:, :-1], g["large|c0|vb"][:, :-1])             # FIXED_LARGE changes the KL
    assert g["full|c0|vb"].shape == (1, 1000)


# ------------------------------------------------------------------------------ 2. the bars
def test_bars_are_the_fp32_restatements_distance():
    """d32 per column and per_clip class over kernel_cases(), the inputs tests/test_gpu_vb.py gives the kernel: what vb_fixture.D32
    records."""
    worst = {per: {k: 0.0 for k in cols} for per, cols in vf.D32.items()}
    for case in vf.kernel_cases():
        v = vf.case_inputs(case)
        d = vf.distance(vf.case_terms(v, vf.terms32), vf.case_terms(v, vf.terms64))
        z = v["t"] == 0
        w = worst[case[1]]
        for name, val in (("vb", d[~z, 0]), ("vb0", d[z, 0]), ("xstart_mse", d[:, 1]), ("mse", d[:, 2]), ("rms", d[:, 3]),
                          ("prior", vf.distance(vf.prior32(v["tab"], v["x0"]), vf.prior64(v["tab"], v["x0"])))):
            if val.size:
                w[name] = max(w[name], float(val.max()))
    for per in sorted(worst):
        print(f"\nper_clip {per}: d32", {k: f"{v:.2e}" for k, v in worst[per].items()}, "bars", {k: f"{vf.bar(k, per):.2e}" for k in worst[per]})
    for per, cols in vf.D32.items():
        for k, rec in cols.items():
            assert rec / 2 <= worst[per][k] <= rec * 2, (per, k, worst[per][k], rec)


def test_kernel_cases_cover_what_the_issue_names():
    cases = vf.kernel_cases()
    assert {c[1] for c in cases} == {1, 3, 255, 256, 257, 181 * 76, 263 * 196} and {c[2] for c in cases} == {1, 3, 65}
    for col, want in ((3, {"", "ddim20"}), (4, {0, 1, 2}), (5, {0, 1}), (6, {0, 1}), (7, {0, 1}), (8, {0, 1})):
        assert {c[col] for c in cases} == want
    assert any(vf.SHAPES[c[1]][1] % 4 for c in cases)
    seen = set()
    for c in cases:
        n = len(vf.tables(c[3])[0]["betas"])
        seen |= {(int(t) == 0, int(t) == 1, int(t) == n // 2, int(t) == n - 1) for t in vf.case_rows(c[2], n, c[1])[1]}
    assert len(seen) == 4                                                # t = 0, 1, interior, last all occur


# ------------------------------------------------------------------------------ 3. the row plan
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65])
@pytest.mark.parametrize("T", [1, 20, 1000])
@pytest.mark.parametrize("rows", ["n", "default", 7])
def test_row_plan(n, T, rows):
    """Every (clip, t) exactly once, no chunk above `rows`, whole timesteps per chunk, and the concatenation views as [T, N] with
    row 0 = t = T - 1: the reference's column order.  rows = 7 is rounded DOWN to whole timesteps of all N clips; below N it is
    refused by name."""
    from mst_amd.diffusion.gaussian_diffusion import vb_row_plan
    r = {"n": n, "default": None}.get(rows, rows)
    if r is not None and r < n:
        with pytest.raises(ValueError, match="below the"):
            vb_row_plan(n, T, r)
        return
    plan = vb_row_plan(n, T, r)
    cap = max(n, 64 // n * n) if r is None else r
    clip = [c for ch in plan for c in ch[0]]
    t = [tt for ch in plan for tt in ch[1]]
    assert sorted(zip(clip, t)) == sorted((c, tt) for c in range(n) for tt in range(T))
    assert all(len(ch[0]) == len(ch[1]) <= cap and len(ch[0]) % n == 0 for ch in plan)
    assert all(len(ch[0]) == cap // n * n for ch in plan[:-1])          # full chunks but the last
    assert np.array_equal(np.array(t).reshape(T, n), np.repeat(np.arange(T)[::-1], n).reshape(T, n))
    assert np.array_equal(np.array(clip).reshape(T, n), np.tile(np.arange(n), (T, 1)))
    if rows == "n":
        assert len(plan) == T                                             # the reference's loop structure


# ------------------------------------------------------------------------------ 4. the loop on the host stand-in
def _loop_inputs(n=3, F=5, T=6, seed=0):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy((0.6 * rng.standard_normal((n, F, 1, T))).astype(np.float32))
    return x, rng


def test_loop_on_the_host_call_order_kwargs_noise_and_reassembly():
    d = diffusion()
    h = on_host(d)
    n, F, T = 3, 5, 6
    x, rng = _loop_inputs(n, F, T)
    steps = d.num_timesteps
    noise = torch.from_numpy(rng.standard_normal((steps, n, F, 1, T)).astype(np.float32))
    y = {"text": ["a", "b", "c"], "lengths": torch.tensor([6, 4, 2]), "mask": torch.arange(T)[None, None, None] < torch.tensor([6, 4, 2]).view(n, 1, 1, 1),
         "scale": torch.tensor([1.0, 2.0, 3.0]), "style": torch.tensor([7, 8, 9]), "text_embed": torch.arange(3.0).view(3, 1).repeat(1, 4),
         "uncond": False, "tag": "passes through"}
    seen = []

    def model(xx, ts, y=None):
        seen.append((xx.clone(), ts.clone(), y))
        return 0.5 * xx + 0.01 * y["scale"].view(-1, 1, 1, 1)

    out = d.calc_bpd_loop(model, x, clip_denoised=False, model_kwargs={"y": y}, noise=noise, rows=7)
    tmap = np.asarray(d.timestep_map)
    # call order: (diffuse, terms) per chunk of 2 timesteps x 3 clips, t descending, then the prior
    kinds = [c[0] for c in h.calls]
    assert kinds == ["diffuse", "terms"] * (steps // 2) + ["prior"] and len(seen) == steps // 2
    tab = h.tab
    for k, (xx, ts, yy) in enumerate(seen):
        t = np.repeat([steps - 1 - 2 * k, steps - 2 - 2 * k], n)
        clip = np.tile(np.arange(n), 2)
        assert h.calls[2 * k][1:] == (clip.tolist(), t.tolist()) == h.calls[2 * k + 1][1:]
        assert np.array_equal(ts.numpy(), tmap[t])                       # the model sees timestep_map[t]
        assert yy["text"] == [y["text"][c] for c in clip] and yy["uncond"] is False and yy["tag"] == "passes through"
        for key in ("lengths", "mask", "scale", "style", "text_embed"):
            assert torch.equal(yy[key], y[key][clip]), key
        # noise[t] reached the row with timestep t: x_t is the float64 q_sample of (x[clip], noise[t, clip])
        a = vf._bc(vf._f32(tab["sqrt_alphas_cumprod"][t]), xx)
        b = vf._bc(vf._f32(tab["sqrt_one_minus_alphas_cumprod"][t]), xx)
        want = a * x.numpy()[clip] + b * noise.numpy()[t, clip]
        assert np.allclose(xx.numpy(), want, rtol=0, atol=1e-6)
    assert out["vb"].shape == out["xstart_mse"].shape == out["mse"].shape == (n, steps) and out["prior_bpd"].shape == (n,)
    assert torch.equal(out["total_bpd"], out["vb"].sum(dim=1) + out["prior_bpd"])
    # column j is t = steps - 1 - j: recompute two columns from the float64 statement
    for j in (0, steps - 1):
        t = np.full(n, steps - 1 - j)
        xx = seen[j // 2][0].numpy()[(j % 2) * n:(j % 2) * n + n]
        mo = 0.5 * xx + 0.01 * y["scale"].view(-1, 1, 1, 1).numpy()
        want = vf.terms64(tab, x.numpy(), xx, mo, noise.numpy()[t[0]], t, clip_denoised=False)
        got = np.stack([out[k][:, j].numpy() for k in ("vb", "xstart_mse", "mse")], axis=1)
        assert np.allclose(got, want[:, :3], rtol=1e-6, atol=0)
    # the same numbers whatever the packing (the stand-in is float64 per row)
    again = d.calc_bpd_loop(model, x, clip_denoised=False, model_kwargs={"y": y}, noise=noise, rows=n)
    for k in ("vb", "xstart_mse", "mse", "prior_bpd"):
        assert torch.equal(out[k], again[k]), k


def test_loop_on_the_host_seeded_noise_and_the_inpainting_pair():
    """Without noise= the pair (n, t)'s noise comes from the seed alone (the stand-in keys it as the kernel does); an
    InpaintingGaussianDiffusion masks it in q_sample and the pair reaches the terms per CLIP, not per row."""
    d = diffusion(inpainting=True)
    h = on_host(d)
    n, F, T = 2, 5, 6
    x, rng = _loop_inputs(n, F, T, 1)
    mask = torch.zeros(n, F, 1, T, dtype=torch.bool)
    mask[:, :2] = True
    motion = torch.from_numpy(rng.standard_normal((n, F, 1, T)).astype(np.float32))
    y = {"inpainting_mask": mask, "inpainted_motion": motion, "text": ["a", "b"]}
    xts = []

    def model(xx, ts, y=None):
        assert y["inpainting_mask"].shape[0] == xx.shape[0] == y["inpainted_motion"].shape[0]      # gathered for the model
        xts.append(xx.clone())
        return 0.3 * xx

    a = d.calc_bpd_loop(model, x, model_kwargs={"y": y}, seed=11, rows=4)
    first = [v.clone() for v in xts]
    del xts[:]
    b = d.calc_bpd_loop(model, x, model_kwargs={"y": y}, seed=11, rows=2)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(torch.cat(first), torch.cat(xts))                 # identical x_t per (clip, t) under both packings
    # masked rows of x_t carry no noise: x_t = sqrt_ac x there
    steps = d.num_timesteps
    a0 = np.float32(vf._f32(h.tab["sqrt_alphas_cumprod"][steps - 1]))
    assert np.allclose(first[0][:n, :2].numpy(), a0 * x[:, :2].numpy(), rtol=0, atol=1e-7)
    torch.manual_seed(5)
    c = d.calc_bpd_loop(model, x, model_kwargs={"y": y})
    torch.manual_seed(5)
    e = d.calc_bpd_loop(model, x, model_kwargs={"y": y})
    assert torch.equal(c["vb"], e["vb"]) and not torch.equal(c["mse"], a["mse"])      # the default seed comes from torch's generator
    # x0-hat of the blended rows is the motion: _vb_terms_bpd exposes it
    t = torch.tensor([3, 0])
    r = d._vb_terms_bpd(model, x, first[0][:n], t, clip_denoised=False, model_kwargs={"y": y})
    assert r["output"].shape == (n,) and torch.equal(r["pred_xstart"][:, :2], motion[:, :2])


def test_refusals_and_signatures():
    from mst_amd.diffusion import gaussian_diffusion as gd
    for name, want in (("_vb_terms_bpd", REF_VB_TERMS), ("_prior_bpd", REF_PRIOR)):
        assert list(inspect.signature(getattr(gd.GaussianDiffusion, name)).parameters) == want
    sig = inspect.signature(gd.GaussianDiffusion.calc_bpd_loop)
    assert list(sig.parameters)[:len(REF_LOOP)] == REF_LOOP
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("noise", "seed", "rows", "progress"))
    assert sig.parameters["clip_denoised"].default is True
    assert "column 0 is t = t - 1" in gd.GaussianDiffusion.calc_bpd_loop.__doc__.lower()
    x, _ = _loop_inputs()
    model = lambda xx, ts, **kw: xx
    with pytest.raises(RuntimeError, match="GPU"):
        diffusion().calc_bpd_loop(model, x)                              # a CPU x_start
    with pytest.raises(RuntimeError, match="GPU"):
        diffusion()._prior_bpd(x)
    d = diffusion(var=gd.ModelVarType.LEARNED_RANGE)
    on_host(d)
    with pytest.raises(NotImplementedError, match="learned variances"):
        d.calc_bpd_loop(model, x)
    d = diffusion()
    on_host(d)
    with pytest.raises(AssertionError, match="noise"):
        d.calc_bpd_loop(model, x, noise=torch.zeros((3,) + tuple(x.shape)))
    with pytest.raises(ValueError, match="below the"):
        d.calc_bpd_loop(model, x, rows=2)


def test_the_abi_refuses_by_name_without_a_gpu():
    import __graft_entry__ as g
    g.build()
    from mst_amd import _native as N
    lib = N.lib()
    fake = C.cast((C.c_char * 64)(), C.c_void_p)            # a non-null operand: every refusal comes before anything is read
    err = lambda: lib.mst_last_error().decode()
    p = fake
    assert lib.mst_vb_diffuse(None, p, p, None, p, p, 1, 4, 0, 0, 0, p, None) != 0 and "mst_vb_diffuse: null" in err()
    assert lib.mst_vb_diffuse(p, p, p, None, p, p, 0, 4, 0, 0, 0, p, None) != 0 and "rows 0" in err()
    assert lib.mst_vb_diffuse(p, p, p, None, p, p, 1, 0, 0, 0, 0, p, None) != 0 and "per_clip 0" in err()
    assert lib.mst_vb_diffuse(p, p, None, None, p, p, 1, 4, 0, 0, 0, p, None) != 0 and "needs feats and frames" in err()
    assert lib.mst_vb_diffuse(p, p, None, None, p, p, 1, 4, 3, 2, 0, p, None) != 0 and "is not per_clip" in err()
    tm = lambda **k: lib.mst_vb_terms(*[k.get(a, d) for a, d in (("s", p), ("tlv", p), ("x0", p), ("xt", p), ("mo", p), ("z", p), ("mask", None),
                                                                  ("motion", None), ("clip", p), ("t", p), ("rows", 1), ("per", 4), ("F", 0),
                                                                  ("T", 0), ("seed", 0), ("mean", 0), ("cd", 1), ("out", p), ("xs", None),
                                                                  ("stream", None))])
    for k in ("s", "tlv", "x0", "xt", "mo", "clip", "t", "out"):
        assert tm(**{k: None}) != 0 and "mst_vb_terms: null" in err(), k
    assert tm(rows=0) != 0 and "rows 0" in err()
    assert tm(per=0) != 0 and "per_clip 0" in err()
    assert tm(mean=3) != 0 and "bad mean type 3" in err()
    assert tm(mean=-1) != 0 and "bad mean type" in err()
    assert tm(mask=p) != 0 and "mask AND motion" in err()
    assert tm(z=None) != 0 and "needs feats and frames" in err()
    assert tm(z=None, F=2, T=3) != 0 and "is not per_clip" in err()
    assert lib.mst_vb_prior(p, None, 1, 4, 0.1, -0.1, p, None) != 0 and "mst_vb_prior: null" in err()
    assert lib.mst_vb_prior(None, p, 1, 4, 0.1, -0.1, p, None) != 0 and "mst_vb_prior: null" in err()
    assert lib.mst_vb_prior(p, p, 0, 4, 0.1, -0.1, p, None) != 0 and "batch 0" in err()
    assert lib.mst_vb_prior(p, p, 1, 0, 0.1, -0.1, p, None) != 0 and "per_clip 0" in err()


def test_schedule_handles_check_rows_before_the_launch():
    """clip / t out of range, given on the host, never reach the device (the kernels gather by them unchecked)."""
    from mst_amd.engine import Schedule
    s = Schedule.__new__(Schedule)
    s.num_steps, s.handle = 20, None
    x = torch.zeros(2, 3, 1, 4)
    for clip, t, what in (([0, 2], [1, 1], "clip index"), ([0, -1], [1, 1], "clip index"), ([0, 1], [1, 20], "timestep index")):
        with pytest.raises(IndexError, match=what):
            s.vb_diffuse(x, clip, t, noise=torch.zeros(2, 3, 1, 4))
        with pytest.raises(IndexError, match=what):
            s.vb_terms(torch.zeros(20), x, x, x, torch.tensor(clip), torch.tensor(t), noise=x)
    with pytest.raises(ValueError, match="one pair per row"):
        s.vb_diffuse(x, [0, 1], [1], noise=x)
    with pytest.raises(RuntimeError, match="needs a GPU"):
        s.vb_diffuse(x, [0, 1], [1, 2], noise=x)                         # valid rows, CPU tensors: refused as everywhere else


# ------------------------------------------------------------------------------ 5. diffusion.losses
def test_losses_against_the_float64_statement():
    from mst_amd.diffusion import losses
    rng = np.random.default_rng(3)
    shp = (4, 7, 1, 9)
    x = rng.standard_normal(shp) * 0.8                                  # |x| > 0.999 for about one element in five
    x.flat[:6] = [-1.0, 1.0, -0.9991, 0.9991, -0.999, 0.999]
    means = x + rng.standard_normal(shp) * np.array([1e-3, 0.05, 1.0, 30.0]).reshape(4, 1, 1, 1)      # ... and saturated CDF arguments
    ls = np.broadcast_to(np.array([-6.0, -2.0, 0.0, -4.0]).reshape(4, 1, 1, 1), shp).copy()
    assert (np.abs(x) > 0.999).sum() > 20
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    # float64 tensors: the functions are the float64 statement, to rounding
    got = losses.discretized_gaussian_log_likelihood(f(x), means=f(means), log_scales=f(ls)).numpy()
    want = vf.discretized_gaussian_log_likelihood(x, means, ls)
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12)
    assert (want == np.log(1e-12)).any() and (want > -1.0).any()           # the clamp and the resolved regime both occur
    assert np.allclose(losses.approx_standard_normal_cdf(f(means)).numpy(), vf.approx_standard_normal_cdf(means), rtol=1e-13, atol=1e-15)
    m2, l2 = rng.standard_normal(shp), rng.standard_normal(shp)
    assert np.allclose(losses.normal_kl(f(x), f(ls), f(m2), f(l2)).numpy(), vf.normal_kl(x, ls, m2, l2), rtol=1e-13, atol=1e-15)
    # float32 tensors: the reference's precision; scalars broadcast and take the tensor's dtype
    k32 = losses.normal_kl(f(x).float(), f(ls).float(), 0.0, 0.0)
    assert k32.dtype == torch.float32 and np.allclose(k32.numpy(), vf.normal_kl(x, ls, 0.0, 0.0), rtol=2e-5, atol=1e-6)
    assert np.allclose(losses.normal_kl(0.5, -1.0, f(m2), 0.25).numpy(), vf.normal_kl(0.5, -1.0, m2, 0.25), rtol=1e-13)
    with pytest.raises(AssertionError, match="at least one argument"):
        losses.normal_kl(0.0, 0.0, 1.0, 0.0)
    with pytest.raises(AssertionError):
        losses.discretized_gaussian_log_likelihood(f(x), means=f(means)[:2], log_scales=f(ls))
    assert np.array_equal(losses.normal_kl(f(x), f(ls), f(x), f(ls)).numpy(), np.zeros(shp))      # KL(p || p) = 0 exactly
