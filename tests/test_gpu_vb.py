"""The variational-bound evaluation on the GPU (csrc/mst_vb.h, `Schedule.vb_diffuse / vb_terms / vb_prior`,
`GaussianDiffusion._vb_terms_bpd / _prior_bpd / calc_bpd_loop`).

  1. `vb_terms` against the float64 statement (tests/vb_fixture.py) over `kernel_cases()`, within the bars measured on the CPU from the
     fp32 restatement (vb_fixture.D32, tests/test_vb_cpu.py): every row of every case is compared.
  2. a row's four values are the same bits alone, anywhere among 65 shuffled rows, and on another stream.
  3. `vb_diffuse` is `Schedule.q_sample` on the gathered operands, bit for bit, from a buffer and from the counter.
  4. `calc_bpd_loop` against the reference's own loop (tests/golden/vb.npz): the model call is the only difference, bounded by the
     forward bar of tests/test_gpu_parity.py and propagated per (clip, t).
  5. the packing (`rows`) does not matter.
  6. a ClassifierFreeSampleModel and an InpaintingGaussianDiffusion with the pair."""

import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
import mst_amd.synthetic as syn
import vb_fixture as vf
from conftest import SEED, rel_l2
from test_gpu_parity import TOL_ELEM, TOL as B_FORWARD           # the forward bar: relative L2 on x0-hat against the fp32 reference
from test_gpu_reverse import cu, dev

pytestmark = pytest.mark.gpu

_SCH = {}


def sched(resp, large=False):
    from mst_amd.engine import Schedule
    if (resp, large) not in _SCH:
        tab, tmap = vf.tables(resp)
        _SCH[resp, large] = Schedule(tab, tmap, dev(), log_variance=vf.model_logvar(tab, large), variance=vf.model_variance(tab, large))
    return _SCH[resp, large]


def true_logvar(resp):
    return cu(vf.tables(resp)[0]["posterior_log_variance_clipped"].astype(np.float32))


def philox(n, F, T, seed, step):
    """mst_philox_normal(N, F, T, seed, step) -> [N, F, 1, T]: what a drawn row (clip, t = step) must see at index clip."""
    from mst_amd import _native as N
    out = torch.empty((n, F, 1, T), device=dev(), dtype=torch.float32)
    N.check(N.lib().mst_philox_normal(N.ptr(out), n, F, T, int(seed), int(step), N.stream_ptr(dev())))
    return out


_PH = {}


def z_of(clip, t, F, T, seed, n):
    key = (n, F, T, seed, t)
    if key not in _PH:
        _PH[key] = philox(n, F, T, seed, t).cpu().numpy()
    return _PH[key][clip]


def run_terms(v, resp, rows=None, want_xstart=False):
    """The kernel on a fixture case (optionally on a subset / permutation `rows` of its rows)."""
    r = np.arange(len(v["t"])) if rows is None else np.asarray(rows)
    s = sched(resp, v["large"])
    c = lambda a: None if a is None else cu(a)
    return s.vb_terms(true_logvar(resp), cu(v["x0"]), cu(v["x_t"][r]), cu(v["out"][r]), v["clip"][r], v["t"][r],
                      noise=None if v["draw"] else cu(v["z"][r]), seed=v["seed"], mask=c(v["mask"]), motion=c(v["motion"]),
                      clip_denoised=v["clip_denoised"], mean_type=v["mean"], want_xstart=want_xstart)


# ------------------------------------------------------------------------------ 1. the terms against float64
@pytest.mark.parametrize("per", sorted(vf.SHAPES))
def test_terms_equal_the_float64_statement_within_the_measured_bars(per):
    """Every case of kernel_cases() at this per_clip, every row compared; x0-hat (stored on request) against the float64 one.
    Prints the worst fraction of each bar."""
    frac = np.zeros(5)
    cases = [c for c in vf.kernel_cases() if c[1] == per]
    assert cases
    for case in cases:
        v = vf.case_inputs(case, z_of)
        got, xs = run_terms(v, case[3], want_xstart=True)
        got = got.cpu().numpy()
        assert got.shape == (len(v["t"]), 4) and np.isfinite(got).all(), case[0]
        want = vf.case_terms(v, vf.terms64)
        f = vf.distance(got, want) / vf.row_bars(v["t"], per)
        assert (f <= 1.0).all(), (case[0], v["t"].tolist(), f.max(axis=0), got[f.max(axis=1).argmax()], want[f.max(axis=1).argmax()])
        z = v["t"] == 0
        frac[0] = max(frac[0], f[~z, 0].max() if (~z).any() else 0)
        frac[4] = max(frac[4], f[z, 0].max() if z.any() else 0)
        frac[1:4] = np.maximum(frac[1:4], f[:, 1:].max(axis=0))
        g = lambda a: None if a is None else a[v["clip"]]
        p64, _ = vf.xstart64(v["tab"], v["out"], v["x_t"], v["t"], v["mean"], v["clip_denoised"], g(v["mask"]), g(v["motion"]))
        assert xs.shape == v["x_t"].shape
        # the stored x0-hat, every mean type: elementwise within 2e-6 (the fp32 elementwise bar of tests/test_gpu_parity.py) of the
        # products the conversion sums -- |out'|, srac |x_t| + srm1ac |out'|, (|out'| + c2 |x_t|) / c1
        e = lambda k: vf._bc(vf._f32(np.asarray(v["tab"][k])[v["t"]]), v["x_t"])
        o = np.abs(vf.xstart64(v["tab"], v["out"], v["x_t"], v["t"], 0, False, g(v["mask"]), g(v["motion"]))[0])
        ax = np.abs(v["x_t"].astype(np.float64))
        scale = {0: o, 1: e("sqrt_recip_alphas_cumprod") * ax + e("sqrt_recipm1_alphas_cumprod") * o,
                 2: (o + e("posterior_mean_coef2") * ax) / e("posterior_mean_coef1")}[v["mean"]]
        assert (np.abs(xs.cpu().numpy() - p64) <= TOL_ELEM * np.maximum(scale, 1e-30)).all(), case[0]
    print(f"\nper_clip {per}: {len(cases)} cases, worst fraction of the bar -- vb {frac[0]:.3f}, xstart_mse {frac[1]:.3f}, "
          f"mse {frac[2]:.3f}, rms {frac[3]:.3f}, vb at t = 0 {frac[4]:.3f}")


def test_prior_equals_the_float64_statement():
    for resp in ("", "ddim20"):
        tab, _ = vf.tables(resp)
        for per, (F, T) in vf.SHAPES.items():
            x = (vf.X_SCALE * syn.normal(SEED, f"vbk/{per}/x0", (3, F, 1, T))).astype(np.float32)
            got = sched(resp).vb_prior(cu(x), tab["sqrt_alphas_cumprod"][-1], tab["log_one_minus_alphas_cumprod"][-1]).cpu().numpy()
            d = vf.distance(got, vf.prior64(tab, x))
            assert d.max() <= vf.bar("prior", per), (resp, per, d)


# ------------------------------------------------------------------------------ 2. position independence
@pytest.mark.parametrize("cid", ["13756-65-ddim20-0-1-0-0-1", "257-65-ddim20-1-0-0-1-1", "255-65-full-0-1-1-0-0"])
def test_a_rows_values_do_not_depend_on_its_position(cid):
    case = next(c for c in vf.kernel_cases() if c[0] == cid)
    v = vf.case_inputs(case, z_of)
    R = len(v["t"])
    assert R == 65
    whole, _ = run_terms(v, case[3])
    perm = np.random.default_rng(7).permutation(R)
    shuffled, _ = run_terms(v, case[3], perm)
    assert torch.equal(shuffled, whole[torch.from_numpy(perm).to(dev())])
    for r in (int(perm[0]), int(perm[R // 2]), int(perm[-1]), 0, R - 1):
        alone, _ = run_terms(v, case[3], [r])
        assert torch.equal(alone[0], whole[r]), r
    side = torch.cuda.Stream(device=dev())
    side.wait_stream(torch.cuda.current_stream(dev()))
    with torch.cuda.stream(side):
        a, _ = run_terms(v, case[3])
        b, _ = run_terms(v, case[3])
    side.synchronize()
    assert torch.equal(a, whole) and torch.equal(b, whole)


# ------------------------------------------------------------------------------ 3. vb_diffuse is q_sample
@pytest.mark.parametrize("F", [181, 263])
@pytest.mark.parametrize("T", [6, 76, 77])
@pytest.mark.parametrize("masked", [0, 1])
def test_diffuse_is_q_sample_on_the_gathered_operands(F, T, masked):
    n, seed = 3, 4242
    for resp in ("", "ddim20"):
        s = sched(resp)
        steps = s.num_steps
        clip = np.array([2, 0, 1, 1, 2, 0, 2])
        t = np.array([0, steps - 1, 1, steps // 2, steps - 1, 0, 3])
        x0 = cu(syn.normal(SEED, f"vbd/{F}/{T}/x0", (n, F, 1, T)))
        z = cu(syn.normal(SEED, f"vbd/{F}/{T}/z", (len(t), F, 1, T)))
        mask = cu((syn.uniform(SEED, f"vbd/{F}/{T}/m", (n, F, 1, T), 0.0, 1.0) < 0.4).astype(np.float32)) if masked else None
        ci, ti = torch.from_numpy(clip).to(dev()), torch.from_numpy(t).to(dev())
        gm = None if mask is None else mask[ci]
        got = s.vb_diffuse(x0, clip, t, noise=z, mask=mask)
        assert torch.equal(got, s.q_sample(x0[ci].contiguous(), ti, z, gm))
        drawn = s.vb_diffuse(x0, clip, t, seed=seed, mask=mask)
        zz = torch.stack([philox(n, F, T, seed, int(tt))[int(c)] for c, tt in zip(clip, t)])
        assert torch.equal(drawn, s.q_sample(x0[ci].contiguous(), ti, zz, gm))
        # the packing does not matter: the same pairs in another order and another batch give the same rows
        other = s.vb_diffuse(x0, clip[::-1].copy(), t[::-1].copy(), seed=seed, mask=mask)
        assert torch.equal(other.flip(0), drawn)
        assert torch.equal(s.vb_diffuse(x0, clip[3:4], t[3:4], seed=seed, mask=mask)[0], drawn[3])


# ------------------------------------------------------------------------------ 4. the loop against the reference's
def _diffusion(resp, large=False, inpainting=False):
    from mst_amd.diffusion import gaussian_diffusion as gd
    from mst_amd.diffusion.inpainting_gaussian_diffusion import InpaintingGaussianDiffusion
    from mst_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    cls = InpaintingGaussianDiffusion if inpainting else SpacedDiffusion
    return cls(use_timesteps=space_timesteps(1000, resp or [1000]), betas=gd.get_named_beta_schedule("cosine", 1000),
               model_mean_type=gd.ModelMeanType.START_X,
               model_var_type=gd.ModelVarType.FIXED_LARGE if large else gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE)


def _model():
    from test_gpu_boundary import build
    return build()["m"]


def _golden_setup(case):
    v = vf.golden_inputs(case)
    tab, _ = vf.tables(v["resp"])
    steps = len(tab["betas"])
    x = cu(v["x"])
    noise = cu(np.stack([vf.golden_noise(case, t, steps) for t in range(steps)]))
    y = {"y": {"text": list(v["prompts"]), "lengths": torch.from_numpy(v["lengths"]).to(dev()), "mask": cu(v["mask"])}}
    return v, tab, steps, x, noise, y


def affine_vb(tab, large, t):
    """(c_t, const_t): vb = c_t xstart_mse + const_t in bits at t != 0 (x_start models, fixed variances), float32-rounded entries."""
    c1 = vf._f32(tab["posterior_mean_coef1"][t])
    lv1, lv2 = vf._f32(tab["posterior_log_variance_clipped"][t]), vf._f32(vf.model_logvar(tab, large)[t])
    return 0.5 * c1 ** 2 * np.exp(-lv2) / vf.LN2, 0.5 * (-1.0 + lv2 - lv1 + np.exp(lv1 - lv2)) / vf.LN2


def propagated(tab, large, steps, out, ref_xs, ref_mse, ref_vb, rms, noise=0.0):
    """The forward bar B on x0-hat, per (clip, t) by the triangle inequality (columns: t = steps - 1 - j):
        |sqrt(xstart_mse) - sqrt(ref)| <= B rms(x0hat_ref)
        |sqrt(mse) - sqrt(ref)|        <= B rms(x0hat_ref) / sqrt_recipm1_ac[t]
        |vb - ref| (t != 0)            <= c_t ((sqrt(ref_xs) + B rms)^2 - ref_xs)                    (vb = c_t xstart_mse + const_t)
    and nothing else.  noise: between two runs of THIS kernel, its output rounding (relative to |ref|, 1e-6); 0 against a reference.
    Returns the worst fraction of each bound."""
    t = np.arange(steps)[::-1]
    bn = B_FORWARD * rms.astype(np.float64)
    f_xs = np.abs(np.sqrt(out["xstart_mse"]) - np.sqrt(ref_xs)) / bn
    srm1 = vf._f32(tab["sqrt_recipm1_alphas_cumprod"][t])[None]
    f_mse = np.abs(np.sqrt(out["mse"]) - np.sqrt(ref_mse)) / (bn / srm1)
    c, _ = affine_vb(tab, large, t)
    bound = c[None] * ((np.sqrt(ref_xs) + bn) ** 2 - ref_xs) + noise * np.abs(ref_vb)
    f_vb = (np.abs(out["vb"] - ref_vb) / bound)[:, :-1]
    return float(f_xs.max()), float(f_mse.max()), float(f_vb.max())


# The reference's own fp32 vb is not the float64 affine map of its xstart_mse: per element it sums -1 + lv2 - lv1 + exp(lv1 - lv2)
# from terms of size 1, which under FIXED_SMALL leaves one ulp of 1 + |lv| where float64 (and this kernel) has exactly 0.  Under
# "ddim20" that is 3e-6 of vb.  Over the full schedule it is 4.7e-3 of vb at t = 992 (8.6e-8 bits of a 1.8e-5-bit term;
# tests/test_vb_cpu.py measures and bounds it), which is MORE than the forward bar propagated through c_t allows there: against the
# golden's vb itself the full-schedule case stands at 3.3 times that bound (measured on an MI355X, printed by the test), a finding
# about the reference's arithmetic, not a tolerance.  So every case is held, with the plain bound, to c_t xstart_mse_golden + const_t
# in float64 -- the identity the bound on vb is derived from -- and the three "ddim20" cases to the golden's vb itself as well.


@pytest.mark.parametrize("case", list(vf.CASES))
def test_loop_against_the_references_golden(case):
    g = vf.golden()
    v, tab, steps, x, noise, y = _golden_setup(case)
    d, m = _diffusion(v["resp"], v["large"]), _model()
    res = d.calc_bpd_loop(m, x, clip_denoised=v["clip_denoised"], model_kwargs=y, noise=noise)
    out = {k: a.cpu().numpy().astype(np.float64) for k, a in res.items()}
    n = v["n"]
    assert out["vb"].shape == (n, steps) and all(np.isfinite(a).all() for a in out.values())
    ref = {k: g[f"{case}|{k}"].astype(np.float64) for k in ("vb", "xstart_mse", "mse", "rms", "prior_bpd", "total_bpd")}
    t = np.arange(steps)[::-1]
    c, const = affine_vb(tab, v["large"], t)
    ref_map = c[None] * ref["xstart_mse"] + const[None]                   # float64: what the bound on vb is derived from
    f_xs, f_mse, f_vb = propagated(tab, v["large"], steps, out, ref["xstart_mse"], ref["mse"], ref_map, ref["rms"])
    _, _, f_direct = propagated(tab, v["large"], steps, out, ref["xstart_mse"], ref["mse"], ref["vb"], ref["rms"])
    print(f"\n{case}: worst fraction of the propagated forward bar -- sqrt(xstart_mse) {f_xs:.3f}, sqrt(mse) {f_mse:.3f}, "
          f"vb against c_t xstart_mse_golden + const_t {f_vb:.3f}, vb against the golden's own fp32 vb {f_direct:.3f}")
    assert f_xs <= 1.0 and f_mse <= 1.0 and f_vb <= 1.0
    if v["resp"] == "ddim20":
        assert f_direct <= 1.0
    # vb is the float64 affine map of the loop's own xstart_mse, at the kernel bar
    want = c[None] * out["xstart_mse"] + const[None]
    assert (np.abs(out["vb"] - want) <= vf.bar("vb") * np.maximum(np.abs(want), vf.DEN_FLOOR[0]))[:, :-1].all()
    # the prior at the kernel bar; the total is the sum of its parts
    assert vf.distance(out["prior_bpd"], vf.prior64(tab, v["x"])).max() <= vf.bar("prior")
    assert torch.equal(res["total_bpd"], res["vb"].sum(dim=1) + res["prior_bpd"])
    # t = 0 is not linear in x0-hat: the float64 statement at the loop's OWN x0-hat (exposed by _vb_terms_bpd), at the kernel bar,
    # and that x0-hat against the golden's stored one by the forward bar
    t0 = torch.zeros(n, dtype=torch.long, device=dev())
    x_t = d.q_sample(x, t0, noise[0])
    r = d._vb_terms_bpd(m, x, x_t, t0, clip_denoised=v["clip_denoised"], model_kwargs=y)
    pred = r["pred_xstart"].cpu().numpy()
    want0 = vf.terms64(tab, v["x"], x_t.cpu().numpy(), None, noise[0].cpu().numpy(), np.zeros(n, dtype=np.int64), large=v["large"],
                       pred=pred)[:, 0]
    d0 = vf.distance(r["output"].cpu().numpy(), want0)
    print(f"{case}: t = 0 against float64 at its own x0-hat: {d0.max():.2e} (bar {vf.bar('vb0'):.2e})")
    assert d0.max() <= vf.bar("vb0")
    for i in range(n):
        e = rel_l2(pred[i:i + 1, ..., ::vf.STRIDE], g[f"{case}|pred|0"][i:i + 1])
        assert e <= B_FORWARD, (i, e)
    for ti in (steps // 2, steps - 1):                                    # ... and at the other two indices the golden keeps x0-hat of
        tt = torch.full((n,), ti, dtype=torch.long, device=dev())
        p = d._vb_terms_bpd(m, x, d.q_sample(x, tt, noise[ti]), tt, clip_denoised=v["clip_denoised"], model_kwargs=y)["pred_xstart"]
        for i in range(n):
            e = rel_l2(p[i:i + 1, ..., ::vf.STRIDE].cpu().numpy(), g[f"{case}|pred|{ti}"][i:i + 1])
            assert e <= B_FORWARD, (ti, i, e)
    # the loop at rows = N makes that very call: the same bits
    if steps <= 20:
        by_n = d.calc_bpd_loop(m, x, clip_denoised=v["clip_denoised"], model_kwargs=y, noise=noise, rows=n)
        assert torch.equal(by_n["vb"][:, -1], r["output"])


# ------------------------------------------------------------------------------ 5. the packing does not matter
def test_default_rows_and_rows_n_agree():
    case = "ddim20|c0"
    g = vf.golden()
    v, tab, steps, x, noise, y = _golden_setup(case)
    d, m = _diffusion(v["resp"]), _model()
    a = d.calc_bpd_loop(m, x, clip_denoised=False, model_kwargs=y, noise=noise)
    b = d.calc_bpd_loop(m, x, clip_denoised=False, model_kwargs=y, noise=noise, rows=v["n"])
    an, bn = ({k: r[k].cpu().numpy().astype(np.float64) for k in r} for r in (a, b))
    f = propagated(tab, False, steps, an, bn["xstart_mse"], bn["mse"], bn["vb"], g[f"{case}|rms"], noise=vf.BAR_FLOOR)
    print(f"\ndefault rows against rows = N: worst fraction of the propagated forward bar {f}")
    assert max(f) <= 1.0
    assert torch.equal(a["prior_bpd"], b["prior_bpd"])
    # seeded: both packings see identical x_t bits per (clip, t), and a seeded loop is reproducible
    from mst_amd.diffusion.gaussian_diffusion import vb_row_plan
    s = d._schedule(dev())
    xt = {}
    for rows in (None, v["n"]):
        parts = [s.vb_diffuse(x, c, t, seed=99) for c, t in vb_row_plan(v["n"], steps, rows)]
        xt[rows] = torch.cat(parts)
    assert torch.equal(xt[None], xt[v["n"]])
    s1 = d.calc_bpd_loop(m, x, clip_denoised=False, model_kwargs=y, seed=99)
    s2 = d.calc_bpd_loop(m, x, clip_denoised=False, model_kwargs=y, seed=99)
    assert all(torch.equal(s1[k], s2[k]) for k in s1)
    assert not torch.equal(s1["mse"], a["mse"])


# ------------------------------------------------------------------------------ 6. CFG wrapper, inpainting diffusion
def test_cfg_wrapper_and_inpainting_diffusion_agree_with_float64_at_their_own_xstart():
    from mst_amd.model.cfg_sampler import ClassifierFreeSampleModel
    v, tab, steps, x, noise, y = _golden_setup("ddim20|c1")
    n = v["n"]
    m = _model()
    cfg = ClassifierFreeSampleModel(m)
    mask = cu(syn.root_horizontal_mask(n, vf.F, vf.T))
    motion = cu(vf.X_SCALE * syn.normal(SEED, "vb/motion", (n, vf.F, 1, vf.T)))
    runs = (("cfg", _diffusion("ddim20"), cfg, {"y": {**y["y"], "scale": torch.tensor([2.5, 1.5], device=dev())}}, None),
            ("inpainting", _diffusion("ddim20", inpainting=True), m,
             {"y": {**y["y"], "inpainting_mask": mask, "inpainted_motion": motion}}, mask))
    for name, d, model, kw, nmask in runs:
        for ti in (0, 7, steps - 1):
            t = torch.full((n,), ti, dtype=torch.long, device=dev())
            x_t = d.q_sample(x, t, noise[ti], model_kwargs=kw)
            if nmask is not None:                                         # the inpainting class masks the noise in q_sample
                a = np.float32(tab["sqrt_alphas_cumprod"][ti])
                assert torch.allclose(x_t[:, :3], a * x[:, :3], rtol=0, atol=1e-6)
            r = d._vb_terms_bpd(model, x, x_t, t, clip_denoised=True, model_kwargs=kw)
            pred = r["pred_xstart"].cpu().numpy()
            if nmask is not None:
                assert torch.equal(r["pred_xstart"][:, :3], motion[:, :3].clamp(-1, 1))      # blended, then clip_denoised
            want = vf.terms64(tab, v["x"], x_t.cpu().numpy(), None, noise[ti].cpu().numpy(), np.full(n, ti), pred=pred)[:, 0]
            dd = vf.distance(r["output"].cpu().numpy(), want)
            assert dd.max() <= (vf.bar("vb0") if ti == 0 else vf.bar("vb")), (name, ti, dd)
        res = d.calc_bpd_loop(model, x, model_kwargs=kw, noise=noise)
        assert res["vb"].shape == (n, steps) and all(torch.isfinite(a).all() for a in res.values()), name
        assert torch.equal(res["total_bpd"], res["vb"].sum(dim=1) + res["prior_bpd"])
        seeded = d.calc_bpd_loop(model, x, model_kwargs=kw, seed=3, rows=n)
        assert all(torch.isfinite(a).all() for a in seeded.values()), name
