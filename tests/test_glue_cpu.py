"""Round 6's launch diet on the Python side changes no value (docs/LAB_NOTES.md R6.17): the two-launch `mask_cond` draws the same Bernoulli
mask from the same generator state and returns the same tensor as the reference's op sequence (model/mdm_forstyledataset.py:288-296); a cached
constant timestep batch and its cached respacing are what `th.full` + the index would give.  CPU: the code paths are device-agnostic."""
import types

import numpy as np
import torch

import mst_amd  # noqa: F401
from mst_amd.diffusion import gaussian_diffusion as gd
from mst_amd.diffusion.respace import _WrappedModel
from mst_amd.model import mdm_forstyledataset as mdm


def test_mask_cond_fast_path_is_the_reference_sequence(monkeypatch):
    mod = types.SimpleNamespace(training=True, cond_mask_prob=0.3)
    cond = torch.randn(64, 512)
    torch.manual_seed(7)
    fast = mdm._mask_cond(mod, cond)
    state_after_fast = torch.get_rng_state()
    monkeypatch.setenv("MST_GLUE_CACHE", "0")
    torch.manual_seed(7)
    ref = mdm._mask_cond(mod, cond)
    assert torch.equal(torch.get_rng_state(), state_after_fast), "the fast path consumed the generator differently"
    assert torch.equal(fast == 0, ref == 0) and torch.allclose(fast, ref, rtol=0, atol=0)
    dropped = (ref.abs().sum(1) == 0).float().mean().item()
    assert 0.1 < dropped < 0.5
    # the mask handed over as drawn (mst_set_text_dropped's input) is the same draw
    monkeypatch.delenv("MST_GLUE_CACHE")
    torch.manual_seed(7)
    drop = mdm._cond_drop(mod, cond)
    assert torch.equal(drop.bool(), ref.abs().sum(1) == 0)
    # eval mode / p = 0: untouched; force_mask: zeros
    mod2 = types.SimpleNamespace(training=False, cond_mask_prob=0.3)
    assert mdm._mask_cond(mod2, cond) is cond
    assert float(mdm._mask_cond(mod, cond, force_mask=True).abs().max()) == 0.0


def test_constant_timesteps_and_their_respacing_from_the_cache(monkeypatch):
    holder = types.SimpleNamespace()
    t = gd.GaussianDiffusion._const_timesteps(holder, 5, 3, "cpu")
    assert torch.equal(t, torch.full((3,), 5, dtype=torch.long)) and t._mst_const == 5
    assert gd.GaussianDiffusion._const_timesteps(holder, 5, 3, "cpu") is t
    assert gd.GaussianDiffusion._const_timesteps(holder, 4, 3, "cpu") is not t
    seen = []
    wrapped = _WrappedModel(lambda x, ts, **kw: seen.append(ts) or x, [0, 50, 100, 150, 200, 250, 300], False, 1000)
    x = torch.zeros(3, 2)
    wrapped(x, t)
    wrapped(x, t)                                           # second call: served from the cache
    wrapped(x, torch.full((3,), 5, dtype=torch.long))       # an untagged tensor: the index path
    assert seen[0] is seen[1] and torch.equal(seen[0], seen[2]) and torch.equal(seen[2], torch.full((3,), 250, dtype=torch.long))
    resc = _WrappedModel(lambda x, ts, **kw: seen.append(ts) or x, [0, 50, 100, 150, 200, 250, 300], True, 1000)
    resc(x, t)
    assert torch.allclose(seen[-1], torch.full((3,), 250.0))
    monkeypatch.setenv("MST_GLUE_CACHE", "0")
    u = gd.GaussianDiffusion._const_timesteps(holder, 5, 3, "cpu")
    assert u is not t and not hasattr(u, "_mst_const") and torch.equal(u, t)


# ---- tests/glue_fixture.py, the float64 closed forms the GPU glue tests measure against, held to what already exists ----------------
def _glue_inputs(n, F, T, seed=5):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, F, 1, T, generator=g)
    b = torch.randn(n, F, 1, T, generator=g)
    m = (torch.rand(n, 1, 1, T, generator=g) > 0.3).float()
    m[..., 0] = 1.0
    return a, b, m, torch.randn(n, generator=g)


def test_fixture_masked_l2_is_the_reference_formula_and_its_autograd():
    import glue_fixture as gf
    a, b, m, g = _glue_inputs(3, 7, 11)
    for aa, mm in ((a, m), (a[:1].expand(3, -1, -1, -1), m[:1].expand(3, -1, -1, -1))):
        bb = b.double().requires_grad_(True)
        ref = gf.masked_l2_torch(aa.double(), bb, mm.double())
        (ref * g.double()).sum().backward()
        assert gf.rel(gf.masked_l2(aa, b, mm), ref) < 1e-14
        assert gf.rel(gf.masked_l2_grad_b(aa, b, mm, g), bb.grad) < 1e-14
    from oracle import diffusion
    assert gf.rel(diffusion.masked_l2(a, b, m), gf.masked_l2(a, b, m)) < 1e-6


def test_fixture_text_cosine_is_the_reference_formula_and_its_autograd():
    import glue_fixture as gf
    g = torch.Generator().manual_seed(6)
    f, m0 = torch.randn(5, 33, generator=g), torch.randn(5, 33, generator=g) * 3
    m = m0.double().requires_grad_(True)
    ref = gf.text_cosine_torch(f.double(), m)
    (ref * 10.0).backward()
    assert abs(gf.text_cosine(f, m0) - float(ref.detach())) < 1e-14
    assert gf.rel(gf.text_cosine_grad_m(f, m0, 10.0), m.grad) < 1e-13
    assert abs(gf.text_cosine(f.double() * 1e3, m0.double() * 1e-3) - gf.text_cosine(f, m0)) < 1e-14          # scale-invariant


def test_fixture_step_gradient_is_autograd_of_the_reference_step():
    import glue_fixture as gf
    from oracle import schedule
    tab, _ = schedule.make("cosine", 1000, "ddim20")
    tab64 = dict(tab)
    g = torch.Generator().manual_seed(7)
    shape = (3, 6, 1, 5)
    out0, x, nz, mot, ws, wp = (torch.randn(shape, generator=g).double() for _ in range(6))
    mask = torch.zeros(shape, dtype=torch.float64)
    mask[:, :2] = 1
    t = torch.tensor([0, 7, 19])

    def ex(arr):                                     # float64 all the way: the closed form carries no fp32 table rounding
        return torch.from_numpy(np.asarray(arr))[t].view(-1, 1, 1, 1)
    for ddim, eta in ((False, 0.0), (True, 0.0), (True, 0.5)):
        for blend in (True, False):
            for clip in (True, False):
                o = out0.clone().requires_grad_(True)
                pred = o * (1 - mask) + mot * mask if blend else o
                if clip:
                    pred = pred.clamp(-1, 1)
                if not ddim:
                    sample = ex(tab64["posterior_mean_coef1"]) * pred + ex(tab64["posterior_mean_coef2"]) * x
                else:
                    eps = (ex(tab64["sqrt_recip_alphas_cumprod"]) * x - pred) / ex(tab64["sqrt_recipm1_alphas_cumprod"])
                    ab, abp = ex(tab64["alphas_cumprod"]), ex(tab64["alphas_cumprod_prev"])
                    sigma = eta * torch.sqrt((1 - abp) / (1 - ab)) * torch.sqrt(1 - ab / abp)
                    sample = pred * torch.sqrt(abp) + torch.sqrt(1 - abp - sigma ** 2) * eps + sigma * nz
                ((sample * ws).sum() + (pred * wp).sum()).backward()
                got = gf.step_d_out(tab64, t.numpy(), ddim, eta, ws, wp, mask if blend else None, pred.detach() if clip else None)
                assert gf.rel(got, o.grad) < 1e-13, (ddim, eta, blend, clip)
    # the fp32 torch form used as the yardstick is the same algebra
    s32, p32 = gf.step_torch(tab, t, True, 0.5, out0.float(), x.float(), nz.float(), mask.float(), mot.float(), False)
    s_ref, _ = diffusion_ddim(tab, out0, x, t, nz, mask, mot)
    assert gf.rel(s32, s_ref) < 1e-6


def diffusion_ddim(tab, out, x, t, nz, mask, mot):
    from oracle import diffusion
    r = diffusion.ddim_sample(tab, out.float(), x.float(), t, nz.float(), eta=0.5, inpainting=True, inpainting_mask=mask.float(),
                              inpainted_motion=mot.float())
    return r["sample"], r["pred_xstart"]


def test_fixture_recover_joints_against_the_reference_outputs_and_the_oracle():
    import os
    import glue_fixture as gf
    import mst_amd.synthetic as syn
    from conftest import GOLDEN, SEED
    from oracle import postprocess
    g = np.load(os.path.join(GOLDEN, "post.npz"))
    for tag in ("hml", "short", "j21"):
        F, T, J, B = (int(v) for v in g[f"{tag}|shape"])
        sample = syn.normal(SEED, f"post/{tag}/sample", (B, F, 1, T))
        mean = (syn.normal(SEED, f"post/{tag}/mean", (F,)) * 0.3).astype(np.float32)
        std = syn.uniform(SEED, f"post/{tag}/std", (F,), 0.2, 1.5).astype(np.float32)
        got = gf.recover_joints(sample, mean, std, J)
        assert got.shape == g[f"{tag}|joints"].shape
        # the goldens are the reference's own fp32 outputs: the bar test_postprocess.py holds the fp32 oracle to
        assert gf.rel(g[f"{tag}|joints"], got) < 2e-5, tag
        assert gf.rel(postprocess.recover_joints(sample, mean, std, J), got) < 2e-5, tag
    # T = 1 and T = 2: no running sum, one term
    one = gf.recover_joints(np.ones((1, 67, 1, 1), np.float32), np.zeros(67, np.float32), np.ones(67, np.float32), 22)
    assert one[0, 0, 0, 0].tolist() == [0.0, 1.0, 0.0] and np.all(one[0, 0, 0, 1:] == 1.0)
