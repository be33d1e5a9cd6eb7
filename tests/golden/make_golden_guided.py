"""Golden vectors of the reference's guided samplers (cond_fn: diffusion/gaussian_diffusion.py:454-506, :577-580, :821-824,
diffusion/inpainting_gaussian_diffusion.py:59-62, :150-153, diffusion/respace.py:104-108) -> tests/golden/guided.npz.

Runs ONLY in the authoring container (reference mounted read-only at /root/reference), on the CPU, with make_golden.py's shims,
seeded weights and text embedding:

    python tests/golden/make_golden_guided.py

Every input is rebuilt by the tests from its seed (tests/guide_fixture.py); only the reference's outputs are stored.  The cond_fn is
the target guide's formula written out here: g = w m (a_t y - x_t), y a seeded target (20 x standard normal), m ones on a few feature rows, a_t = 1 or
sqrt(alphas_cumprod[t]) of the ORIGINAL 1000-step process at the timestep the cond_fn receives (under SpacedDiffusion: timestep_map[t]).

  * single steps, one clip: p_sample, ddim_sample(eta 0) and ddim_sample(eta 0.5) of plain SpacedDiffusion (no inpainting pair) and of
    InpaintingGaussianDiffusion (with the pair), both a_t modes, recorded noise; Xia shape (181, 1, 76) under respacings "", "100",
    "ddim20" at index 0, an interior index and the last index; HumanML shape (263, 1, 196) once under "ddim20".  The x0-hat does not
    depend on the sampler or the guide (asserted here) and is stored once per case.  Outputs are kept at every feature of every
    STRIDE-th frame, as make_golden_plms.py keeps them.
  * one epsilon-model and one previous-x case (Xia, "ddim20", index 10, SpacedDiffusion with that ModelMeanType around the same net).
  * whole 20-step loops under "ddim20" (Xia, plain SpacedDiffusion, a_t following the schedule): guided ddim_sample_loop(eta 0) and
    p_sample_loop, and the unguided loops from the same noise.  Asserted: guided and unguided differ by >= 0.05 relative L2.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden import SEED, syn  # noqa: E402

PROMPT = "a person walks proudly"
SHAPES = {"xia": (181, 76), "hml": (263, 196)}
STRIDE = {"xia": 19, "hml": 49}
INDICES = {"": (0, 500, 999), "100": (0, 50, 99), "ddim20": (0, 10, 19)}
SAMPLERS = {"ddpm": None, "ddim0": 0.0, "ddim0.5": 0.5}
GUIDE_ROWS = slice(3, 12)
WEIGHT = 2.5
TARGET_SCALE = 20.0      # the target's magnitude: late in the schedule variance_t is small, so the pull has to be long for the ancestral loop to move
MOVED = 0.05


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def main():
    mg.install_shims()
    gd = importlib.import_module("diffusion.gaussian_diffusion")
    rs = importlib.import_module("diffusion.respace")
    igd = importlib.import_module("diffusion.inpainting_gaussian_diffusion")
    mdm = importlib.import_module("model.mdm_forstyledataset")
    mu = importlib.import_module("utils.model_util")
    sqrt_ac = torch.from_numpy(np.sqrt(np.cumprod(1.0 - gd.get_named_beta_schedule("cosine", 1000))))      # the ORIGINAL process
    out = {}

    def cond_fn_of(target, gmask, follow):
        def cond_fn(x, t, **kwargs):
            a = sqrt_ac[t].float().view(-1, 1, 1, 1) if follow else 1.0
            return (WEIGHT * gmask) * (a * target - x)
        return cond_fn

    def step(d, sampler, model, x, t, kw, cond_fn, tag):
        with torch.no_grad(), mg.recorded_noise(tag):
            if SAMPLERS[sampler] is None:
                return d.p_sample(model, x, torch.tensor([t]), clip_denoised=False, cond_fn=cond_fn, model_kwargs=kw)
            return d.ddim_sample(model, x, torch.tensor([t]), clip_denoised=False, cond_fn=cond_fn, model_kwargs=kw, eta=SAMPLERS[sampler])

    for tag, (F, T) in SHAPES.items():
        model = mg.build_reference_model(mdm, F)
        shp = (1, F, 1, T)
        x = torch.from_numpy(syn.normal(SEED, f"guided/{tag}/x", shp))
        mask = torch.from_numpy(syn.root_horizontal_mask(1, F, T))
        motion = torch.from_numpy(syn.normal(SEED, f"guided/{tag}/motion", shp))
        target = torch.from_numpy(TARGET_SCALE * syn.normal(SEED, f"guided/{tag}/target", shp))
        gmask = torch.zeros(shp)
        gmask[:, GUIDE_ROWS] = 1
        y = {"text": [PROMPT], "mask": torch.ones(1, 1, 1, T)}
        keep = lambda a: a.numpy()[..., ::STRIDE[tag]].copy()
        cases = [(resp, t, v) for resp in ("", "100", "ddim20") for t in INDICES[resp] for v in (0, 1)] if tag == "xia" else [("ddim20", 10, 1)]
        for resp, t, variant in cases:
            d = mu.create_gaussian_diffusion(mg.args_for(), igd.InpaintingGaussianDiffusion if variant else rs.SpacedDiffusion, resp)
            kw = {"y": {**y, "inpainting_mask": mask, "inpainted_motion": motion}} if variant else {"y": dict(y)}
            key = f"{tag}|{resp}|{t}|{variant}"
            for sampler in SAMPLERS:
                plain = step(d, sampler, model, x, t, kw, None, f"guided/{key}")
                for follow in (0, 1):
                    r = step(d, sampler, model, x, t, kw, cond_fn_of(target, gmask, follow), f"guided/{key}")
                    assert torch.equal(r["pred_xstart"], plain["pred_xstart"]), "x0-hat depends on the guide"
                    out[f"{key}|{sampler}|{follow}|sample"] = keep(r["sample"])
                out.setdefault(f"{key}|pred_xstart", keep(plain["pred_xstart"]))
                assert np.array_equal(out[f"{key}|pred_xstart"], keep(plain["pred_xstart"]))
            print(key, flush=True)
        if tag != "xia":
            continue
        for name, mt in (("eps", gd.ModelMeanType.EPSILON), ("prevx", gd.ModelMeanType.PREVIOUS_X)):
            d = rs.SpacedDiffusion(use_timesteps=rs.space_timesteps(1000, "ddim20"), betas=gd.get_named_beta_schedule("cosine", 1000),
                                   model_mean_type=mt, model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE)
            for sampler in ("ddpm", "ddim0.5"):
                r = step(d, sampler, model, x, 10, {"y": dict(y)}, cond_fn_of(target, gmask, 1), f"guided/xia|{name}")
                out[f"xia|{name}|{sampler}|sample"] = keep(r["sample"])
                out[f"xia|{name}|pred_xstart"] = keep(r["pred_xstart"])
            print(name, flush=True)
        d = mu.create_gaussian_diffusion(mg.args_for(), rs.SpacedDiffusion, "ddim20")
        noise = torch.from_numpy(syn.normal(SEED, "guided/xia/xT", shp))
        kw = {"y": dict(y)}
        for kind, cf in (("plain", None), ("guided", cond_fn_of(target, gmask, 1))):
            with torch.no_grad():
                with mg.recorded_noise("guided/xia/ddim"):             # (eta = 0: the draws are multiplied by sigma = 0)
                    s = d.ddim_sample_loop(model, shp, noise=noise.clone(), clip_denoised=False, cond_fn=cf, model_kwargs=kw, eta=0.0)
                out[f"xia|loop20|ddim|{kind}"] = s.numpy().copy()
                with mg.recorded_noise("guided/xia/ddpm"):
                    s = d.p_sample_loop(model, shp, noise=noise.clone(), clip_denoised=False, cond_fn=cf, model_kwargs=kw)
                out[f"xia|loop20|ddpm|{kind}"] = s.numpy().copy()
            print("loops", kind, flush=True)
        for smp in ("ddim", "ddpm"):
            moved = rel_l2(out[f"xia|loop20|{smp}|guided"], out[f"xia|loop20|{smp}|plain"])
            print(f"{smp}: guided vs unguided loop {moved:.3f} relative L2")
            assert np.isfinite(out[f"xia|loop20|{smp}|guided"]).all() and moved >= MOVED, (smp, moved)
    path = os.path.join(HERE, "guided.npz")
    np.savez_compressed(path, **out)
    print("guided.npz", os.path.getsize(path) // 1024, "KiB,", len(out), "arrays")


if __name__ == "__main__":
    main()
