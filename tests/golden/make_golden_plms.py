"""Golden vectors of the reference's PLMS sampler (diffusion/gaussian_diffusion.py:1084-1279) -> tests/golden/plms.npz.

Runs ONLY in the authoring container (reference mounted read-only at /root/reference), on the CPU, with make_golden.py's shims,
seeded weights and text embedding:

    python tests/golden/make_golden_plms.py [--only steps,euler,loops]      (--only: recompute those groups, keep the rest of the file)

Every input is rebuilt by the tests from its seed (tests/plms_fixture.py: `golden_inputs`); only the reference's outputs are stored.

  * single multistep steps, one clip each: `plms_sample(order=c, old_out={"old_eps": seeded history of c - 1 entries})` for
    c = 1 .. 4 -- Xia shape (181, 1, 76) under respacings "", "100", "ddim20" at index 0, an interior index and the last index, with
    and without the inpainting pair; HumanML shape (263, 1, 196) under "ddim20" only.  A step's x0-hat does not depend on c, so it is
    stored once per (shape, respacing, index, pair) and the sample once per c.  To keep the file under a megabyte the outputs are
    stored at every feature of every STRIDE-th frame (Xia: frames 0, 19, 38, 57; HumanML: 0, 49, 98, 147) -- the inputs are whole
    clips, and every stored value depends on all of them through the attention.
  * first steps of a chain (`old_out=None`, order 2: the two-evaluation Pseudo Improved Euler step) at an interior index and the last
    index of "ddim20", both shapes, with and without the pair: sample, x0-hat, the eps the history takes and the model's raw output
    of the SECOND evaluation (`out2`, recorded by a wrapper around the model: plms_sample does not return it), strided the same way.
  * whole 20-step `plms_sample_loop` clips at orders 2, 3 and 4 (Xia, plain SpacedDiffusion, no pair) and, from the same noise, the
    reference's `ddim_sample_loop(eta=0)`: the yardstick of the whole-loop test.
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
RESPACINGS = {"xia": ("", "100", "ddim20"), "hml": ("ddim20",)}
EULER_INDICES = (10, 19)


def main(groups=("steps", "euler", "loops")):
    mg.install_shims()
    rs = importlib.import_module("diffusion.respace")
    igd = importlib.import_module("diffusion.inpainting_gaussian_diffusion")
    mdm = importlib.import_module("model.mdm_forstyledataset")
    mu = importlib.import_module("utils.model_util")
    path = os.path.join(HERE, "plms.npz")
    out = dict(np.load(path)) if set(groups) != {"steps", "euler", "loops"} else {}      # (--only: the other groups stay as they are)
    for tag, (F, T) in SHAPES.items():
        model = mg.build_reference_model(mdm, F)
        shp = (1, F, 1, T)
        x = torch.from_numpy(syn.normal(SEED, f"plms/{tag}/x", shp))
        mask = torch.from_numpy(syn.root_horizontal_mask(1, F, T))
        motion = torch.from_numpy(syn.normal(SEED, f"plms/{tag}/motion", shp))
        hist = [torch.from_numpy(syn.normal(SEED, f"plms/{tag}/h{k}", shp)) for k in (1, 2, 3)]      # h1 newest .. h3 oldest
        y = {"text": [PROMPT], "mask": torch.ones(1, 1, 1, T)}
        keep = lambda a: a.numpy()[..., ::STRIDE[tag]].copy()
        for resp in RESPACINGS[tag]:
            d = mu.create_gaussian_diffusion(mg.args_for(), igd.InpaintingGaussianDiffusion, resp)
            for t in INDICES[resp] if "steps" in groups else ():
                for pair in (0, 1):
                    kw = {"y": {**y, "inpainting_mask": mask, "inpainted_motion": motion}} if pair else {"y": dict(y)}
                    for c in (1, 2, 3, 4):
                        old = [h.clone() for h in hist[:c - 1]][::-1]                                # oldest first, as old_eps holds them
                        with torch.no_grad():
                            r = d.plms_sample(model, x, torch.tensor([t]), clip_denoised=False, model_kwargs=kw, order=c,
                                              old_out={"old_eps": old})
                        assert len(r["old_eps"]) == c - 1
                        out[f"{tag}|{resp}|{t}|{pair}|{c}|sample"] = keep(r["sample"])
                        if c == 1:
                            out[f"{tag}|{resp}|{t}|{pair}|pred_xstart"] = keep(r["pred_xstart"])
                    print(tag, resp, t, pair, flush=True)
            if resp == "ddim20" and "euler" in groups:
                for t in EULER_INDICES:
                    for pair in (0, 1):
                        kw = {"y": {**y, "inpainting_mask": mask, "inpainted_motion": motion}} if pair else {"y": dict(y)}
                        raw = []

                        def recording(xx, ts, **k):
                            raw.append(model(xx, ts, **k))
                            return raw[-1]

                        with torch.no_grad():
                            r = d.plms_sample(recording, x, torch.tensor([t]), clip_denoised=False, model_kwargs=kw, order=2, old_out=None)
                        assert len(r["old_eps"]) == 1 and len(raw) == 2
                        out[f"{tag}|euler|{t}|{pair}|sample"] = keep(r["sample"])
                        out[f"{tag}|euler|{t}|{pair}|pred_xstart"] = keep(r["pred_xstart"])
                        out[f"{tag}|euler|{t}|{pair}|eps"] = keep(r["old_eps"][0])
                        out[f"{tag}|euler|{t}|{pair}|out2"] = keep(raw[1])      # the model at (x_mid, t - 1), before the blend
                    print(tag, "euler", t, flush=True)
        if tag == "xia" and "loops" in groups:
            d = mu.create_gaussian_diffusion(mg.args_for(), rs.SpacedDiffusion, "ddim20")
            noise = torch.from_numpy(syn.normal(SEED, "plms/xia/noise", shp))
            kw = {"y": dict(y)}
            with torch.no_grad():
                for order in (2, 3, 4):
                    s = d.plms_sample_loop(model, shp, noise=noise.clone(), clip_denoised=False, model_kwargs=kw, order=order)
                    out[f"xia|loop20|plms{order}"] = s.numpy().copy()
                    print("loop order", order, flush=True)
                with mg.recorded_noise("plms/xia/ddim"):               # (eta = 0: the draws are multiplied by sigma = 0)
                    s = d.ddim_sample_loop(model, shp, noise=noise.clone(), clip_denoised=False, model_kwargs=kw, eta=0.0)
                out["xia|loop20|ddim"] = s.numpy().copy()
    np.savez_compressed(path, **out)
    print("plms.npz", os.path.getsize(path) // 1024, "KiB,", len(out), "arrays")


if __name__ == "__main__":
    main(tuple(sys.argv[sys.argv.index("--only") + 1].split(",")) if "--only" in sys.argv else ("steps", "euler", "loops"))
