"""Golden vectors of the reference's `ddim_reverse_sample` (diffusion/gaussian_diffusion.py:910-946) -> tests/golden/reverse.npz.

Runs ONLY in the authoring container (reference mounted read-only at /root/reference), on the CPU, with make_golden.py's shims,
seeded weights and text embedding:

    python tests/golden/make_golden_reverse.py

Every input is rebuilt by the tests from its seed (tests/reverse_fixture.py: `golden_inputs`); only the reference's outputs are stored.

  * single steps, one clip each: Xia shape (181, 1, 76) under respacings "", "100", "ddim20" at index 0, an interior index and the
    last index, with and without the inpainting pair; HumanML shape (263, 1, 196) under "ddim20" only.  To keep the file well under a
    megabyte a step's two outputs are stored at every feature of every STRIDE-th frame (Xia: frames 0, 7, .., 70; HumanML: 0, 17, ..,
    187) -- the inputs are whole clips, and every stored value depends on all of them through the attention.
  * `xia|inv20|latent`: a full 20-step ddim20 inversion made by looping that method over t = 0 .. 19 (whole clip), and
    `xia|inv20|decoded`: that latent through the reference's `ddim_sample_loop(noise=latent, eta=0)` (whole clip).  Both on the plain
    SpacedDiffusion (no inpainting pair: InpaintingGaussianDiffusion.ddim_sample wants a mask even where it blends nothing).
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
STRIDE = {"xia": 7, "hml": 17}
INDICES = {"": (0, 500, 999), "100": (0, 50, 99), "ddim20": (0, 10, 19)}
RESPACINGS = {"xia": ("", "100", "ddim20"), "hml": ("ddim20",)}


def main():
    mg.install_shims()
    rs = importlib.import_module("diffusion.respace")
    igd = importlib.import_module("diffusion.inpainting_gaussian_diffusion")
    mdm = importlib.import_module("model.mdm_forstyledataset")
    mu = importlib.import_module("utils.model_util")
    out = {}
    for tag, (F, T) in SHAPES.items():
        model = mg.build_reference_model(mdm, F)
        shp = (1, F, 1, T)
        x = torch.from_numpy(syn.normal(SEED, f"rev/{tag}/x", shp))
        mask = torch.from_numpy(syn.root_horizontal_mask(1, F, T))
        motion = torch.from_numpy(syn.normal(SEED, f"rev/{tag}/motion", shp))
        y = {"text": [PROMPT], "mask": torch.ones(1, 1, 1, T)}
        for resp in RESPACINGS[tag]:
            d = mu.create_gaussian_diffusion(mg.args_for(), igd.InpaintingGaussianDiffusion, resp)
            for t in INDICES[resp]:
                for pair in (0, 1):
                    kw = {"y": {**y, "inpainting_mask": mask, "inpainted_motion": motion}} if pair else {"y": dict(y)}
                    with torch.no_grad():
                        r = d.ddim_reverse_sample(model, x, torch.tensor([t]), clip_denoised=False, model_kwargs=kw)
                    for k in ("sample", "pred_xstart"):
                        out[f"{tag}|{resp}|{t}|{pair}|{k}"] = r[k].numpy()[..., ::STRIDE[tag]].copy()
        if tag == "xia":
            d = mu.create_gaussian_diffusion(mg.args_for(), rs.SpacedDiffusion, "ddim20")
            img = torch.from_numpy(syn.normal(SEED, "rev/xia/content", shp))
            kw = {"y": dict(y)}
            with torch.no_grad():
                for t in range(20):
                    img = d.ddim_reverse_sample(model, img, torch.tensor([t]), clip_denoised=False, model_kwargs=kw)["sample"]
                out["xia|inv20|latent"] = img.numpy().copy()
                with mg.recorded_noise("rev/xia/decode"):          # (eta = 0: the draws are multiplied by sigma = 0)
                    dec = d.ddim_sample_loop(model, shp, noise=img, clip_denoised=False, model_kwargs=kw, eta=0.0)
                out["xia|inv20|decoded"] = dec.numpy().copy()
    path = os.path.join(HERE, "reverse.npz")
    np.savez_compressed(path, **out)
    print("reverse.npz", os.path.getsize(path) // 1024, "KiB,", len(out), "arrays")


if __name__ == "__main__":
    main()
