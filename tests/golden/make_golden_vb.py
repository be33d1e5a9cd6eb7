"""Golden vectors of the reference's variational-bound evaluation (diffusion/gaussian_diffusion.py:1281-1314 `_vb_terms_bpd`,
:1529-1545 `_prior_bpd`, :1547-1602 `calc_bpd_loop`) -> tests/golden/vb.npz.

Runs only where the reference checkout is mounted (make_golden.REF), on the CPU, with make_golden.py's shims, seeded weights, text
embedding and `recorded_noise`:

    python tests/golden/make_golden_vb.py

Every input is rebuilt by the tests from its seed (tests/vb_fixture.py: `golden_inputs`, `golden_noise`); only the reference's outputs
are stored, all of them small per-(clip, t) arrays:

  * CASES (tests/vb_fixture.py has the same table): the Xia shape (181, 1, 76);
      "ddim20|c1", "ddim20|c0"   SpacedDiffusion "ddim20", FIXED_SMALL, N = 2 clips of lengths 76 and 40, clip_denoised on / off
      "full|c0"                  the full 1000-step process, N = 1 clip, clip_denoised off
      "large|c0"                 "ddim20" under FIXED_LARGE (sigma_small = False), N = 2, clip_denoised off
  * per case the five outputs of calc_bpd_loop (column 0 is t = T - 1: the reference appends while t descends), and from a recording
    wrapper around `_vb_terms_bpd`: `rms` [N, T], the root mean square of every step's pred_xstart (same column order), and
    `pred|<t>` = pred_xstart itself at t in {0, an interior index, T - 1}, every feature of every 19th frame.
  * the k-th `randn_like` of the loop (k = 0 at t = T - 1) is `syn.normal(SEED, "vb/<case>/noise/<k>")`."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden import SEED, syn  # noqa: E402

PROMPTS = ["a person walks proudly", "an old man jumps"]
F, T = 181, 76
LENGTHS = (76, 40)
STRIDE = 19
X_SCALE = 0.6          # x_start = 0.6 * normal: about one element in ten lies beyond +-0.999, so the decoder term takes all three branches
# case -> (respacing, sigma_small, clips, clip_denoised)
CASES = {"ddim20|c1": ("ddim20", True, 2, True), "ddim20|c0": ("ddim20", True, 2, False), "full|c0": ("", True, 1, False),
         "large|c0": ("ddim20", False, 2, False)}


def main():
    mg.install_shims()
    rs = importlib.import_module("diffusion.respace")
    mdm = importlib.import_module("model.mdm_forstyledataset")
    mu = importlib.import_module("utils.model_util")
    model = mg.build_reference_model(mdm, F)
    out = {}
    for case, (resp, small, n, clip) in CASES.items():
        args = mg.args_for()
        args.sigma_small = small
        d = mu.create_gaussian_diffusion(args, rs.SpacedDiffusion, resp)
        steps = d.num_timesteps
        x = torch.from_numpy(X_SCALE * syn.normal(SEED, "vb/x", (2, F, 1, T))[:n])
        lengths = torch.tensor(LENGTHS[:n])
        y = {"text": PROMPTS[:n], "lengths": lengths, "mask": (torch.arange(T)[None] < lengths[:, None]).view(n, 1, 1, T)}
        keep_t = (0, steps // 2, steps - 1)
        preds = []
        orig = d._vb_terms_bpd

        def recording(*a, **k):
            r = orig(*a, **k)
            preds.append(r["pred_xstart"].detach().clone())
            return r

        d._vb_terms_bpd = recording
        with mg.recorded_noise(f"vb/{case}"):
            r = d.calc_bpd_loop(model, x, clip_denoised=clip, model_kwargs={"y": y})
        assert len(preds) == steps
        for k in ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse"):
            out[f"{case}|{k}"] = r[k].numpy().copy()
        out[f"{case}|rms"] = torch.stack([p.double().pow(2).mean(dim=(1, 2, 3)).sqrt() for p in preds], dim=1).float().numpy()
        for t in keep_t:
            out[f"{case}|pred|{t}"] = preds[steps - 1 - t].numpy()[..., ::STRIDE].copy()
        print(case, "total_bpd", r["total_bpd"].numpy(), flush=True)
    path = os.path.join(HERE, "vb.npz")
    np.savez_compressed(path, **out)
    print("vb.npz", os.path.getsize(path) // 1024, "KiB,", len(out), "arrays")


if __name__ == "__main__":
    main()
