"""The variational-bound evaluation: what packing (clip, timestep) rows buys.  `calc_bpd_loop` over the full 1000-step process at the
HumanML shape (263 x 196), in-kernel Philox noise, an engine-backed model callable, same box, interleaved:

  (a) default rows -- whole timesteps of all N clips up to 64 rows a model call (1 clip: 16 calls of 64 rows)
  (b) rows = N     -- the reference's loop structure on the same kernels (1000 calls of N rows)

for N = 1 and N = 8 clips; one untimed warm-up of each, then `--reps` loops each, alternating, timed with device events around a
synchronised call; medians.  Then the terms kernel alone (one workgroup per row) against the model call it follows, at 64 rows and at
1 row: `--reps` medians of the mean of `--inner` back-to-back launches.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", type=int, default=1000, help="timesteps of the process (1000: the full one)")
    args = ap.parse_args()
    import numpy as np
    import torch
    import mst_amd  # noqa: F401
    from mst_amd import synthetic as syn
    from mst_amd.diffusion import gaussian_diffusion as gd
    from mst_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    from mst_amd.engine import DenoiserEngine

    dev = torch.device("cuda:0")
    F, T, R = 263, 196, 64
    eng = DenoiserEngine(F, T, R, device=dev)
    eng.load_state_dict({k: torch.from_numpy(v) for k, v in syn.denoiser_state(1, F).items()}, pe=torch.from_numpy(syn.positional_table(5000, 512)))
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = SpacedDiffusion(use_timesteps=space_timesteps(1000, [args.steps]), betas=gd.get_named_beta_schedule("cosine", 1000),
                        model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE)

    def model(x, t, y=None):                    # what an engine-backed denoiser does per call: the rows' text, then the forward
        eng.set_text(y["text_embed"])
        return eng.forward(x, t)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    out = {"shape": [F, 1, T], "steps": d.num_timesteps, "reps": args.reps}
    for n in (1, 8):
        x = cu(0.6 * syn.normal(1, f"x{n}", (n, F, 1, T)))
        kw = {"y": {"text_embed": cu(syn.normal(1, "txt", (n, 512))), "mask": torch.ones(n, 1, 1, T, device=dev)}}
        run = {"default": lambda: d.calc_bpd_loop(model, x, model_kwargs=kw, seed=5),
               "rows_n": lambda: d.calc_bpd_loop(model, x, model_kwargs=kw, seed=5, rows=n)}
        for f in run.values():
            f()
        ms = {k: [] for k in run}
        for _ in range(args.reps):
            for k, f in run.items():
                ms[k].append(timed(f))
        med = {k: statistics.median(v) for k, v in ms.items()}
        out[f"clips{n}"] = {"default_rows": max(n, 64 // n * n), "default_ms": round(med["default"], 1), "rows_n_ms": round(med["rows_n"], 1),
                            "rows_n_over_default": round(med["rows_n"] / med["default"], 2),
                            "default_all_ms": [round(v, 1) for v in ms["default"]], "rows_n_all_ms": [round(v, 1) for v in ms["rows_n"]]}

    # the terms kernel alone against the model call in front of it
    sch = d._schedule(dev)
    tlv = d._vb_true_logvar(dev)
    x = cu(0.6 * syn.normal(1, "x8", (8, F, 1, T)))
    for rows in (64, 1):
        clip = torch.arange(rows, device=dev) % 8
        t = (torch.arange(rows, device=dev) * 15 + 3) % d.num_timesteps
        x_t = sch.vb_diffuse(x, clip, t, seed=5)
        eng.set_text(cu(syn.normal(1, "txt", (rows, 512))))
        mo = eng.forward(x_t, t)
        z = torch.randn_like(x_t)
        fns = {"terms_draw": lambda: sch.vb_terms(tlv, x, x_t, mo, clip, t, seed=5),
               "terms_buffer": lambda: sch.vb_terms(tlv, x, x_t, mo, clip, t, noise=z),
               "diffuse_draw": lambda: sch.vb_diffuse(x, clip, t, seed=5),
               "model": lambda: eng.forward(x_t, t)}
        for f in fns.values():
            f()
        ms = {k: [] for k in fns}
        for _ in range(args.reps):
            for k, f in fns.items():
                ms[k].append(timed(lambda: [f() for _ in range(args.inner)]) / args.inner)
        out[f"rows{rows}_us"] = {k: round(statistics.median(v) * 1e3, 1) for k, v in ms.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
