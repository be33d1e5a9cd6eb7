"""Guided sampling: what the guide costs.  1000-step DDPM loops at the HumanML shape (263 x 196), batch 64, root-horizontal inpainting
mask, in-kernel Philox noise, same box, interleaved:

  (a) unguided  -- mst_sample_loop (the headline path)
  (b) target    -- mst_sample_loop_guided with MST_GUIDE_TARGET (target + mask + per-clip weight, a_t following the schedule): the
                   step kernel reads two more fp32 tensors a step
  (c) callback  -- the path an arbitrary Python cond_fn takes: TargetGuide.__call__ in torch on x_t, then a ONE-step
                   mst_sample_loop_guided with MST_GUIDE_GRADIENT, per step (no native loop, no graph)

(a) and (b): one untimed warm-up loop, then `--reps` full loops each, alternating, timed with device events around a synchronised
call; medians.  (c): `--cb-steps` steps after a warm-up of 10.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--denoise-steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--cb-steps", type=int, default=100)
    args = ap.parse_args()
    import numpy as np
    import torch
    import mst_amd  # noqa: F401
    from mst_amd import synthetic as syn
    from mst_amd.diffusion.guidance import TargetGuide
    from mst_amd.engine import DenoiserEngine, Schedule, SAMPLER_DDPM, guide_args
    from oracle import schedule

    dev = torch.device("cuda:0")
    F, T, B, n = 263, 196, args.batch, args.denoise_steps
    eng = DenoiserEngine(F, T, B, device=dev)
    eng.load_state_dict({k: torch.from_numpy(v) for k, v in syn.denoiser_state(1, F).items()}, pe=torch.from_numpy(syn.positional_table(5000, 512)))
    tab, tmap = schedule.make("cosine", 1000, "")
    sch = Schedule(tab, tmap, dev)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    shp = (B, F, 1, T)
    x0, txt = cu(syn.normal(1, "x", shp)), cu(syn.normal(1, "txt", (B, 512)))
    mask, motion = cu(syn.root_horizontal_mask(B, F, T)), cu(syn.normal(1, "motion", shp))
    target = cu(syn.normal(1, "target", shp))
    gmask = torch.zeros(shp, device=dev)
    gmask[:, 3:12] = 1
    weight = torch.full((B,), 2.0, device=dev)
    eng.set_text(txt)
    ga = guide_args(x0, target=target, mask=gmask, weight=weight, follow_schedule=True)
    guide = TargetGuide(target, mask=gmask, weight=weight, alphas_cumprod=tab["alphas_cumprod"])

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def loop(g):
        return eng.sample_loop(sch, x0.clone(), n - 1, 0, SAMPLER_DDPM, mask=mask, motion=motion, seed=5, guide=g)

    loop(None), loop(ga)
    ms = {"unguided": [], "target": []}
    for _ in range(args.reps):
        ms["unguided"].append(timed(lambda: loop(None)))
        ms["target"].append(timed(lambda: loop(ga)))
    un, tg = statistics.median(ms["unguided"]), statistics.median(ms["target"])

    x = x0.clone()

    def callback_steps(k, t0):
        for j in range(k):
            t = t0 - j
            g = guide(x, torch.full((B,), t, device=dev))
            eng.sample_loop(sch, x, t, t, SAMPLER_DDPM, mask=mask, motion=motion, seed=5 + j, guide=guide_args(x, grad=g))

    callback_steps(10, n - 1)
    cb = timed(lambda: callback_steps(args.cb_steps, n - 11)) / args.cb_steps
    print(json.dumps({"shape": [B, F, 1, T], "denoise_steps": n, "reps": args.reps,
                      "unguided_ms": round(un, 1), "unguided_clips_per_s": round(B / un * 1e3, 2), "unguided_all_ms": [round(v, 1) for v in ms["unguided"]],
                      "target_guided_ms": round(tg, 1), "target_guided_clips_per_s": round(B / tg * 1e3, 2), "target_all_ms": [round(v, 1) for v in ms["target"]],
                      "target_over_unguided": round(tg / un, 4), "unguided_ms_per_step": round(un / n, 4), "target_ms_per_step": round(tg / n, 4),
                      "callback_ms_per_step": round(cb, 4), "callback_steps": args.cb_steps}))


if __name__ == "__main__":
    main()
