"""Windowed sampling: what the stitch costs.  8 long clips x 1200 frames at the HumanML width (263 features), window 196, overlap 48:
8 windows a clip, 64 windows -- the benchmark's batch.  DDIM (eta 0) over a respaced schedule, root-horizontal inpainting pair,
same box, interleaved:

  (a) windows        -- mst_sample_loop_windows: every step enqueued from the host, the slice streams joined and k_window_stitch run
                        behind every step, the last stitch also the fold
  (b) independent    -- mst_sample_loop on the same 64 windows as independent clips, default settings (chained frame rows, fused embed)
  (c) independent, MST_FUSE_FRAMES=0 -- the same on an engine created with MST_FUSE_FRAMES=0: (a)'s launch sequence without the stitch
                        and the per-step join.  (a) - (c) is the feature's cost.

  (d) stochastic windows (only with --sampler ddpm, or --sampler ddim --eta != 0) -- mst_window_sample_loop reading buffer noise that
                        mst_window_noise drew in long-clip coordinates, in chunks bounded as GaussianDiffusion bounds them (64 steps,
                        256 MB); the fill is inside the timed region.  (d) - (a) is what the noise term costs over the deterministic
                        windowed loop of the same run: the fill, and the step's 4 bytes per element of buffer read.

(b) and (c) run the unchanged entry point.  One untimed warm-up loop each, then `--reps` loops each, alternating, timed with device
events around a synchronised call; medians.  Also: k_window_unfold and k_window_stitch (with the fold) alone, event-timed over `--kernel-reps`
launches; with (d) also k_window_noise alone, per step.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--respacing", default="100", help="timestep respacing of the 1000-step cosine schedule; every index is run")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--frames", type=int, default=1200)
    ap.add_argument("--window", type=int, default=196)
    ap.add_argument("--overlap", type=int, default=48)
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--sampler", choices=("ddim", "ddpm"), default="ddim", help="ddpm, or ddim with --eta != 0: also time leg (d)")
    ap.add_argument("--eta", type=float, default=0.0)
    args = ap.parse_args()
    import numpy as np
    import torch
    import mst_amd  # noqa: F401
    from mst_amd import synthetic as syn
    from mst_amd.diffusion.windows import WindowPlan, noise_windows, stitch_, unfold
    from mst_amd.engine import DenoiserEngine, Schedule, SAMPLER_DDIM, SAMPLER_DDPM
    from oracle import schedule

    dev = torch.device("cuda:0")
    F, C, L, W, O = 263, args.clips, args.frames, args.window, args.overlap
    plan = WindowPlan([L] * C, W, O, dev)
    N = plan.n_windows
    weights = {k: torch.from_numpy(v) for k, v in syn.denoiser_state(1, F).items()}
    pe = torch.from_numpy(syn.positional_table(5000, 512))

    def engine(fuse_frames):
        old = os.environ.get("MST_FUSE_FRAMES")
        if not fuse_frames:
            os.environ["MST_FUSE_FRAMES"] = "0"                     # read once, at engine creation
        try:
            eng = DenoiserEngine(F, W, N, device=dev)
        finally:
            if not fuse_frames:
                if old is None:
                    del os.environ["MST_FUSE_FRAMES"]
                else:
                    os.environ["MST_FUSE_FRAMES"] = old
        eng.load_state_dict(weights, pe=pe)
        return eng

    eng, eng_plain = engine(True), engine(False)
    tab, tmap = schedule.make("cosine", 1000, args.respacing)
    sch = Schedule(tab, tmap, dev)
    n = sch.num_steps
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    shp = (C, F, 1, L)
    x_long = cu(syn.normal(1, "x", shp))
    mask_long, motion_long = cu(syn.root_horizontal_mask(C, F, L)), cu(syn.normal(1, "motion", shp))
    x0, mask, motion = unfold(x_long, plan), unfold(mask_long, plan), unfold(motion_long, plan)
    txt = cu(syn.normal(1, "txt", (C, 512)))[plan.win_clip_tensor()]
    for e in (eng, eng_plain):
        e.set_text(txt)
    out_long = torch.empty(shp, device=dev)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    legs = {
        "windows": lambda: eng.sample_loop_windows(sch, x0.clone(), plan, n - 1, 0, mask=mask, motion=motion, fold_out=out_long),
        "independent": lambda: eng.sample_loop(sch, x0.clone(), n - 1, 0, SAMPLER_DDIM, eta=0.0, mask=mask, motion=motion, seed=0),
        "independent_fuse_frames_0": lambda: eng_plain.sample_loop(sch, x0.clone(), n - 1, 0, SAMPLER_DDIM, eta=0.0, mask=mask, motion=motion,
                                                                   seed=0),
    }
    noisy = args.sampler == "ddpm" or args.eta != 0.0
    chunk = max(1, min(64, (256 << 20) // (x0.numel() * 4)))       # GaussianDiffusion.noise_chunk / noise_chunk_bytes

    def stochastic():
        x = x0.clone()
        for c0 in range(0, n, chunk):
            k = min(chunk, n - c0)
            buf = noise_windows(plan, F, 1 + c0, 0, k)
            eng.window_sample_loop(sch, x, plan, n - 1 - c0, n - c0 - k, SAMPLER_DDPM if args.sampler == "ddpm" else SAMPLER_DDIM, args.eta,
                                   mask=mask, motion=motion, noise=buf, fold_out=out_long if c0 + k == n else None)
    if noisy:
        legs["windows_stochastic"] = stochastic
    for fn in legs.values():
        fn()
    ms = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}

    xs = x0.clone()
    xs += torch.randn_like(xs)                                      # windows that disagree: the stitch averages and stores
    stitch_(xs.clone(), plan, long_out=out_long)
    scratch = [xs.clone() for _ in range(args.kernel_reps)]         # a fresh copy a launch: a stitched copy agrees and would store nothing
    k_st = timed(lambda: [stitch_(w, plan, long_out=out_long) for w in scratch]) / args.kernel_reps
    del scratch
    k_un = timed(lambda: [unfold(x_long, plan) for _ in range(args.kernel_reps)]) / args.kernel_reps
    cost = med["windows"] - med["independent_fuse_frames_0"]
    extra = {}
    if noisy:
        def fills():
            for _ in range(args.kernel_reps):                       # (each buffer is dropped at once: the allocator hands the same block out again)
                noise_windows(plan, F, 1, 0, chunk)
        k_nz = timed(fills) / args.kernel_reps / chunk
        d = med["windows_stochastic"] - med["windows"]
        extra = {"sampler": args.sampler, "eta": args.eta, "noise_chunk_steps": chunk, "noise_fill_us_per_step": round(k_nz * 1e3, 2),
                 "noise_term_cost_ms_per_step": round(d / n, 4), "noise_term_cost_over_windows": round(d / med["windows"], 4)}
    print(json.dumps({
        "long_shape": list(shp), "window": W, "overlap": O, "windows": N, "slices": eng.loop_slices(N, False, W), "steps": n, "reps": args.reps,
        **{f"{k}_ms": round(v, 2) for k, v in med.items()}, **{f"{k}_all_ms": [round(t, 2) for t in v] for k, v in ms.items()},
        **{f"{k}_ms_per_step": round(v / n, 4) for k, v in med.items()},
        "feature_cost_ms_per_step": round(cost / n, 4), "feature_cost_over_fuse_frames_0": round(cost / med["independent_fuse_frames_0"], 4),
        "windows_over_independent": round(med["windows"] / med["independent"], 4),
        "long_frames_per_s": round(C * L / med["windows"] * 1e3, 1),
        "stitch_fold_us": round(k_st * 1e3, 2), "unfold_us": round(k_un * 1e3, 2), "windows_mb": round(xs.numel() * 4 / 1e6, 1), **extra}))


if __name__ == "__main__":
    main()
