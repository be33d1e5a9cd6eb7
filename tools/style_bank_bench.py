"""Several styles in one batch: clips/s of a 1000-step DDPM loop at the HumanML shape (263 x 196), 8 styles x 8 clips.

  (a) mixed   -- the 64 clips (style i % 8 for clip i) as ONE batch-64 loop through a style bank (csrc/mst_style.h)
  (b) ceiling -- the same 64 clips all on one style through the single-style kernels (the headline batch-64 path)
  (c) looped  -- eight per-style batch-8 loops back to back, one engine per style: what a user runs without a bank

Each run: one untimed warm-up call, then `--steps` denoise steps timed with device events around a synchronised call (in-kernel
Philox noise), repeated `--reps` times; the median step time is scaled to 1000 steps.  Prints one JSON line.
(a) orders its segments / clips XCD-affine by default; MST_STYLE_XCD=0 runs it in plain order (the A/B of that placement)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--styles", type=int, default=8)
    ap.add_argument("--clips", type=int, default=8, help="clips per style")
    args = ap.parse_args()
    import numpy as np
    import torch
    import mst_amd  # noqa: F401
    from mst_amd import synthetic as syn
    from mst_amd.engine import DenoiserEngine, Schedule, SAMPLER_DDPM, LAYER_TENSORS
    from oracle import schedule

    dev = torch.device("cuda:0")
    F, T, K, C = 263, 196, args.styles, args.clips
    B = K * C
    pe = torch.from_numpy(syn.positional_table(5000, 512))
    prior = syn.denoiser_state(1, F)
    weights = []
    for s in range(K):
        w = syn.denoiser_state(100 + s, F)
        w.update({k: v for k, v in prior.items() if not k.startswith("seqTransEncoder.")})
        weights.append(w)

    def engine(rows, w):
        e = DenoiserEngine(F, T, rows, device=dev)
        e.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, pe=pe)
        return e

    tab, tmap = schedule.make("cosine", 1000, "")
    sch = Schedule(tab, tmap, dev)
    x0 = torch.from_numpy(syn.normal(1, "x", (B, F, 1, T))).to(dev)
    txt = torch.from_numpy(syn.normal(1, "txt", (B, 512))).to(dev)

    bank = engine(B, weights[0])
    bank.style_slots(K)
    for s in range(1, K):
        bank.load_layers_slot(s, [torch.from_numpy(weights[s][f"seqTransEncoder.layers.{i}.{k}"]).to(dev) for i in range(8) for k in LAYER_TENSORS])
    solo = [engine(C, weights[s]) for s in range(K)]
    torch.cuda.synchronize()

    def loop(calls):
        """calls: [(engine, x slice)]: every loop of one timed run, back to back."""
        xs = [x.clone() for _, x in calls]
        for (e, _), x in zip(calls, xs):
            e.sample_loop(sch, x, args.steps - 1, 0, SAMPLER_DDPM, seed=5)

    def timed(setup, calls):
        setup()
        loop(calls)                                   # warm-up (per-kernel LDS opt-ins, first-touch)
        torch.cuda.synchronize()
        per_step = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            loop(calls)
            b.record()
            b.synchronize()
            per_step.append(a.elapsed_time(b) / 1e3 / args.steps)
        med = statistics.median(per_step)
        return {"clips_per_s": round(B / (med * 1000), 3), "ms_per_step": round(med * 1e3, 4),
                "ms_per_step_range": [round(min(per_step) * 1e3, 4), round(max(per_step) * 1e3, 4)]}

    def mixed_setup():
        bank.set_text(txt)
        bank.set_styles([i % K for i in range(B)])

    def ceiling_setup():
        bank.set_text(txt)
        bank.set_styles(None)                         # the single-style kernels

    def looped_setup():
        for s in range(K):
            solo[s].set_text(txt[s * C:(s + 1) * C])

    res = {"mixed": timed(mixed_setup, [(bank, x0)]),
           "ceiling": timed(ceiling_setup, [(bank, x0)]),
           "looped": timed(looped_setup, [(solo[s], x0[s * C:(s + 1) * C]) for s in range(K)])}
    line = {"metric": f"style bank clips/sec (1000-step DDPM, {K} styles x {C} clips, Bx263x196)",
            "styles": K, "clips_per_style": C, "steps_timed": args.steps, "reps": args.reps,
            "xcd_affine": os.environ.get("MST_STYLE_XCD", "1") not in ("", "0"),
            **res,
            "mixed_over_looped": round(res["mixed"]["clips_per_s"] / res["looped"]["clips_per_s"], 3),
            "mixed_over_ceiling": round(res["mixed"]["clips_per_s"] / res["ceiling"]["clips_per_s"], 3)}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
