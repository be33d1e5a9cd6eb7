"""The evaluator path: what scoring generated clips costs on the GPU.  Seeded weights at the real widths (tests/eval_fixture.py):

  embed      1024 clips x (263, 1, 196) in the samplers' layout, embedded in batches of 32 with the renormalising affine
  stats      on those 1024 x 512 embeddings: activation statistics of them and of the same clips embedded without the affine, and
             the Frechet distance of the two (the matrix square root on the host, timed apart), R-precision top-3 over 32 batches
             of 32, matching score, diversity of 300 pairs
  families   one batch of 32 clips x 196 frames, each kernel family on its own: the two conv GEMMs, out_net + input_emb, the GRU's input
             projections (N = 6144), the 49-step recurrence, the output net (two Linears around LayerNorm); then the distance + rank
             kernel at 32 x 32 and 1024 x 1024, the double covariance at 1024 x 512, 1024 pair norms

Each is event-timed: the calls between two device events, the median of `--reps` (10) after `--warmup` untimed runs.  Next to them the
seconds the reference's own modules took for 32 clips on the CPU when tests/golden/eval.npz was written (a figure from the authoring
machine, the motivation rather than a same-box comparison).  No time is a pass / fail bar.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import numpy as np
    import torch
    import mst_amd  # noqa: F401
    import eval_fixture as ef
    from mst_amd.data_loaders import evaluator_wrapper as ew
    from mst_amd.utils import metrics as mt

    dev = torch.device("cuda:0")
    gold = np.load(os.path.join(ROOT, "tests", "golden", "eval.npz"))
    F, T, B = 263, 196, args.batch
    mv, mo, tx = ef.nets(F)
    t = lambda sd: {k: torch.from_numpy(v) for k, v in sd.items()}
    ev = ew.MotionEvaluator(t(mv), t(mo), t(tx), dim_pose=F, device=dev)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        out = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b))
        return round(statistics.median(out), 4)

    sample = torch.randn(args.clips, F, 1, T, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    lengths = [T - 4 * (b % 8) for b in range(args.clips)]
    scale = torch.from_numpy((0.5 + ef.syn.uniform01(ef.SEED, "eval/bench/scale", F)).astype(np.float32)).to(dev)
    shift = torch.from_numpy(ef.syn.normal(ef.SEED, "eval/bench/shift", (F,))).to(dev)

    def embed_all():
        return torch.cat([ev.embed_samples(sample[i:i + B], lengths[i:i + B], scale, shift) for i in range(0, args.clips, B)])

    res = {"clips": args.clips, "batch": B, "reps": args.reps}
    res["embed_ms"] = timed(embed_all)
    res["embed_ms_per_batch"] = round(res["embed_ms"] / (args.clips / B), 4)
    emb = embed_all()
    other = torch.cat([ev.embed_samples(sample[i:i + B], lengths[i:i + B]) for i in range(0, args.clips, B)])      # the same clips, not renormalised
    first = np.random.RandomState(1).choice(args.clips, 300, replace=False)

    def stats():
        mt.calculate_activation_statistics(emb)
        mt.calculate_activation_statistics(other)
        for i in range(0, args.clips - 31, 32):
            mt.calculate_R_precision(emb[i:i + 32], other[i:i + 32], 3)
        mt.calculate_matching_score(emb, other)
        np.random.seed(1)
        mt.calculate_diversity(emb, 300)

    res["stats_device_ms"] = timed(stats)
    (mu_a, cov_a), (mu_b, cov_b) = mt.calculate_activation_statistics(emb), mt.calculate_activation_statistics(other)
    t0 = time.perf_counter()
    res["fid"] = float(mt.calculate_frechet_distance(mu_a, cov_a, mu_b, cov_b))
    res["frechet_host_s"] = round(time.perf_counter() - t0, 3)

    # ---- the kernel families, one batch
    x = sample[:B].contiguous()
    steps = np.asarray(lengths[:B]) // 4
    T1, T2 = ew.conv_frames(T), ew.movement_frames(T)
    m, g = ev.movement, ev.motion
    fam = {}
    conv1 = lambda: ev._gemm(x, m["conv1_w"], m["conv1_b"], B * T1, leaky=True, mode=2, batch=B, frames=T, channels=F - 4, ldx=F, sb=F * T,
                             scale=scale, shift=shift)
    y1 = conv1()
    conv2 = lambda: ev._gemm(y1, m["conv2_w"], m["conv2_b"], B * T2, leaky=True, mode=1, batch=B, frames=T1, channels=512, ldx=512, sb=T1 * 512)
    y2 = conv2()
    lin = lambda: ev._gemm(ev._gemm(y2, m["out_w"], m["out_b"], B * T2), g["in_w"], g["in_b"], B * T2)
    e = lin()
    proj = lambda: ev._gemm(e, g["w_ih"], g["b_ih"], B * T2)
    xp = proj()
    H = g["w_hh"].shape[2]
    steps_dev = torch.as_tensor(steps.astype(np.int32)).to(dev)
    work, last = torch.empty(2, B, 2 * H, device=dev), torch.empty(B, 2 * H, device=dev)
    N = ew.N

    def gru():
        N.check(N.lib().mst_eval_gru(N.ptr(xp), N.ptr(g["w_hh"]), N.ptr(g["b_hh"]), N.ptr(g["hidden"]), N.ptr(steps_dev), B, T2, H,
                                     int(steps.max()), N.ptr(work), N.ptr(last), N.stream_ptr(dev)))

    def out_net():
        y = ev._gemm(last, g["o0_w"], g["o0_b"], B)
        z = torch.empty_like(y)
        N.check(N.lib().mst_eval_layernorm(N.ptr(y), N.ptr(g["ln_w"]), N.ptr(g["ln_b"]), N.ptr(z), B, H, ew.LN_EPS, 1, N.stream_ptr(dev)))
        return ev._gemm(z, g["o3_w"], g["o3_b"], B)

    with torch.cuda.device(dev):
        for name, fn in (("conv1_gemm", conv1), ("conv2_gemm", conv2), ("out_net_input_emb_gemms", lin), ("gru_input_projection_gemm", proj),
                         (f"gru_{int(steps.max())}_steps", gru), ("output_net", out_net)):
            fam[name + "_ms"] = timed(fn)
    fam["dist_rank_32x32_ms"] = timed(lambda: mt.calculate_R_precision(emb[:32], emb[32:64], 3))
    fam[f"dist_rank_{args.clips}x{args.clips}_ms"] = timed(lambda: mt.calculate_R_precision(emb, emb.flip(0), 3))
    fam[f"cov_f64_{args.clips}x512_ms"] = timed(lambda: mt.calculate_activation_statistics(emb))
    fam["pair_norms_1024_ms"] = timed(lambda: mt._pair_norms(emb, emb, first.repeat(4)[:1024], first[::-1].repeat(4)[:1024], "bench"))
    res["families"] = fam
    res["reference_cpu_s_per_32_clips"] = round(float(gold["seconds|embed32"]), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
