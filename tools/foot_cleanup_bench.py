"""Foot-skate cleanup: what the demo's output stage costs on the GPU (sample/demo_style_transfer.py:310-313).  Batch 64 at the HumanML
shape, the demo's settings (vel3 at 0.05, force_on_floor, after_butterworth, interp_length 5), seeded clips with planted stance phases
(tests/foot_fixture.py):

  (a) two_passes   -- two remove_fs calls on 64 x (196, 22, 3) joints already on the GPU, pass 1 against a content motion
  (b) clean_joints -- recover_joints + the two passes from a 64 x (263, 1, 196) sample

Each is enqueued `--iters` times between two device events after `--warmup` untimed rounds; the figure is the mean per round, the median
over `--reps` such measurements.  Next to them: the seconds per clip the reference took for the same two passes on ONE clip when
tests/golden/fs.npz was written (a CPU figure from the authoring machine, the motivation rather than a same-box comparison).
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    import mst_amd  # noqa: F401
    import foot_fixture as ff
    from mst_amd.utils import foot_cleanup as fc

    dev = torch.device("cuda:0")
    B, T, J, F = args.batch, 196, 22, 263
    fs = np.load(os.path.join(ROOT, "tests", "golden", "fs.npz"))
    clips = [ff.make_clip(1, f"bench/{b % 8}", T, J, ff.FID22) for b in range(B)]          # eight distinct clips, repeated
    content = torch.from_numpy(np.stack([ff.make_clip(1, f"bench/content{b % 8}", T, J, ff.FID22) for b in range(B)])).to(dev)
    joints = torch.from_numpy(np.stack(clips)).to(dev)
    packed = [ff.sample_from_joints(c, 1, "bench/sample") for c in clips[:8]]
    sample = torch.from_numpy(np.stack([packed[b % 8][0] for b in range(B)])).to(dev)
    mean, std = packed[0][1], packed[0][2]
    names, kw = list(ff.NAMES22), dict(force_on_floor=True, after_butterworth=True, use_vel3=True, vel3_thr=0.05)

    def two_passes():
        a = fc.remove_fs("", joints, content, names, ff.EE_NAMES, **kw)[0]
        return fc.remove_fs("", a, a, names, ff.EE_NAMES, **kw)[0]

    def clean():
        return fc.clean_joints(sample, mean, std, J, ff.FID22, ref_joints=content)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        out = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(args.iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b) * 1e3 / args.iters)
        return out

    tp, cj = timed(two_passes), timed(clean)
    ref_s = float(fs["ref_seconds_per_clip"])
    m_tp, m_cj = statistics.median(tp), statistics.median(cj)
    print(json.dumps({"shape": [B, T, J, 3], "two_passes_us": round(m_tp, 1), "two_passes_all_us": [round(v, 1) for v in tp],
                      "clean_joints_us": round(m_cj, 1), "clean_joints_all_us": [round(v, 1) for v in cj],
                      "two_passes_us_per_clip": round(m_tp / B, 2), "clips_per_s_two_passes": round(B / m_tp * 1e6, 0),
                      "reference_cpu_s_per_clip": round(ref_s, 4), "reference_over_gpu_per_clip": round(ref_s * 1e6 / (m_tp / B), 0),
                      "max_frames_22": fc.max_frames(J), "iters": args.iters, "reps": args.reps}))


if __name__ == "__main__":
    main()
