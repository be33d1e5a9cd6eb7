"""Joint-rotation fit: what the demo's last numeric stage, fit_joints_bvh's 100 Adam iterations (sample/demo_style_transfer.py:217, :306,
:318), costs on the GPU.  Seeded skeletons and clips of tests/ik_fixture.py:

  (a) batch   -- fit_joints on 64 x 196 frames x 21 joints (12 544 frames: 196 workgroups of 64 lanes), the samplers' layout with mean / std
  (b) single  -- fit_joints on 1 x 76 frames x 20 joints (two workgroups), the shape of one Xia clip

Each is enqueued `--iters` times between two device events after `--warmup` untimed rounds; the figure is the mean per round, the median
over `--reps` such measurements.  Next to them: the seconds per clip the reference took for 100 iterations when tests/golden/ik.npz was
written (a CPU figure from the authoring machine, the motivation rather than a same-box comparison).  Prints one JSON line."""
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
    ap.add_argument("--fit-iters", type=int, default=100)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    import mst_amd  # noqa: F401
    import ik_fixture as ik
    from mst_amd.utils import joint_fit as jf

    dev = torch.device("cuda:0")
    gold = np.load(os.path.join(ROOT, "tests", "golden", "ik.npz"))

    def case(B, T, J, sampler):
        _, parents, off = ik.humanoid(1, J, scale=6.0 if J == 21 else 1.0)
        data, target = ik.make_clip(1, f"bench/J{J}", T, J, parents, off, B=min(B, 8))          # eight distinct clips, repeated
        data, target = np.concatenate([data] * (B // len(data) + 1))[:B], np.concatenate([target] * (B // len(target) + 1))[:B]
        g = torch.from_numpy(target).to(dev)
        if not sampler:
            d = torch.from_numpy(data).to(dev)
            return lambda: jf.fit_joints(d, J, parents, off, g, args.fit_iters)
        F = 9 * J + 1
        mean, std = np.zeros(F, np.float32), np.ones(F, np.float32)
        d = torch.from_numpy(np.ascontiguousarray(data.transpose(0, 2, 1)[:, :, None, :])).to(dev)
        m, s = torch.from_numpy(mean).to(dev), torch.from_numpy(std).to(dev)
        return lambda: jf.fit_joints(d, J, parents, off, g, args.fit_iters, mean=m, std=s)

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
            out.append(a.elapsed_time(b) / args.iters)
        return out

    batch, single = timed(case(args.batch, 196, 21, True)), timed(case(1, 76, 20, False))
    m_b, m_s = statistics.median(batch), statistics.median(single)
    ref = {k.split("|")[0]: round(float(gold[k]), 3) for k in gold.files if k.endswith("|seconds") and "I100" in k}
    print(json.dumps({"fit_iters": args.fit_iters, "batch_shape": [args.batch, 196, 21], "batch_ms": round(m_b, 3),
                      "batch_all_ms": [round(v, 3) for v in batch], "batch_ms_per_clip": round(m_b / args.batch, 4),
                      "single_shape": [1, 76, 20], "single_ms": round(m_s, 3), "single_all_ms": [round(v, 3) for v in single],
                      "reference_cpu_s_per_clip_100_iters": ref, "max_joints": jf.max_joints(), "max_frames_21": jf.max_frames(21),
                      "iters": args.iters, "reps": args.reps}))


if __name__ == "__main__":
    main()
