"""Motion encoder: what turning joints back into feature rows costs on the GPU.  Seeded skeletons and clips of tests/encode_fixture.py:

  (a) hml     -- encode_joints on 64 x 196 frames x 22 joints, mode "hml" (263 features: chain IK, local velocities, contacts), mean / std
  (b) posrot  -- encode_joints on 64 x 196 frames x 21 joints, mode "posrot" (190 features, rotations given), mean / std

Each is enqueued `--iters` times between two device events after `--warmup` untimed rounds; the figure is the mean per round (one launch
and its output allocations), the median over `--reps` such measurements.  Next to them: the seconds per clip the reference's process_file /
process_file_with_rotation took at T = 197 when tests/golden/encode.npz was written (a CPU figure from the authoring machine, the motivation
rather than a same-box comparison).  Prints one JSON line."""
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
    import encode_fixture as ef
    from mst_amd.utils import motion_process as mp

    dev = torch.device("cuda:0")
    gold = np.load(os.path.join(ROOT, "tests", "golden", "encode.npz"))

    def case(B, T, J, mode):
        sk = ef.skeleton(1, J, 6.0 if J == 21 else 1.0)
        pos, rot = ef.make_clip(1, f"bench/{mode}", T, sk, mode, B=min(B, 8), scale=6.0 if J == 21 else 1.0, pace=0.4, gated=True)
        pos, rot = (np.concatenate([a] * (B // len(a) + 1))[:B] for a in (pos, rot))             # eight distinct clips, repeated
        F = ef.feats(J, mode)
        p, r = torch.from_numpy(pos).to(dev), torch.from_numpy(rot).to(dev) if mode == ef.POSROT else None
        m, s = torch.zeros(F, device=dev), torch.ones(F, device=dev)
        kw = sk.kw()
        return lambda: mp.encode_joints(p, r, mode=mode, mean=m, std=s, **kw)

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

    hml, posrot = timed(case(args.batch, 196, 22, ef.HML)), timed(case(args.batch, 196, 21, ef.POSROT))
    m_h, m_p = statistics.median(hml), statistics.median(posrot)
    ref = {k.rsplit("|", 1)[0]: round(float(gold[k]), 4) for k in gold.files if k.endswith("|seconds")}
    print(json.dumps({"hml_shape": [args.batch, 196, 22], "hml_ms": round(m_h, 4), "hml_all_ms": [round(v, 4) for v in hml],
                      "hml_us_per_clip": round(1e3 * m_h / args.batch, 3), "posrot_shape": [args.batch, 196, 21], "posrot_ms": round(m_p, 4),
                      "posrot_all_ms": [round(v, 4) for v in posrot], "posrot_us_per_clip": round(1e3 * m_p / args.batch, 3),
                      "reference_cpu_s_per_clip": ref, "max_frames": mp.encode_max_frames(22, ef.HML), "iters": args.iters,
                      "reps": args.reps}))


if __name__ == "__main__":
    main()
