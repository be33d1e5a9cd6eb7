"""Rotation-channel decode: what reading a sample's own rotations costs on the GPU, next to the 100-iteration fit it can replace for a
preview.  Seeded trees and rows of tests/rotdec_fixture.py, every output asked for:

  hml_rot   64 x 196 frames x 22 joints (the 263-feature row), and 8 x 4096 frames
  pos_ik    the same two shapes: the positions of the 263-feature row through the chain IK
  real_rot  64 x 196 frames x 21 joints (the 190-feature row), and 8 x 4096 frames
  fit       fit_joints on 64 x 196 frames x 21 joints, 100 iterations, in the same run: the route to a file that needs no decode

Each is event-timed: one launch between two device events, the median of `--reps` (20) after `--warmup` untimed calls.  Next to them the
seconds per 196-frame clip the reference's functions took when tests/golden/rotdec.npz was written (a CPU figure from the authoring
machine, the motivation rather than a same-box comparison).  No time is a pass / fail bar.  Prints one JSON line."""
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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    import mst_amd  # noqa: F401
    import ik_fixture as ik
    import rotdec_fixture as rf
    from mst_amd.utils import joint_fit as jf
    from mst_amd.utils import rot_decode as rd

    dev = torch.device("cuda:0")
    gold = np.load(os.path.join(ROOT, "tests", "golden", "rotdec.npz"))

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

    def case(route, name, B, T):
        J, chains, off = rf.tree(name)
        rows = rf.make_rows(name, route, T, B=min(B, 4))                                   # four distinct clips, repeated
        x = torch.from_numpy(np.concatenate([rows] * (B // len(rows) + 1))[:B]).to(dev)
        ik = dict(raw_offsets=rf.raw_of(off), face_joint_indx=rf.face_of(J)) if route == rf.POS else {}
        return lambda: rd.decode_rotations(x, J, chains, off, route=route, joints=True, local=route == rf.REAL, **ik)

    res = {"reps": args.reps}
    for route, name in ((rf.HML, "t2m22"), (rf.POS, "t2m22"), (rf.REAL, "mid21")):
        res[f"{route}_{args.batch}x196_ms"] = timed(case(route, name, args.batch, 196))
        res[f"{route}_8x4096_ms"] = timed(case(route, name, 8, 4096))
    J = 21
    _, parents, off = ik.humanoid(1, J, scale=6.0)
    data, target = ik.make_clip(1, f"bench/J{J}", 196, J, parents, off, B=8)
    data, target = np.concatenate([data] * 8)[:args.batch], np.concatenate([target] * 8)[:args.batch]
    d, g = torch.from_numpy(data).to(dev), torch.from_numpy(target).to(dev)
    res[f"fit_joints_{args.batch}x196_100_iters_ms"] = timed(lambda: jf.fit_joints(d, J, parents, off, g, 100))
    res["reference_cpu_s_per_196_frame_clip"] = {k.split("|")[1]: round(float(gold[k]), 4) for k in gold.files if k.startswith("seconds|")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
