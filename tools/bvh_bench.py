"""Motion files: what the GPU stages and the host's text passes cost.  Two batches of 24-joint clips (32 file joints with their End
Sites, root with 6 channels, the rest 3): 64 clips x 196 frames and 8 clips x 4096 frames.

  device   `decode_channels` (k_bvh_decode: all file joints, and a 22-joint selection), `quats_to_channels` (k_quats_to_channels) and
           `retarget_joints` (k_retarget, 22 joints): one untimed call, then `--reps` calls each, event-timed around a synchronised
           call; medians, in ms per batch
  host     `parse_bvh` and `format_bvh` of one clip of each length, best of three, in ms per clip
  recorded the reference's seconds per clip from tests/golden/bvh.npz (`read_bvh` and `save_bvh` of a 4096-frame 24-joint clip,
           `uniform_skeleton_basic` of a 60-frame 22-joint one), measured on the CPU of the machine that made the goldens

Prints one JSON line."""
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
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    import mst_amd  # noqa: F401
    import bvh_fixture as bf
    from mst_amd.utils import bvh
    from mst_amd.utils import motion_process as mp

    dev = torch.device("cuda:0")
    gold = np.load(os.path.join(ROOT, "tests", "golden", "bvh.npz"))

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return round(statistics.median(ms), 4)

    def best(fn):
        t = 1e9
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            t = min(t, time.perf_counter() - t0)
        return round(t * 1e3, 3)

    sk = bf.file_skeleton(bf.SEED, "bench", 32, "root6", "zyx")
    sel = sk.not_end_index[:22]
    rsk, rpos, tgt, l_idx = bf.retarget_case(bf.SEED, 22, 196)
    out = {"file_joints": sk.joints, "joints": len(sk.not_end_index), "reps": args.reps}
    for B, T in ((64, 196), (8, 4096)):
        host = bf.channels(bf.SEED, "bench", sk, T)
        ch = torch.from_numpy(np.repeat(host, B, 0)).to(dev)
        m = bvh.decode_channels(ch, sk)
        keep = sk.not_end_index
        quats, root = m.rotations[:, :, keep].contiguous(), m.positions[:, :, 0].contiguous()
        pos = torch.from_numpy(np.tile(rpos, (B, (T + 195) // 196, 1, 1))[:, :T].copy()).to(dev)
        text = bvh.format_bvh(sk, host[0])
        key = f"{B}x{T}"
        out[key] = {
            "decode_ms": timed(lambda: bvh.decode_channels(ch, sk)),
            "decode_select22_ms": timed(lambda: bvh.decode_channels(ch, sk, joints=sel)),
            "quats_to_channels_ms": timed(lambda: bvh.quats_to_channels(quats, root, sk.simple_parents)),
            "retarget_ms": timed(lambda: mp.retarget_joints(pos, tgt, rsk.raw, rsk.chains, l_idx, rsk.face)),
            "host_parse_ms_per_clip": best(lambda: bvh.parse_bvh(text)),
            "host_format_ms_per_clip": best(lambda: bvh.format_bvh(sk, host[0])),
        }
    out["reference_cpu_s_per_clip"] = {"read_bvh_4096x24": round(float(gold["seconds|read_bvh|T4096J24"]), 4),
                                       "save_bvh_4096x24": round(float(gold["seconds|save_bvh|T4096J24"]), 4),
                                       "uniform_skeleton_basic_60x22": round(float(gold["retarget|J22T60|seconds"]), 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
