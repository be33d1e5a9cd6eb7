"""Rendering clips to frames: what `render_motion` costs at the sampler's batch, 64 clips x 196 frames x 22 joints at 300 x 300.

  one call             `render_motion` on the whole batch, without a trace and with a root trace
  frames= chunks       the traced batch through `frames=(t0, t0 + 32)`, a call a chunk: what `render_to_file` does a clip at a time
  long clips           8 clips x 4096 frames, without and with a root trace (a trace at frame t has t points: this is where the trace's
                       cost shows), rendered through `frames=` chunks of 512 so the video of a long clip is never resident whole
  matplotlib           a modernised loop of the reference's `explicit_plot_3d_motion` (Agg, `canvas.draw()` per frame, no encoding) on
                       the CPU for ONE clip of 196 frames, when matplotlib is importable: the stand-in for the reference, whose own
                       function does not run on a current matplotlib

The GPU entries are interleaved: each is called once untimed, then `--reps` (5) rounds of all of them in turn, each event-timed around
a synchronised call; medians, in ms.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def matplotlib_loop(joints, chains, scale=1.3, radius=3):
    """One clip [T, J, 3] -> seconds for the reference's scene drawn frame by frame on an Agg canvas, root_horizontal trace included."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import numpy as np
    from mpl_toolkits.mplot3d import Axes3D
    from mpl_toolkits.mplot3d.art3d import Poly3DCollection
    data = joints.astype(np.float64) * scale
    fig = plt.figure(figsize=(3, 3), dpi=100)
    ax = Axes3D(fig)
    fig.add_axes(ax)
    mins, maxs = data.min((0, 1)), data.max((0, 1))
    data[:, :, 1] -= mins[1]
    traj = data[:, 0].copy()
    data[..., 0] -= data[:, 0:1, 0]
    data[..., 2] -= data[:, 0:1, 2]
    colors = ["#DD5A37", "#D69E00", "#B75A39", "#FF6D00", "#DDB50E"]

    def update(t):
        ax.clear()
        ax.set_xlim3d([-radius / 2, radius / 2])
        ax.set_ylim3d([0, radius])
        ax.set_zlim3d([-radius / 3.0, radius * 2 / 3.0])
        ax.view_init(elev=120, azim=-90)
        ax.grid(False)
        x0, x1, z0, z1 = mins[0] - traj[t, 0], maxs[0] - traj[t, 0], mins[2] - traj[t, 2], maxs[2] - traj[t, 2]
        plane = Poly3DCollection([[[x0, 0, z0], [x0, 0, z1], [x1, 0, z1], [x1, 0, z0]]])
        plane.set_facecolor((0.5, 0.5, 0.5, 0.5))
        ax.add_collection3d(plane)
        for chain, color in zip(chains, colors):
            ax.plot3D(data[t, chain, 0], data[t, chain, 1], data[t, chain, 2], linewidth=4.0, color=color)
        ax.plot3D(traj[:t, 0] - traj[t, 0], np.zeros(t), traj[:t, 2] - traj[t, 2], linewidth=2.0, color=colors[0])
        ax.set_axis_off()
        fig.canvas.draw()

    for t in range(3):
        update(t)
    start = time.perf_counter()
    for t in range(len(data)):
        update(t)
    took = time.perf_counter() - start
    plt.close(fig)
    return took


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=196)
    ap.add_argument("--long-clips", type=int, default=8)
    ap.add_argument("--long-frames", type=int, default=4096)
    ap.add_argument("--size", type=int, default=300)
    ap.add_argument("--no-matplotlib", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import mst_amd  # noqa: F401
    import render_fixture as rf
    from mst_amd.utils import plot_script as ps

    dev = torch.device("cuda:0")
    J, chains = 22, rf.chains_of(22)
    short = torch.from_numpy(rf.walk(31, args.clips, args.frames, J)).to(dev)
    long = torch.from_numpy(rf.walk(32, args.long_clips, args.long_frames, J)).to(dev)
    trace = ["root_horizontal"]

    def chunked(joints, step, features):
        T = joints.shape[1]
        for s in range(0, T, step):
            ps.render_motion(joints, chains, painting_features=features, size=args.size, frames=(s, min(s + step, T)))

    def timed(entries):
        for fn in entries.values():
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in entries}
        for _ in range(args.reps):
            for k, fn in entries.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                ms[k].append(a.elapsed_time(b))
        return {k: round(statistics.median(v), 3) for k, v in ms.items()}

    out = {"clips": args.clips, "frames": args.frames, "joints": J, "size": args.size, "reps": args.reps, "tile": 32,
           "chunk": ps.limits()["chunk"]}
    out.update(timed({
        "one_call_ms": lambda: ps.render_motion(short, chains, size=args.size),
        "one_call_traced_ms": lambda: ps.render_motion(short, chains, painting_features=trace, size=args.size),
        "chunks_of_32_traced_ms": lambda: chunked(short, 32, trace),
    }))
    out["long_clips"], out["long_frames"] = args.long_clips, args.long_frames
    out.update(timed({
        "long_ms": lambda: chunked(long, 512, ()),
        "long_traced_ms": lambda: chunked(long, 512, trace),
    }))
    frames = args.clips * args.frames
    out["frames_per_s_traced"] = round(frames / (out["one_call_traced_ms"] * 1e-3))
    out["long_traced_over_untraced"] = round(out["long_traced_ms"] / out["long_ms"], 2)
    if not args.no_matplotlib:
        try:
            import matplotlib
        except ImportError:
            matplotlib = None
        if matplotlib is not None:
            s = matplotlib_loop(short[0].cpu().numpy(), chains)
            out["matplotlib_version"] = matplotlib.__version__
            out["matplotlib_one_clip_s"] = round(s, 3)
            out["matplotlib_frames_per_s"] = round(args.frames / s, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
