"""Golden vectors of the render path.  Run in the authoring container only (the reference checkout on the path, matplotlib installed):
    python tests/golden/make_golden_render.py -> render.npz

Stored:
  `cam|proj`                        `Axes3D.get_proj()` of the installed matplotlib for the reference's axes: an `Axes3D` added to a
                                    (3, 3) figure, the limits `explicit_plot_3d_motion` sets (radius 3) and `view_init(120, -90)`
  `cam|points`                      a dozen seeded points inside the axis box
  `cam|pixels|300`, `cam|pixels|150`  where `proj_transform` and `transData` put them in the 300 x 300 and the 150 x 150 figure
  `cam|matplotlib`                  the version that drew them
  `colors|<case>`                   the `frame_colors` list the reference's own `plot_3d_motion` hands to `explicit_plot_3d_motion`
                                    (data_loaders/humanml/utils/plot_script.py:30-56), as palette indices (0 blue, 1 orange, 2 purple),
                                    for every case of COLOR_CASES: the reference's module is imported unmodified and its
                                    `explicit_plot_3d_motion` replaced by a recorder, so nothing is drawn
Asserted before anything is written: the origin lands at (154.054, 85.452) px in the 300 x 300 figure; this package's `default_camera`
agrees with the recorded matrix to 1e-12 and with the pixels to 1e-9 of the image side; `frame_colors` returns every recorded list."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
from mst_amd.utils import plot_script as ps  # noqa: E402

NAMES = ("blue", "orange", "purple", "upper_body")
# case -> (frames, keyword arguments of plot_3d_motion)
COLOR_CASES = {
    "default": (12, dict(gt_frames=[0, 3, 4, 11])),
    "default_none": (5, dict()),
    "upper_body": (9, dict(vis_mode="upper_body", gt_frames=[1, 2])),
    "gt": (7, dict(vis_mode="gt", gt_frames=[2])),
    "unfold": (40, dict(vis_mode="unfold", handshake_size=10, blend_size=5)),
    "unfold_arb_len": (60, dict(vis_mode="unfold_arb_len", handshake_size=8, blend_size=3, step_sizes=[30, 52, 70], lengths=[30, 40, 36])),
    "unfold_arb_len_two": (20, dict(vis_mode="unfold_arb_len", handshake_size=4, blend_size=2, step_sizes=[20, 30], lengths=[20, 16])),
}
RADIUS = 3


def camera():
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from mpl_toolkits.mplot3d import Axes3D, proj3d
    g = np.random.default_rng(mg.SEED)
    lo, hi = np.array([-RADIUS / 2, 0.0, -RADIUS / 3.0]), np.array([RADIUS / 2, RADIUS, RADIUS * 2 / 3.0])
    points = g.uniform(lo, hi, (12, 3))
    out = {"cam|points": points, "cam|matplotlib": np.array(matplotlib.__version__)}
    for dpi in (100, 50):
        fig = plt.figure(figsize=(3, 3), dpi=dpi)
        ax = Axes3D(fig)
        fig.add_axes(ax)
        ax.set_xlim3d([-RADIUS / 2, RADIUS / 2])
        ax.set_ylim3d([0, RADIUS])
        ax.set_zlim3d([-RADIUS / 3.0, RADIUS * 2 / 3.0])
        ax.view_init(elev=120, azim=-90)
        fig.canvas.draw()
        M = ax.get_proj()
        x, y, _ = proj3d.proj_transform(points[:, 0], points[:, 1], points[:, 2], M)
        out[f"cam|pixels|{3 * dpi}"] = ax.transData.transform(np.stack([x, y], 1))
        if dpi == 100:
            out["cam|proj"] = M
            x0, y0, _ = proj3d.proj_transform(0.0, 0.0, 0.0, M)
            origin = ax.transData.transform((x0, y0))
            print("origin at", origin)
            assert np.allclose(origin, (154.054, 85.452), atol=1e-3)
        else:
            assert np.array_equal(M, out["cam|proj"])
        plt.close(fig)
    return out


def colors():
    mg.install_shims()
    from data_loaders.humanml.utils import plot_script as ref
    seen = {}

    def recorder(save_path, kinematic_tree, joints, title, dataset, **kw):
        seen["colors"] = list(kw["frame_colors"])

    ref.explicit_plot_3d_motion = recorder
    out = {}
    for case, (T, kw) in COLOR_CASES.items():
        ref.plot_3d_motion("unused.mp4", [[0, 1]], np.zeros((T, 2, 3), np.float32), "title", "humanml", **kw)
        out[f"colors|{case}"] = np.array([NAMES.index(c) for c in seen["colors"]], np.int8)
        print(case, len(seen["colors"]), "names")
    return out


def main():
    out = camera()
    out.update(colors())
    P, _ = ps.default_camera(300, 300, RADIUS)
    assert np.abs(P - out["cam|proj"]).max() < 1e-12
    for side in (300, 150):
        P, A = ps.default_camera(side, side, RADIUS)
        v = np.c_[out["cam|points"], np.ones(12)] @ P.T
        pix = (A @ np.stack([v[:, 0] / v[:, 3], v[:, 1] / v[:, 3], np.ones(12)])).T
        d = np.abs(pix - out[f"cam|pixels|{side}"]).max() / side
        print(f"closed form vs matplotlib at {side}: {d:.3e} of the side")
        assert d < 1e-9
    for case, (T, kw) in COLOR_CASES.items():
        kw = dict(kw)
        got = ps.frame_colors(T, kw.pop("vis_mode", "default"), **kw)
        assert [NAMES.index(c) for c in got] == out[f"colors|{case}"].tolist(), case
    path = os.path.join(HERE, "render.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
