"""The render path without a GPU: the C ABI's declarations and refusals, the default camera's closed form against the installed
matplotlib and against its recording (tests/golden/render.npz), `frame_colors` against the lists the reference's own `plot_3d_motion`
formed, the invariants of tests/render_fixture.py's restatement, `save_frames` and `title_overlay`."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
import render_fixture as rf
from conftest import GOLDEN, ROOT
from mst_amd import _native
from mst_amd.utils import plot_script as ps

NEW = ("mst_render_bounds", "mst_render_frames", "mst_render_max_frames", "mst_render_max_joints", "mst_render_chains_drawn",
       "mst_render_max_traces", "mst_render_max_side", "mst_render_chunk")


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "render.npz")) as z:
        return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------ the C ABI
def test_symbols_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "mst_engine.h")) as fh:
        header = fh.read()
    lib = _native.lib()
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _native.SIGNATURES and getattr(lib, name).argtypes == _native.SIGNATURES[name][1]
    assert "plot_script.py:168-311" in header
    assert (lib.mst_render_max_frames(), lib.mst_render_max_joints(), lib.mst_render_chains_drawn(), lib.mst_render_max_traces(),
            lib.mst_render_max_side()) == (4096, 64, 5, 8, 1024)
    assert lib.mst_render_chunk() >= 64
    assert ps.limits()["frames"] == 4096


def _ints(values):
    return (C.c_int32 * len(values))(*values)


def test_abi_refusals_need_no_gpu():
    lib = _native.lib()
    ok, bnd, out, outf = 64, 4096, 8192, 16384              # never dereferenced: every call below is refused first
    P, A = ps.default_camera(32, 32)

    def call(entry="frames", scene_null=False, view_null=False, bounds=bnd, o=out, of=None, **kw):
        s = dict(joints=ok, joints2=None, strides=(66, 66, 3, 1), lengths=None, batch=2, frames=9, J=22, scale=1.3)
        v = dict(chains=[[0, 1, 2], [0, 3]], kinds=[0, 2], tjoints=[0, 5], palette=None, W=32, H=32, dpi=100.0, overlay=None, ob=0, t0=0, t1=9,
                 n_chains=None, n_traces=None)
        for k, val in kw.items():
            (s if k in s else v)[k] = val
        scene = _native.MstRenderScene(s["joints"], s["joints2"], *s["strides"], s["lengths"], s["batch"], s["frames"], s["J"], s["scale"])
        view = _native.MstRenderView()
        offs = np.concatenate([[0], np.cumsum([len(c) for c in v["chains"]])]).astype(int).tolist()
        keep = (_ints(offs), _ints([j for c in v["chains"] for j in c] or [0]), _ints(v["kinds"] or [0]), _ints(v["tjoints"] or [0]))
        view.n_chains = len(v["chains"]) if v["n_chains"] is None else v["n_chains"]
        view.n_traces = len(v["kinds"]) if v["n_traces"] is None else v["n_traces"]
        view.chain_offsets_host, view.chain_joints_host, view.trace_kinds_host, view.trace_joints_host = keep
        view.palette_dev = v["palette"]
        view.proj = (C.c_float * 16)(*P.reshape(-1))
        view.affine = (C.c_float * 6)(*A.reshape(-1))
        view.width, view.height, view.dpi, view.overlay_dev, view.overlay_batch, view.t0, view.t1 = \
            v["W"], v["H"], v["dpi"], v["overlay"], v["ob"], v["t0"], v["t1"]
        sp = None if scene_null else C.byref(scene)
        if entry == "bounds":
            return lib.mst_render_bounds(sp, bounds, None)
        return lib.mst_render_frames(sp, bounds, None if view_null else C.byref(view), o, of, None)

    cases = [
        (dict(batch=0), b"batch"), (dict(batch=65536), b"batch"), (dict(frames=0), b"frames"), (dict(frames=4097), b"frames"),
        (dict(J=0), b"joints"), (dict(J=65), b"joints"), (dict(chains=[[0, 22]]), b"chain 0 names joint 22"),
        (dict(chains=[[0, 1]] * 5 + [[-1, 0]]), b"chain 5 names joint -1"), (dict(chains=[[0, 1]] * 17), b"chains"),
        (dict(chains=[[0] * 129]), b"points"), (dict(chains=[[0] * 100, [1] * 100]), b"points"),
        (dict(kinds=[2], tjoints=[22]), b"trace 0 names joint 22"), (dict(kinds=[2], tjoints=[-1]), b"trace 0 names joint -1"),
        (dict(kinds=[3], tjoints=[0]), b"kind"), (dict(kinds=[0] * 9, tjoints=[0] * 9), b"traces"),
        (dict(W=15), b"image"), (dict(H=1025), b"image"), (dict(W=1025), b"image"), (dict(H=15), b"image"),
        (dict(joints=None), b"null joints"), (dict(bounds=None), b"null bounds or output"), (dict(o=None), b"null bounds or output"),
        (dict(scene_null=True), b"null scene"), (dict(view_null=True), b"null view"),
        (dict(overlay=ok + 1, ob=3), b"overlay"), (dict(overlay=ok + 1, ob=0), b"overlay"),
        (dict(t0=-1), b"frame range"), (dict(t0=4, t1=4), b"frame range"), (dict(t1=10), b"frame range"), (dict(t0=5, t1=3), b"frame range"),
        (dict(o=ok), b"an output may not be an input"), (dict(of=ok), b"an output may not be an input"), (dict(o=bnd), b"an output may not be an input"),
        (dict(overlay=out, ob=1), b"an output may not be an input"), (dict(palette=outf, of=outf), b"an output may not be an input"),
        (dict(joints2=out), b"an output may not be an input"), (dict(lengths=out), b"an output may not be an input"),
        (dict(of=out), b"the two outputs"), (dict(strides=(66, 66, 0, 1)), b"strides"), (dict(scale=float("nan")), b"scale"),
        (dict(dpi=0.0), b"dpi"), (dict(dpi=float("inf")), b"dpi"),
        (dict(entry="bounds", batch=0), b"mst_render_bounds: batch"), (dict(entry="bounds", frames=4097), b"mst_render_bounds: frames"),
        (dict(entry="bounds", J=65), b"mst_render_bounds: joints"), (dict(entry="bounds", joints=None), b"mst_render_bounds: null joints"),
        (dict(entry="bounds", bounds=None), b"null bounds"), (dict(entry="bounds", bounds=ok), b"may not be an input"),
        (dict(entry="bounds", scene_null=True), b"null scene"),
    ]
    for kw, word in cases:
        assert call(**kw) != 0, kw
        assert word in lib.mst_last_error(), (kw, lib.mst_last_error())


def test_python_argument_checks_raise_on_the_host():
    j = torch.zeros(2, 9, 22, 3)
    chains = rf.chains_of(22)
    for kw, err in ((dict(joints=j.numpy()), TypeError), (dict(layout="guess"), ValueError), (dict(joints=j[0]), ValueError),
                    (dict(joints=j.permute(0, 2, 3, 1)), ValueError),            # [B, J, 3, T] without layout='bjct': never guessed
                    (dict(joints2=j[:1]), ValueError), (dict(size=15), ValueError), (dict(size=(300, 1025)), ValueError),
                    (dict(kinematic_tree=[[0, 22]]), ValueError), (dict(kinematic_tree=[[0, 1]] * 17), ValueError),
                    (dict(painting_features=["left_wrist"]), ValueError), (dict(painting_features=[22]), ValueError),
                    (dict(painting_features=["nobody"], names=["pelvis"]), ValueError), (dict(painting_features=list(range(9))), ValueError),
                    (dict(frames=(0, 10)), ValueError), (dict(frames=(3, 3)), ValueError), (dict(lengths=[9]), ValueError),
                    (dict(lengths=[9, 0]), ValueError), (dict(lengths=[9, 10]), ValueError), (dict(palette="green"), ValueError),
                    (dict(palette=np.zeros(8, np.int32)), ValueError), (dict(palette=np.full(9, 4)), ValueError),
                    (dict(camera=(np.eye(3), np.zeros((2, 3)))), ValueError), (dict(overlay=np.zeros((30, 30), np.uint8)), ValueError),
                    (dict(overlay=np.zeros((3, 300, 300), np.uint8)), ValueError), (dict(dpi=0), ValueError), (dict(scale=float("inf")), ValueError),
                    (dict(), RuntimeError)):                                     # a CPU tensor: there is no CPU path
        args = dict(joints=j, kinematic_tree=chains)
        args.update(kw)
        with pytest.raises(err):
            ps.render_motion(**args)
    with pytest.raises(ValueError, match="dataset"):
        ps.explicit_plot_3d_motion(None, chains, j, "t", "nowhere")
    assert ps._traces("t", ["root", "left_wrist", 3, "root_horizontal"], ["pelvis", "left_wrist"], 22) == ([0, 1, 2, 2], [0, 0, 1, 3])
    assert ps._traces("t", "", None, 22) == ([], [])                            # the demo's "".split(',') names nothing
    for pal in ("purple", ["blue", "orange", "orange"], np.array([0, 1, 1]), np.array([[0, 1, 1], [2, 2, 3]])):
        got = ps._palette("t", pal, 2, 3)                                        # [B][T] as the kernel reads it: rows, not a broadcast view
        assert got.flags.c_contiguous and got.dtype == np.int32 and got.shape == (2, 3)
    assert ps._palette("t", ["blue", "orange", "orange"], 2, 3).tolist() == [[0, 1, 1], [0, 1, 1]]


# ------------------------------------------------------------------------------------------ the camera
def _closed_form_pixels(points, side):
    P, A = ps.default_camera(side, side)
    v = np.c_[points, np.ones(len(points))] @ P.T
    return P, (A @ np.stack([v[:, 0] / v[:, 3], v[:, 1] / v[:, 3], np.ones(len(points))])).T


def test_default_camera_equals_the_recording(gold):
    P, pix = _closed_form_pixels(gold["cam|points"], 300)
    assert np.abs(P - gold["cam|proj"]).max() < 1e-12
    for side in (300, 150):
        d = np.abs(_closed_form_pixels(gold["cam|points"], side)[1] - gold[f"cam|pixels|{side}"]).max() / side
        print(f"closed form vs recording at {side}: {d:.3e} of the side")
        assert d <= 1e-9
    origin = _closed_form_pixels(np.zeros((1, 3)), 300)[1][0]
    assert np.allclose(origin, (154.054, 85.452), atol=1e-3)


def test_default_camera_equals_the_installed_matplotlib(gold):
    matplotlib = pytest.importorskip("matplotlib")
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from mpl_toolkits.mplot3d import Axes3D, proj3d
    g = np.random.default_rng(7)
    r = 3
    points = g.uniform([-r / 2, 0, -r / 3], [r / 2, r, 2 * r / 3], (12, 3))
    for dpi in (100, 50):
        fig = plt.figure(figsize=(3, 3), dpi=dpi)
        try:
            ax = Axes3D(fig)
            fig.add_axes(ax)
            ax.set_xlim3d([-r / 2, r / 2])
            ax.set_ylim3d([0, r])
            ax.set_zlim3d([-r / 3.0, r * 2 / 3.0])
            ax.view_init(elev=120, azim=-90)
            fig.canvas.draw()
            M = ax.get_proj()
            x, y, _ = proj3d.proj_transform(points[:, 0], points[:, 1], points[:, 2], M)
            want = ax.transData.transform(np.stack([x, y], 1))
        finally:
            plt.close(fig)
        P, pix = _closed_form_pixels(points, 3 * dpi)
        d = np.abs(pix - want).max() / (3 * dpi)
        print(f"closed form vs matplotlib {matplotlib.__version__} at {3 * dpi}: matrix {np.abs(P - M).max():.3e}, pixels {d:.3e} of the side")
        assert np.abs(P - M).max() < 1e-12 and d <= 1e-9


def test_camera_options_and_non_square_definition():
    P10, _ = ps.default_camera(300, 300)
    P75, _ = ps.default_camera(300, 300, dist=7.5)
    assert P10[2, 3] == -10.0 and P75[2, 3] == -7.5
    _, A = ps.default_camera(200, 120)                       # the square map of 120, centred: 40 pixels of margin left and right
    _, S = ps.default_camera(120, 120)
    assert np.allclose(A[:, :2], S[:, :2]) and np.isclose(A[0, 2], S[0, 2] + 40.0) and np.isclose(A[1, 2], S[1, 2])
    with pytest.raises(ValueError):
        ps.default_camera(300, 300, radius=0)


# ------------------------------------------------------------------------------------------ frame colours
def test_frame_colors_equal_the_references_lists(gold):
    import sys
    sys.path.insert(0, GOLDEN)
    try:
        from make_golden_render import COLOR_CASES
    finally:
        sys.path.remove(GOLDEN)
    assert {f"colors|{c}" for c in COLOR_CASES} == {k for k in gold if k.startswith("colors|")}
    modes = set()
    for case, (T, kw) in COLOR_CASES.items():
        kw = dict(kw)
        mode = kw.pop("vis_mode", "default")
        modes.add(mode)
        got = ps.frame_colors(T, mode, **kw)
        assert [ps.PALETTE_NAMES.index(c) for c in got] == gold[f"colors|{case}"].tolist(), case
    assert modes == {"default", "upper_body", "gt", "unfold", "unfold_arb_len"}
    # frames behind the list are blue; under 'upper_body' an orange frame reads the upper_body palette
    assert ps.palette_indices(["orange", "purple"], 4).tolist() == [1, 2, 0, 0]
    assert ps.palette_indices(["orange", "blue"], 3, upper_body=True).tolist() == [3, 0, 0]
    assert np.array_equal(rf.PALETTE[3], np.concatenate([rf.PALETTE[0][:2], rf.PALETTE[1][2:]]))


# ------------------------------------------------------------------------------------------ the restatement's own invariants
def _flat_camera(side):
    """x right, y up, one unit a pixel, w = 1: the image plane is the xy plane."""
    return np.eye(4), np.array([[1.0, 0, 0], [0, 1.0, 0]])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_invariants(dtype):
    P, A = _flat_camera(48)
    # one clip, two frames, three joints: a horizontal bone at y = 30 (after the floor shift) and a joint far below that sets the floor
    j = np.zeros((1, 2, 3, 3), np.float32)
    j[0, :, 0] = (10.0, 30.0, 0.0)
    j[0, :, 1] = (40.0, 30.0, 0.0)
    j[0, :, 2] = (10.0, 0.0, 0.0)
    kw = dict(dtype=dtype, proj=P, affine=A, W=48, H=48, scale=1.0)
    img = rf.render(j, [[0, 1]], **kw)
    u8 = rf.quantise(img)
    assert img.dtype == dtype and img.shape == (1, 2, 48, 48, 3)
    # points are seen from the root (10, ., 0): the bone runs from x = 0 to x = 30 at y = 30; pixel row 48 - 30 - 0.5 -> centres at 29.5, 30.5
    row, col = 48 - 30, 15
    assert np.array_equal(u8[0, 0, row, col], rf.PALETTE[1, 0]) and np.array_equal(u8[0, 0, row - 1, col], rf.PALETTE[1, 0])
    assert np.array_equal(u8[0, 0, 5, 40], (255, 255, 255))              # background; the quad is degenerate here (z extent 0)
    assert np.array_equal(u8[0, 0], u8[0, 1])
    # a quad alone: the joints spread in x and z, looked at from above (y up in the image is -z here)
    top = np.array([[1.0, 0, 0, 0], [0, 0, 1.0, 0], [0, 1.0, 0, 0], [0, 0, 0, 1.0]])
    q = np.zeros((1, 1, 2, 3), np.float32)
    q[0, 0, 0] = (8.0, 0.0, 8.0)
    q[0, 0, 1] = (40.0, 0.0, 40.0)
    quad = rf.quantise(rf.render(q, [], **dict(kw, proj=top, affine=np.array([[1.0, 0, 8.0], [0, 1.0, 8.0]]))))
    assert np.array_equal(quad[0, 0, 48 - 20, 20], (191, 191, 191)) and np.array_equal(quad[0, 0, 2, 2], (255, 255, 255))
    # a trace of one point draws nothing: frame 1 of a root trace has one point, of a joint trace two
    w = rf.walk(3, 1, 4, 22)
    Pd, Ad = ps.default_camera(48, 48)
    kd = dict(dtype=dtype, proj=Pd, affine=Ad, W=48, H=48)
    plain = rf.render(w, rf.chains_of(22), **kd)
    traced = rf.render(w, rf.chains_of(22), traces=[(rf.ROOT, 0)], **kd)
    assert np.array_equal(plain[0, :2], traced[0, :2]) and not np.array_equal(plain[0, 3], traced[0, 3])
    # a sub-range equals the slice; frames behind the length are zeros
    both = rf.render(w, rf.chains_of(22), traces=[(rf.ROOT, 0), (rf.JOINT, 7)], **kd)
    assert np.array_equal(rf.render(w, rf.chains_of(22), traces=[(rf.ROOT, 0), (rf.JOINT, 7)], frames=(2, 4), **kd), both[:, 2:4])
    short = rf.render(w, rf.chains_of(22), [2], **kd)
    assert not short[0, 2:].any() and short[0, :2].any()
    # 0 in the overlay leaves a pixel untouched, 255 makes it black
    ov = np.zeros((1, 48, 48), np.uint8)
    ov[0, :5] = 255
    over = rf.render(w, rf.chains_of(22), overlay=ov, **kd)
    assert not over[0, :, :5].any() and np.array_equal(over[0, :, 5:], plain[0, :, 5:])


def test_restatement_in_float32_is_close_to_float64():
    w = rf.walk(4, 1, 3, 21)
    P, A = ps.default_camera(37, 29)
    f32, f64 = (rf.render(w, rf.chains_of(21), dtype=dt, proj=P, affine=A, W=37, H=29, traces=[(rf.ROOT_HORIZONTAL, 0)]) for dt in (np.float32, np.float64))
    assert f32.dtype == np.float32 and 0 < rf.distance(f32, f64) < 1e-4
    assert np.abs(rf.quantise(f32).astype(int) - rf.quantise(f64).astype(int)).max() <= 1


# ------------------------------------------------------------------------------------------ files and titles
def _frames(T=5, H=16, W=20):
    g = np.random.default_rng(1)
    return g.integers(0, 256, (T, H, W, 3), dtype=np.uint8)


def test_save_frames_npy_round_trip(tmp_path):
    f = _frames()
    assert np.array_equal(np.load(ps.save_frames(tmp_path / "a.npy", f)), f)
    assert np.array_equal(np.load(ps.save_frames(tmp_path / "b.npy", torch.from_numpy(f), chunk=2)), f)
    assert np.array_equal(np.load(ps.save_frames(tmp_path / "c.npy", (f[s:s + 2] for s in range(0, 5, 2)))), f)     # pieces, as render_to_file hands them over
    with pytest.raises(ValueError, match="none of"):
        ps.save_frames(tmp_path / "a.avi", f)
    with pytest.raises(ValueError, match="uint8"):
        ps.save_frames(tmp_path / "d.npy", f.astype(np.float32))


def test_save_frames_gif_and_png_round_trip(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    f = np.zeros((3, 16, 20, 3), np.uint8)                  # few colours: a GIF's palette holds them exactly
    f[0, :8] = (255, 0, 0)
    f[1, :, :10] = (0, 255, 0)
    f[2, 4:12, 5:15] = (0, 0, 255)
    ps.save_frames(tmp_path / "a.gif", f, fps=10)
    with Image.open(tmp_path / "a.gif") as im:
        assert im.n_frames == 3
        for i in range(3):
            im.seek(i)
            assert np.array_equal(np.asarray(im.convert("RGB")), f[i])
    g = _frames(3)
    ps.save_frames(tmp_path / "b.png", g)
    for i in range(3):
        with Image.open(tmp_path / f"b_{i:04d}.png") as im:
            assert np.array_equal(np.asarray(im), g[i])


def test_save_frames_mp4_without_ffmpeg_raises_the_named_error(tmp_path, monkeypatch):
    monkeypatch.setenv("PATH", str(tmp_path))                # a PATH that holds no ffmpeg
    with pytest.raises(ps.FfmpegNotFound, match="ffmpeg"):
        ps.save_frames(tmp_path / "a.mp4", _frames())
    assert not (tmp_path / "a.mp4").exists()


def test_title_overlay_stays_in_the_top_strip():
    pytest.importorskip("PIL")
    mask = ps.title_overlay("a person walks forward and then turns around slowly", 300, 300)
    assert mask.shape == (300, 300) and mask.dtype == np.uint8
    assert mask[:60].any() and not mask[60:].any()
    small = ps.title_overlay("walk", 16, 16)
    assert small.shape == (16, 16) and not small[3:].any()
