"""k_mesh_bounds / k_mesh_vertices / k_mesh_frames (csrc/mst_mesh.h) behind `render_meshes` against tests/mesh_fixture.py's restatements.

Per case the float image and the face-index image equal the float32 restatement bit for bit (asserted: the kernels achieve it).  The
bar that must hold is the project's: max |kernel - f64| <= 4 x the float32 restatement's own max |f32 - f64|, floor 1e-6, measured
over the pixels whose winning faces agree between the kernel's index images (every sub-sample) and the float64 restatement's; the
pixels left out are silhouette or tie flips, at most 1 % of the pixels any face covers and none in the one-triangle and tie cases
(tests/test_mesh_cpu.py holds the float32 restatement to the same cap without a GPU).  The uint8 image is exactly floor(255 f + 0.5)
of the kernel's own float image and within one level of float64 on the agreeing pixels.  Every case's images are computed once.
Measured on an MI355X: kernel vs the float32 restatement 0 on all fourteen cases (images and indices), so kernel vs float64 is the
restatement's own 4.5e-8 .. 2.4e-6 against bars of 1e-6 .. 9.6e-6; one pixel of `two_chunks` (0.19 % of its covered pixels) changes
winner against float64; 37 tests in 12 s.

One reading differs from the issue's list: sub-sample 0 of samples = 3 lies at (1/6, 1/6) of the pixel and the only sample of
samples = 1 at its centre, so their winners differ along every silhouette; what is the same point is the CENTRE sub-sample (index 4)
of samples = 3, and that is what `test_ids_at_the_pixel_centre_are_the_same_for_samples_1_and_3` compares (`ids_sample=`)."""
import os

import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
import mesh_fixture as mf
from mst_amd.visualize import mesh_render as mr

pytestmark = pytest.mark.gpu
NAMES = ["b1_t1_16", "b1_t2_37x29", "tie_32", "shared_edge_33", "behind_32", "zero_area_32", "chunk_plus_1", "two_chunks", "ico_96_s1",
         "ico_96_s2", "ico_96_s3", "b3_t9", "b33_t9_37x29", "mesh_camera_300"]
_CASES = None
_DONE = {}


def case(name):
    global _CASES
    if _CASES is None:
        _CASES = mf.cases(mr.limits()["chunk"])
        assert sorted(_CASES) == sorted(NAMES)
    return _CASES[name]


def gpu_render(c, stream=None, layout="frames", **over):
    """-> (uint8, float, ids at `ids_sample`) as numpy."""
    c = dict(c, **over)
    dev = torch.device("cuda:0")
    H, W = c["size"]
    cam = c.get("camera")
    kw = dict(lengths=c.get("lengths"), width=W, height=H, samples=c["samples"], frames=c.get("frames"),
              camera=None if isinstance(cam, str) else mf.case_camera(c, mr.mesh_camera, mr.mesh_affine), layout=layout,
              return_float=True, return_ids=True, ids_sample=c.get("ids_sample", 0))
    if "budget" in c:
        kw["budget"] = c["budget"]
    v = torch.from_numpy(c["verts"]).to(dev)
    if layout == "reference":
        v = v.permute(0, 2, 3, 1).contiguous()               # [B, V, 3, T], as Rotation2xyz writes them
    if stream is None:
        got = mr.render_meshes(v, c["faces"], **kw)
    else:
        stream.wait_stream(torch.cuda.current_stream(dev))
        got = mr.render_meshes(v, c["faces"], stream=stream, **kw)
        stream.synchronize()
    torch.cuda.synchronize()
    return tuple(g.cpu().numpy() for g in got)


def done(name):
    if name not in _DONE:
        c = case(name)
        u8, f, ids0 = gpu_render(c)
        ids = [ids0] + [gpu_render(c, ids_sample=k)[2] for k in range(1, c["samples"] ** 2)]
        ids = np.stack(ids, 2)                               # [B, T, S * S, H, W]
        f32, f64 = (mf.restate(c, dt, mr.mesh_camera, mr.mesh_affine) for dt in (np.float32, np.float64))
        agree, flips = mf.agreement(ids, f64["ids"], f64["covered"])
        own, got = mf.distance(f32["img"], f64["img"], agree), mf.distance(f, f64["img"], agree)
        print(f"{name}: covered {int(f64['covered'].sum())}, flips left out {flips:.4%}; kernel vs f64 {got:.3e}; f32 restatement vs f64 "
              f"{own:.3e}; bar {mf.bar(own):.3e}; kernel vs f32 restatement {mf.distance(f, f32['img']):.3e}, ids differing "
              f"{int((ids != f32['ids']).sum())}")
        _DONE[name] = dict(u8=u8, f=f, ids=ids, f32=f32, f64=f64, agree=agree, flips=flips, own=own, got=got)
    return _DONE[name]


# ------------------------------------------------------------------------------------------ against the restatements
@pytest.mark.parametrize("name", NAMES)
def test_float_and_index_images(name):
    r = done(name)
    assert r["f"].dtype == np.float32 and r["f"].shape == r["f64"]["img"].shape and r["ids"].dtype == np.int32
    assert np.isfinite(r["f"]).all() and r["f"].min() >= 0.0 and r["f"].max() <= 1.0
    assert r["f64"]["covered"].any() and (r["ids"] >= 0).any()               # something is drawn
    assert r["flips"] <= (0.0 if case(name).get("strict") else mf.FLIP_CAP), (name, r["flips"])
    assert r["got"] <= mf.bar(r["own"]), (name, r["got"], r["own"])
    # bit for bit the float32 restatement: the kernels achieve it
    assert np.array_equal(r["ids"], r["f32"]["ids"])
    assert np.array_equal(r["f"], r["f32"]["img"])


@pytest.mark.parametrize("name", NAMES)
def test_uint8_image(name):
    r = done(name)
    assert r["u8"].dtype == np.uint8
    assert np.array_equal(r["u8"], mf.quantise(r["f"]))      # exactly floor(255 f + 0.5) of the kernel's own float image
    want = mf.quantise(r["f64"]["img"]).astype(np.int16)
    worst = int(np.abs(r["u8"].astype(np.int16) - want)[r["agree"]].max())
    print(f"{name}: levels from the f64 image on the agreeing pixels: {worst}")
    assert worst <= 1


def test_cases_are_what_they_claim():
    chunk = mr.limits()["chunk"]
    assert len(case("chunk_plus_1")["faces"]) == chunk + 1 and len(case("two_chunks")["faces"]) == 2 * chunk
    assert set(np.unique(done("behind_32")["ids"])) == {-1, 0}                # the face with a vertex behind the camera is dropped whole
    assert set(np.unique(done("zero_area_32")["ids"])) == {-1, 0, 1}
    t = done("tie_32")
    both = (t["f64"]["ids"] == 0) & (t["ids"] == 0)
    assert both.sum() > 50 and set(np.unique(t["ids"])) == {-1, 0, 1}
    e = done("shared_edge_33")["ids"][0, 0, 0]
    assert (e[8:25, 16] == 0).all()                                          # the shared edge's pixel centres: no gap, the lower face
    last = done("two_chunks")["ids"]
    assert last.max() >= chunk                                               # faces of the second chunk win somewhere


# ------------------------------------------------------------------------------------------ position independence and isolation
def test_a_clips_frames_do_not_depend_on_the_batch_the_stream_the_range_or_other_rows():
    c = case("b33_t9_37x29")
    pick, n = 6, 7                                           # lengths[6] = 9 - 2
    assert c["lengths"][pick] == n
    full = done("b33_t9_37x29")
    want = tuple(full[k][pick] for k in ("u8", "f")) + (full["ids"][pick, :, 0],)
    assert not want[0][n:].any() and not want[1][n:].any() and (want[2][n:] == -1).all() and want[0][:n].any()
    for b, length in enumerate(c["lengths"]):                # exact zeros at and behind every length
        assert not full["u8"][b, length:].any() and not full["f"][b, length:].any() and (full["ids"][b, length:] == -1).all()

    def same(got, b=0, sl=slice(None)):
        return all(np.array_equal(g[b], w[sl]) for g, w in zip(got, want))

    assert same(gpu_render(c, verts=c["verts"][pick:pick + 1], lengths=[n]))                          # alone
    for place in (0, 32):                                                                            # first and last in the batch
        order = [b for b in range(33) if b != pick]
        order.insert(place, pick)
        assert same(gpu_render(c, verts=c["verts"][order], lengths=[c["lengths"][b] for b in order]), place), place
    assert same(gpu_render(c, stream=torch.cuda.Stream()), pick)                                     # on a side stream
    assert same(gpu_render(c, frames=(2, 6)), pick, slice(2, 6))                                     # under frames=
    per = mr.frame_bytes(33, c["verts"].shape[2], 29, 37, True, True)
    assert len(mr.plan_frame_chunks(0, 9, per, per)) == 9
    assert same(gpu_render(c, budget=per), pick)                                                     # chunks of one frame, copied in
    assert same(gpu_render(c, verts=c["verts"][pick:pick + 1], lengths=[n], budget=1))               # one clip: chunks written in place
    poisoned = np.full_like(c["verts"], np.nan)
    poisoned[pick, :n] = c["verts"][pick, :n]
    assert same(gpu_render(c, verts=poisoned), pick)                                                 # NaN everywhere else


@pytest.mark.parametrize("rng", [(0, 1), (8, 9), (3, 6)])
def test_frame_sub_range_equals_the_slice(rng):
    c = case("b3_t9")
    got = gpu_render(c, frames=rng)
    r = done("b3_t9")
    assert got[0].shape == (3, rng[1] - rng[0], 48, 48, 4)
    assert np.array_equal(got[0], r["u8"][:, rng[0]:rng[1]]) and np.array_equal(got[1], r["f"][:, rng[0]:rng[1]])
    assert np.array_equal(got[2], r["ids"][:, rng[0]:rng[1], 0])


def test_both_vertex_layouts_read_the_same_clip_in_place():
    for name in ("b3_t9", "mesh_camera_300"):
        got = gpu_render(case(name), layout="reference")
        assert np.array_equal(got[0], done(name)["u8"]) and np.array_equal(got[1], done(name)["f"])


def test_ids_at_the_pixel_centre_are_the_same_for_samples_1_and_3():
    one, three = done("ico_96_s1")["ids"], done("ico_96_s3")["ids"]
    assert one.shape[2] == 1 and three.shape[2] == 9
    assert np.array_equal(one[:, :, 0], three[:, :, 4])      # (1 + 0.5) / 3 = 0.5 exactly: the same point
    assert not np.array_equal(one[:, :, 0], three[:, :, 0])  # sub-sample 0 of samples = 3 is another point: the silhouette moves


def test_default_colours_and_given_colours():
    c = case("b3_t9")
    dev = torch.device("cuda:0")
    v = torch.from_numpy(c["verts"]).to(dev)
    P, A = mf.case_camera(c, mr.mesh_camera, mr.mesh_affine)
    kw = dict(lengths=c["lengths"], width=48, height=48, camera=(P, A), layout="frames")
    ramp = mr.render_meshes(v, c["faces"], **kw)
    given = mr.render_meshes(v, c["faces"], colors=mr.default_colors(9), **kw)
    assert int((ramp.int() - given.int()).abs().max()) <= 1                  # the ramp in float32 on the device, in float64 on the host
    red = np.zeros((9, 4), np.float32)
    red[:, 0] = red[:, 3] = 1.0
    img = mr.render_meshes(v, c["faces"], colors=red, bg=(0, 0, 0, 0), **kw).cpu().numpy()
    inside = done("b3_t9")["ids"][0, 0].min(0) >= 0
    assert (img[0, 0][inside][:, 1:3] == 0).all() and (img[0, 0][inside][:, 3] == 255).all() and (img[0, 0][inside][:, 0] >= 102).all()
    assert not img[0, 0][~done("b3_t9")["f64"]["covered"][0, 0]].any()


# ------------------------------------------------------------------------------------------ the reference's entry point
def test_render_final_runs_end_to_end_and_reads_its_cache(tmp_path, capsys):
    pytest.importorskip("PIL")
    from PIL import Image
    import smplify_fixture as xf
    from mst_amd.model import smpl
    from mst_amd.visualize import render_final
    from mst_amd.visualize.joints2smpl.src.prior import MaxMixturePrior
    body = smpl.SMPLBody.from_arrays(**xf.body83(), device=torch.device("cuda:0"))
    init_pose, _, j3d = xf.fit_inputs(22)
    render_final.configure(body=body, pose_prior=MaxMixturePrior.from_arrays(**xf.GMM), mean_pose=init_pose[0].numpy(),
                           mean_shape=np.zeros(10, np.float32), num_smplify_iters=2, width=64, height=48)
    try:
        outdir = str(tmp_path) + os.sep
        motions = j3d.numpy().copy()
        low = motions[:, :, 1].min()
        frames = render_final.render(motions, outdir=outdir, name="clip", pred=True)
        assert motions[:, :, 1].min() == 0.0 and low != 0.0                  # the height offset, in place, as the reference
        assert frames.is_cuda and tuple(frames.shape) == (4, 48, 64, 4) and frames.dtype == torch.uint8
        assert os.path.exists(outdir + "clip_pred.pt") and sorted(os.listdir(outdir + "clip")) == ["0_pred.png", "pred.gif"]
        with Image.open(outdir + "clip/0_pred.png") as im:
            assert im.mode == "RGBA" and np.array_equal(np.asarray(im), frames[0].cpu().numpy())
        with Image.open(outdir + "clip/pred.gif") as im:
            assert im.n_frames == 4
        host = frames.cpu().numpy()
        assert (host[..., 3] == 204).any() and (host[..., 3] > 204).any()    # background alpha 0.8, the body's 0.98
        first = {n: open(outdir + "clip/" + n, "rb").read() for n in ("0_pred.png", "pred.gif")}
        capsys.readouterr()
        again = render_final.render(j3d.numpy().copy(), outdir=outdir, name="clip", pred=True)
        assert "clip_pred.pt" in capsys.readouterr().out                     # the cache was read, as the reference prints
        assert torch.equal(again, frames)
        assert first == {n: open(outdir + "clip/" + n, "rb").read() for n in first}
        render_final.render(j3d.numpy().copy(), outdir=outdir, name="clip", pred=False)
        assert os.path.exists(outdir + "clip_gt.pt") and os.path.exists(outdir + "clip/gt.gif")
    finally:
        render_final.configure()
    with pytest.raises(RuntimeError, match="no SMPL body"):
        render_final.render(j3d.numpy().copy(), outdir=str(tmp_path) + os.sep, name="x")
