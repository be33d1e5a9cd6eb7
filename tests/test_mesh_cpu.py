"""The mesh render path without a GPU: the C ABI's declarations and refusals, the CSR builder, the cameras against independent float64
constructions, the colour ramp, the frame-chunk planner, the invariants of tests/mesh_fixture.py's restatement, and the condition of
the GPU cases: the float32 restatement itself keeps the flip cap on every one of them.

The refusals go to the real library, which needs no device to refuse (as tests/test_render_cpu.py does): tests/lib_stub.py's recording
stub accepts everything, so it serves the other half -- that `render_meshes` raises on the host before any entry point is called."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
import lib_stub
import mesh_fixture as mf
from conftest import ROOT
from mst_amd import _native
from mst_amd.visualize import mesh_render as mr

NEW = ("mst_mesh_bounds", "mst_mesh_vertices", "mst_mesh_frames", "mst_mesh_workspace_bytes", "mst_mesh_max_vertices",
       "mst_mesh_max_faces", "mst_mesh_max_side", "mst_mesh_max_samples", "mst_mesh_chunk")


# ------------------------------------------------------------------------------------------ the C ABI
def test_symbols_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "mst_engine.h")) as fh:
        header = fh.read()
    lib = _native.lib()
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _native.SIGNATURES and getattr(lib, name).argtypes == _native.SIGNATURES[name][1]
    assert "render_final.py:79-89" in header and "no near-plane" in header
    lim = mr.limits()
    assert (lim["vertices"], lim["faces"], lim["side"], lim["samples"]) == (32768, 65536, 1024, 4)
    assert lim["chunk"] >= 64 and lim["chunk"] % 256 == 0
    assert lib.mst_mesh_workspace_bytes(2, 3, 300) == 2 * 3 * (5 * 300 + 4 * 2) * 4
    assert lib.mst_mesh_workspace_bytes(2, 3, 300) == mr.frame_bytes(2, 300, 0, 0) * 3
    assert lib.mst_mesh_workspace_bytes(0, 3, 300) == 0 and lib.mst_mesh_workspace_bytes(1, 1, 32769) == 0


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def test_abi_refusals_need_no_gpu():
    lib = _native.lib()
    ok, ws, out, outf, oid = 4096, 8192, 16384, 32768, 65536      # never dereferenced: every call below is refused first
    v, faces = mf.quad()
    off, adj = mf.adjacency(faces, 4)
    P = np.ascontiguousarray(np.eye(4).reshape(1, 16), np.float32)

    def call(entry="frames", scene_null=False, view_null=False, **kw):
        s = dict(verts=ok, strides=(48, 12, 3, 1), lengths=None, batch=2, frames=4, V=4, F=2, faces=_i32(faces), faces_dev=ok + 16,
                 off=_i32(off), off_dev=ok + 32, adj=_i32(adj), adj_dev=ok + 48, proj=P, proj_dev=ok + 64, pb=1, affine=[8, 0, 8, 0, 8, 8],
                 W=16, H=16, S=2, light=[0, 0, 1], ambient=0.4, colors=None, bg=[1, 1, 1, 0.8], t0=0, t1=4, ids_sample=0, ws=ws, wsb=1 << 20,
                 out=out, outf=None, oid=None, bounds=out)
        assert set(kw) <= set(s), set(kw) - set(s)
        s.update(kw)
        host = lambda a: None if a is None else a.ctypes.data      # noqa: E731
        scene = _native.MstMeshScene(s["verts"], *s["strides"], s["lengths"], s["batch"], s["frames"], s["V"], s["F"], host(s["faces"]),
                                     s["faces_dev"], host(s["off"]), s["off_dev"], host(s["adj"]), s["adj_dev"])
        view = _native.MstMeshView()
        view.proj_host, view.proj_dev, view.proj_batch = host(s["proj"]), s["proj_dev"], s["pb"]
        view.affine = (C.c_float * 6)(*s["affine"])
        view.width, view.height, view.samples = s["W"], s["H"], s["S"]
        view.light = (C.c_float * 3)(*s["light"])
        view.ambient, view.colors_dev = s["ambient"], s["colors"]
        view.background = (C.c_float * 4)(*s["bg"])
        view.t0, view.t1, view.ids_sample = s["t0"], s["t1"], s["ids_sample"]
        sp, vp = (None if scene_null else C.byref(scene)), (None if view_null else C.byref(view))
        if entry == "bounds":
            return lib.mst_mesh_bounds(sp, s["bounds"], None)
        if entry == "vertices":
            return lib.mst_mesh_vertices(sp, vp, s["ws"], s["wsb"], None)
        return lib.mst_mesh_frames(sp, vp, s["ws"], s["wsb"], s["out"], s["outf"], s["oid"], None)

    bad_face, bad_adj, bad_off = faces.copy(), adj.copy(), off.copy()
    bad_face[1, 2] = 4
    bad_adj[3] = 2
    bad_off[4] -= 1
    falling = off.copy()
    falling[2] = falling[1] - 1
    nanP = P.copy()
    nanP[0, 5] = np.nan
    need = lib.mst_mesh_workspace_bytes(2, 4, 4)
    cases = [
        (dict(scene_null=True), b"null scene"), (dict(view_null=True), b"null view"), (dict(verts=None), b"null vertices"),
        (dict(batch=0), b"batch"), (dict(batch=65536), b"batch"), (dict(frames=0), b"frames"), (dict(frames=65536), b"frames"),
        (dict(V=0), b"vertices 0"), (dict(V=32769), b"vertices 32769"), (dict(F=0), b"faces 0"), (dict(F=65537), b"faces 65537"),
        (dict(strides=(48, 12, 0, 1)), b"strides"), (dict(strides=(48, 12, 3, -1)), b"strides"),
        (dict(faces=None), b"null faces"), (dict(faces_dev=None), b"null faces"), (dict(off=None), b"null adjacency"),
        (dict(adj_dev=None), b"null adjacency"), (dict(faces=_i32(bad_face)), b"face 1 names vertex 4"),
        (dict(faces=_i32(-faces - 1)), b"face 0 names vertex -1"), (dict(off=_i32(bad_off)), b"adjacency rows sum to 5"),
        (dict(off=_i32(falling)), b"adjacency offsets fall at vertex 1"), (dict(adj=_i32(bad_adj)), b"adjacency entry 3 names face 2"),
        (dict(proj=None), b"null matrix"), (dict(proj_dev=None), b"null matrix"), (dict(pb=3), b"3 matrices for 2 clips"),
        (dict(proj=nanP), b"not finite"), (dict(affine=[8, 0, float("inf"), 0, 8, 8]), b"not finite"),
        (dict(W=15), b"image"), (dict(H=1025), b"image"), (dict(W=1025), b"image"), (dict(H=15), b"image"),
        (dict(S=0), b"samples 0"), (dict(S=5), b"samples 5"), (dict(ids_sample=4), b"ids_sample"), (dict(ids_sample=-1), b"ids_sample"),
        (dict(light=[0, float("nan"), 1]), b"light"), (dict(ambient=float("inf")), b"ambient"), (dict(bg=[1, 1, float("nan"), 1]), b"background"),
        (dict(t0=-1), b"frame range"), (dict(t0=2, t1=2), b"frame range"), (dict(t1=5), b"frame range"), (dict(t0=3, t1=1), b"frame range"),
        (dict(ws=None), b"null workspace"), (dict(wsb=need - 1), b"mst_mesh_workspace_bytes says"), (dict(ws=ws + 2), b"workspace is not 4-byte aligned"),
        (dict(out=None), b"null output"), (dict(out=out + 1), b"aligned"), (dict(outf=outf + 4), b"aligned"), (dict(oid=oid + 2), b"aligned"),
        (dict(out=ok), b"an output may not be an input"), (dict(outf=ws), b"an output may not be an input"),
        (dict(oid=ok + 16), b"an output may not be an input"), (dict(colors=outf, outf=outf), b"an output may not be an input"),
        (dict(lengths=out), b"an output may not be an input"), (dict(outf=out), b"may not share"), (dict(outf=outf, oid=outf), b"may not share"),
        (dict(entry="vertices", ws=ok), b"the workspace may not be an input"), (dict(entry="vertices", V=0), b"mst_mesh_vertices: vertices"),
        (dict(entry="vertices", wsb=need - 1), b"mst_mesh_vertices: workspace"), (dict(entry="vertices", S=5), b"mst_mesh_vertices: samples"),
        (dict(entry="vertices", faces=_i32(bad_face)), b"mst_mesh_vertices: face 1"), (dict(entry="vertices", view_null=True), b"null view"),
        (dict(entry="bounds", batch=0), b"mst_mesh_bounds: batch"), (dict(entry="bounds", V=32769), b"mst_mesh_bounds: vertices"),
        (dict(entry="bounds", verts=None), b"mst_mesh_bounds: null vertices"), (dict(entry="bounds", bounds=None), b"null bounds"),
        (dict(entry="bounds", bounds=ok), b"may not be an input"), (dict(entry="bounds", scene_null=True), b"null scene"),
        (dict(entry="bounds", strides=(0, 12, 3, 1)), b"mst_mesh_bounds: strides"),
    ]
    for kw, word in cases:
        assert call(**kw) != 0, kw
        assert word in lib.mst_last_error(), (kw, lib.mst_last_error())


def test_python_argument_checks_raise_before_any_entry_point(monkeypatch):
    stub = lib_stub.install(monkeypatch)
    v = torch.zeros(2, 4, 3, 5)
    _, faces = mf.quad()
    for kw, err in ((dict(vertices=v.numpy()), TypeError), (dict(layout="guess"), ValueError), (dict(vertices=v[0]), ValueError),
                    (dict(vertices=v.permute(0, 3, 1, 2)), ValueError),             # [B, T, V, 3] without layout='frames': never guessed
                    (dict(width=15), ValueError), (dict(height=1025), ValueError), (dict(samples=0), ValueError), (dict(samples=5), ValueError),
                    (dict(ids_sample=4), ValueError), (dict(frames=(0, 6)), ValueError), (dict(frames=(2, 2)), ValueError),
                    (dict(lengths=[5]), ValueError), (dict(lengths=[5, 0]), ValueError), (dict(lengths=[5, 6]), ValueError),
                    (dict(faces_or_topology=np.array([[0, 1, 4]])), ValueError), (dict(faces_or_topology=np.zeros((2, 4), int)), ValueError),
                    (dict(faces_or_topology=np.zeros((2, 3))), ValueError), (dict(light=(0, 0, 0)), ValueError), (dict(light=(0, 1)), ValueError),
                    (dict(bg=(1, 1, 1)), ValueError), (dict(ambient=float("nan")), ValueError), (dict(colors=np.zeros((4, 4))), ValueError),
                    (dict(colors=np.full((5, 4), np.nan)), ValueError), (dict(camera=(np.eye(3), np.zeros((2, 3)))), ValueError),
                    (dict(camera=(np.full((4, 4), np.inf), np.zeros((2, 3)))), ValueError), (dict(out=torch.zeros(2, 5, 16, 16, 3, dtype=torch.uint8)), ValueError),
                    (dict(), RuntimeError)):                                        # a CPU tensor: there is no CPU path
        args = dict(vertices=v, faces_or_topology=faces, width=16, height=16)
        args.update(kw)
        with pytest.raises(err):
            mr.render_meshes(**args)
    assert stub.lib.calls == []


# ------------------------------------------------------------------------------------------ topology
@pytest.mark.parametrize("mesh", ["quad", "ico", "blob", "degenerate"])
def test_csr_builder_equals_the_brute_force_adjacency(mesh):
    v, f = {"quad": mf.quad, "ico": lambda: mf.icosphere(2), "blob": lambda: mf.blob(131, 700),
            "degenerate": lambda: (np.zeros((6, 3), np.float32), np.array([[0, 0, 3], [5, 3, 3], [3, 0, 5]], np.int32))}[mesh]()
    V = len(v)
    topo = mr.MeshTopology(f, V)
    off, adj = mf.adjacency(f, V)
    assert topo.adj_offsets.dtype == np.int32 and topo.adj_faces.dtype == np.int32 and topo.faces.flags.c_contiguous
    assert np.array_equal(topo.adj_offsets, off) and np.array_equal(topo.adj_faces, adj)
    assert topo.adj_offsets[-1] == 3 * len(f) and (np.diff(topo.adj_offsets) >= 0).all()
    for k in range(V):
        row = topo.adj_faces[topo.adj_offsets[k]:topo.adj_offsets[k + 1]]
        assert (np.diff(row) >= 0).all() and all(k in f[i] for i in row)
    assert mr.MeshTopology(f).num_vertices == int(f.max()) + 1


def test_smpl_body_caches_its_topology():
    import smpl_fixture as sf
    from mst_amd.model import smpl
    body = smpl.SMPLBody.from_arrays(**sf.synthetic_body(83), device="cpu")
    topo = body.topology
    assert topo is body.topology and topo is smpl.SMPL(body).topology
    assert topo.num_vertices == 83 and np.array_equal(topo.faces, body.faces)


# ------------------------------------------------------------------------------------------ cameras, colours, planner
def test_mesh_camera_equals_the_gltf_formula_and_the_inverse_pose():
    g = np.random.default_rng(5)
    for _ in range(6):
        lo = g.uniform(-3, 0.5, 3)
        hi = lo + g.uniform(0.1, 6, 3)
        aspect, yfov, n = g.uniform(0.5, 2), g.uniform(0.6, 1.6), g.uniform(0.01, 0.2)
        minx, maxx, minz = lo[0] - 0.5, hi[0] + 0.5, lo[2] - 0.5
        c = -np.pi / 6
        pose = np.array([[1, 0, 0, (minx + maxx) / 2], [0, np.cos(c), -np.sin(c), 1.5],
                         [0, np.sin(c), np.cos(c), max(4, minz + (1.5 - lo[1]) * 2, maxx - minx)], [0, 0, 0, 1]])
        P = np.zeros((4, 4))                                 # glTF: the infinite perspective projection matrix
        P[0, 0], P[1, 1], P[2, 2], P[2, 3], P[3, 2] = 1 / (aspect * np.tan(0.5 * yfov)), 1 / np.tan(0.5 * yfov), -1, -2 * n, -1
        want = P @ np.linalg.inv(pose)
        got = mr.mesh_camera(np.concatenate([lo, hi]), yfov=yfov, znear=n, aspect=aspect)
        assert got.shape == (4, 4) and np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    b = np.array([[-1, 0, -1, 1, 1.8, 1, 0, 0], [-4, 0.1, 3, 4, 2, 5, 0, 0]], np.float32)       # k_mesh_bounds' rows, a batch
    both = mr.mesh_camera(b)
    assert both.shape == (2, 4, 4) and np.array_equal(both[1], mr.mesh_camera(b[1, :6]))
    assert both[0, 3, 3] == pytest.approx(-(np.sin(-np.pi / 6) * 1.5 - np.cos(-np.pi / 6) * 4.0))       # z = max(4, ...) = 4
    assert mr.mesh_camera(b[1])[0, 3] == 0 and mr.mesh_camera(b[1] + np.float32(1))[0, 3] != 0
    A = mr.mesh_affine(960, 480)
    assert np.array_equal(A @ [-1, -1, 1], [0, 0]) and np.array_equal(A @ [1, 1, 1], [960, 480])
    with pytest.raises(ValueError):
        mr.mesh_camera(np.zeros(5))


def test_weak_perspective_camera_equals_the_references_four_lines():
    from mst_amd.visualize import render_final
    scale, translation = (0.75, 0.6), (0.2, 0.1)
    P = np.eye(4)
    P[0, 0] = scale[0]
    P[1, 1] = scale[1]
    P[0, 3] = translation[0] * scale[0]
    P[1, 3] = -translation[1] * scale[1]
    P[2, 2] = -1
    assert np.array_equal(mr.weak_perspective_camera(scale, translation), P)
    assert np.array_equal(render_final.WeakPerspectiveCamera(scale, translation).get_projection_matrix(960, 960), P)


def test_default_colour_ramp_and_its_clamp():
    c = mr.default_colors(300)
    assert c.shape == (300, 4) and (c[:, 0] == 1).all() and (c[:, 3] == 0.9).all()
    assert np.allclose(c[0], [1, 145 / 255, 33 / 255, 0.9]) and np.allclose(c[10, 1:3], [153 / 255, 38 / 255])
    assert c[137, 1] < 1 and c[138, 1] == 1 and (c[138:, 1] == 1).all()          # green passes 255 at n = 138
    assert c[:, 2].max() < 1 and (np.diff(c[:, 2]) > 0).all()
    for dt in (np.float32, np.float64):
        assert np.abs(mf.default_colors(300, dt) - c).max() < (1e-6 if dt is np.float32 else 1e-15)


def test_frame_chunk_planner():
    per = mr.frame_bytes(8, 6890, 960, 960)
    assert per == 8 * ((5 * 6890 + 4 * 27) * 4 + 960 * 960 * 4)
    assert mr.frame_bytes(1, 256, 16, 16, True, True) == (5 * 256 + 4) * 4 + 256 * 24
    n = (4 << 30) // per                                     # 8 clips at 960 x 960 under the default 4 GiB: two chunks
    assert 98 <= n < 196 and mr.plan_frame_chunks(0, 196, per) == [(0, n), (n, 196)]
    assert mr.plan_frame_chunks(3, 8, 100, budget=250) == [(3, 5), (5, 7), (7, 8)]
    assert mr.plan_frame_chunks(0, 3, 100, budget=1) == [(0, 1), (1, 2), (2, 3)]  # never fewer than one frame
    assert mr.plan_frame_chunks(0, 3, 100, budget=10 ** 9) == [(0, 3)]
    with pytest.raises(ValueError):
        mr.plan_frame_chunks(3, 3, 100)


# ------------------------------------------------------------------------------------------ the restatement's own invariants
CASES = mf.cases(_native.lib().mst_mesh_chunk())
_DONE = {}


def both(name):
    if name not in _DONE:
        c = CASES[name]
        _DONE[name] = tuple(mf.restate(c, dt, mr.mesh_camera, mr.mesh_affine) for dt in (np.float32, np.float64))
    return _DONE[name]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_invariants(dtype):
    k = 0 if dtype is np.float32 else 1
    # a shared edge through pixel centres leaves no gap: every centre on it is covered, and goes to the lower face
    r = both("shared_edge_33")[k]
    ids = r["ids"][0, 0, 0]
    col = ids[:, 16]
    rows = np.arange(33)
    on_edge = (33 - rows - 0.5 >= 8.5) & (33 - rows - 0.5 <= 24.5)
    assert (col[on_edge] == 0).all() and (col[~on_edge] == -1).all()
    assert (ids[16, 9:22] >= 0).all() and set(ids[16, 9:17]) == {0} and set(ids[16, 17:22]) == {1}
    assert r["img"].dtype == dtype and r["img"].shape == (1, 1, 33, 33, 4)
    # a coplanar tie goes to the lower face index, wherever both cover
    t = both("tie_32")[k]
    c = CASES["tie_32"]
    for face, other in ((0, 1), (1, 0)):
        alone = mf.restate(dict(c, faces=c["faces"][face:face + 1]), dtype, mr.mesh_camera, mr.mesh_affine)["ids"] >= 0
        rest = mf.restate(dict(c, faces=c["faces"][other:other + 1]), dtype, mr.mesh_camera, mr.mesh_affine)["ids"] >= 0
        assert (alone & rest).sum() > 50
        assert (t["ids"][alone & rest] == 0).all() and (t["ids"][alone & ~rest] == face).all()
    # a triangle with a vertex at w <= 0 is not drawn; the other one is
    b = both("behind_32")[k]
    assert set(np.unique(b["ids"])) == {-1, 0}                # faces reversed: face 0 is (0, 2, 3), face 1 names the vertex behind
    # a zero-area face draws nothing
    z = both("zero_area_32")[k]
    assert set(np.unique(z["ids"])) == {-1, 0, 1}
    # samples = 2 equals the mean of the four sub-sample images, summed in order and divided last
    c = CASES["b1_t2_37x29"]
    r = mf.restate(c, dtype, mr.mesh_camera, mr.mesh_affine, parts=True)
    sub = r["sub"]
    mean = np.clip((((sub[:, :, 0] + sub[:, :, 1]) + sub[:, :, 2]) + sub[:, :, 3]) / dtype(4), 0, 1)
    assert np.array_equal(mean, r["img"]) and sub.shape[2] == 4
    # ... and each sub-sample image is the samples = 1 image of a camera shifted to that sub-sample: the top-left one here
    P, A = mf.case_camera(c, mr.mesh_camera, mr.mesh_affine)
    A0 = A.copy()
    A0[:, 2] += (0.25, -0.25)
    one = mf.render(c["verts"], c["faces"], dtype=np.float64, proj=P, affine=A0, W=37, H=29, samples=1)
    if dtype is np.float64:
        assert np.array_equal(one["ids"][:, :, 0], r["ids"][:, :, 0])
    # background where nothing covers, the frame's colour times the shade where something does; dead frames are zeros
    bg = np.asarray(mf.BG, dtype)
    assert np.array_equal(r["img"][0, 0, 0, 0], bg)
    d = both("b3_t9")[k]
    assert not d["img"][1, 4:].any() and not d["img"][2, 1:].any() and d["img"][1, :4].any() and (d["ids"][2, 1:] == -1).all()
    inside = d["ids"][0, 0].min(0) >= 0
    assert inside.sum() > 100 and np.allclose(d["img"][0, 0][inside][:, 3], 0.9 + 0.1 * 0.8)
    # a sub-range equals the slice
    c3 = CASES["b3_t9"]
    assert np.array_equal(mf.restate(c3, dtype, mr.mesh_camera, mr.mesh_affine, frames=(2, 5))["img"], d["img"][:, 2:5])


@pytest.mark.parametrize("name", sorted(CASES))
def test_float32_restatement_keeps_the_flip_cap(name):
    """The condition of the GPU test: winners flip between float32 and float64 on at most 1 % of the covered pixels (none in the
    strict cases), and off those pixels float32 is close to float64."""
    f32, f64 = both(name)
    agree, flips = mf.agreement(f32["ids"], f64["ids"], f64["covered"])
    own = mf.distance(f32["img"], f64["img"], agree)
    worst = int(np.abs(mf.quantise(f32["img"]).astype(int) - mf.quantise(f64["img"]).astype(int))[agree].max())
    print(f"{name}: covered {int(f64['covered'].sum())}, flips {flips:.4%}, f32 vs f64 on agreeing pixels {own:.3e}, levels {worst}")
    assert f64["covered"].sum() > 0
    assert flips <= (0.0 if CASES[name].get("strict") else mf.FLIP_CAP)
    assert own < 1e-4 and worst <= 1


def test_cases_are_what_they_claim():
    chunk = mr.limits()["chunk"]
    assert len(CASES["chunk_plus_1"]["faces"]) == chunk + 1 and len(CASES["two_chunks"]["faces"]) == 2 * chunk
    assert CASES["chunk_plus_1"]["verts"].shape[2] % 64 != 0
    assert [len(mf.icosphere(k)[0]) for k in (1, 2)] == [42, 162] and len(mf.icosphere(2)[1]) == 320
    assert CASES["b33_t9_37x29"]["verts"].shape[:2] == (33, 9) and CASES["b3_t9"]["lengths"] == [9, 4, 1]
    assert {CASES[f"ico_96_s{s}"]["samples"] for s in (1, 2, 3)} == {1, 2, 3}
    v, f = mf.icosphere(1)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert ((n * v[f].mean(1)).sum(1) > 0).all()             # wound outwards
