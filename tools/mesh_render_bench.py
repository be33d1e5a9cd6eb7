"""Rendering meshes to frames: what `render_meshes` costs on a body of SMPL's size, 6890 vertices and 13 776 faces.

The body is SYNTHETIC (no SMPL file is bundled): a closed latitude-longitude surface of 84 rings x 82 columns plus two poles, which
has exactly SMPL's vertex and face counts, shaped as an ellipsoid 1.7 high that turns and walks across the clip.

  shapes      8 clips x 196 frames at 960 x 960 (the reference's image), 64 x 196 at 256 x 256, 8 x 4096 at 256 x 256
  samples     1 and 2 a side
  stages      k_mesh_bounds, k_mesh_vertices, k_mesh_frames each on its own through the C ABI, over the whole frame range, and
              `render_meshes` as a user calls it (bounds, the camera on the host, frame chunks under the default 4 GiB budget)
  fill        torch's fill kernel over the same uint8 output, in the same run: the HBM write floor for those bytes

Every entry is called once untimed, then `--reps` (5) rounds of all entries of a shape in turn, each event-timed around a synchronised
call; medians, in ms.  Prints one JSON line.  pyrender itself is not measured: it does not run without a GL stack."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_body(rings=84, cols=82):
    import numpy as np
    th = np.pi * (np.arange(rings) + 1) / (rings + 1)
    ph = 2 * np.pi * np.arange(cols) / cols
    x = 0.25 * np.sin(th)[:, None] * np.cos(ph)[None]
    z = 0.15 * np.sin(th)[:, None] * np.sin(ph)[None]
    y = 0.85 + 0.85 * np.cos(th)[:, None] * np.ones_like(ph)[None]
    v = np.concatenate([[[0, 1.7, 0]], np.stack([x, y, z], -1).reshape(-1, 3), [[0, 0, 0]]]).astype(np.float32)
    f = []
    for c in range(cols):
        f.append((0, 1 + (c + 1) % cols, 1 + c))
        f.append((len(v) - 1, 1 + (rings - 1) * cols + c, 1 + (rings - 1) * cols + (c + 1) % cols))
    for r in range(rings - 1):
        for c in range(cols):
            a, b = 1 + r * cols + c, 1 + r * cols + (c + 1) % cols
            f += [(a, b, a + cols), (b, b + cols, a + cols)]
    return v, np.array(f, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="8x196x960,64x196x256,8x4096x256")
    ap.add_argument("--samples", default="1,2")
    args = ap.parse_args()
    import numpy as np
    import torch
    import mst_amd  # noqa: F401
    from mst_amd import _native as N
    from mst_amd.visualize import mesh_render as mr

    dev = torch.device("cuda:0")
    v, f = synthetic_body()
    topo = mr.MeshTopology(f, len(v))
    f_dev, off_dev, adj_dev = topo.on(dev)
    lib = N.lib()
    out = {"vertices": len(v), "faces": len(f), "body": "synthetic", "reps": args.reps, "tile": 32, "chunk": mr.limits()["chunk"], "runs": []}

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
        return {k: round(statistics.median(x), 3) for k, x in ms.items()}

    for shape in args.shapes.split(","):
        B, T, side = (int(x) for x in shape.split("x"))
        base = torch.from_numpy(v).to(dev)
        t = torch.arange(T, device=dev, dtype=torch.float32)
        ang = 0.05 * t[None, :] + torch.arange(B, device=dev, dtype=torch.float32)[:, None]
        cs, sn = torch.cos(ang)[..., None], torch.sin(ang)[..., None]
        verts = torch.stack([cs * base[:, 0] + sn * base[:, 2] + (0.004 * t)[None, :, None], base[:, 1].expand(B, T, -1),
                             -sn * base[:, 0] + cs * base[:, 2] + (0.002 * t)[None, :, None]], -1).contiguous()    # [B, T, V, 3]
        del cs, sn, ang
        st = verts.stride()
        scene = N.MstMeshScene(verts.data_ptr(), st[0], st[1], st[2], st[3], None, B, T, len(v), len(f), topo.faces.ctypes.data,
                               f_dev.data_ptr(), topo.adj_offsets.ctypes.data, off_dev.data_ptr(), topo.adj_faces.ctypes.data, adj_dev.data_ptr())
        bounds = torch.empty(B, 8, dtype=torch.float32, device=dev)
        sp = N.stream_ptr(dev)
        N.check(lib.mst_mesh_bounds(C.byref(scene), N.ptr(bounds), sp))
        proj32 = np.ascontiguousarray(mr.mesh_camera(bounds.cpu().numpy()).reshape(-1, 16), dtype=np.float32)
        proj_dev = torch.from_numpy(proj32).to(dev)
        nbytes = int(lib.mst_mesh_workspace_bytes(B, T, len(v)))
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        img = torch.empty(B, T, side, side, 4, dtype=torch.uint8, device=dev)
        for S in (int(x) for x in args.samples.split(",")):
            view = N.MstMeshView()
            view.proj_host, view.proj_dev, view.proj_batch = proj32.ctypes.data, proj_dev.data_ptr(), B
            view.affine = (C.c_float * 6)(*[float(x) for x in mr.mesh_affine(side, side).reshape(-1)])
            view.width, view.height, view.samples = side, side, S
            view.light = (C.c_float * 3)(*mr.DEFAULT_LIGHT)
            view.ambient = mr.DEFAULT_AMBIENT
            view.background = (C.c_float * 4)(*mr.DEFAULT_BG)
            view.t0, view.t1 = 0, T
            r = timed({
                "bounds_ms": lambda: N.check(lib.mst_mesh_bounds(C.byref(scene), N.ptr(bounds), sp)),
                "vertices_ms": lambda: N.check(lib.mst_mesh_vertices(C.byref(scene), C.byref(view), N.ptr(ws), nbytes, sp)),
                "frames_ms": lambda: N.check(lib.mst_mesh_frames(C.byref(scene), C.byref(view), N.ptr(ws), nbytes, N.ptr(img), None, None, sp)),
                "render_meshes_ms": lambda: mr.render_meshes(verts, topo, width=side, height=side, samples=S, layout="frames", out=img),
                "fill_ms": lambda: img.fill_(7),
            })
            N.check(lib.mst_mesh_frames(C.byref(scene), C.byref(view), N.ptr(ws), nbytes, N.ptr(img), None, None, sp))   # after the fill
            covered = float((img[0, T // 2, :, :, 3] != 204).float().mean())
            r.update(clips=B, frames=T, side=side, samples=S, output_bytes=img.numel(), workspace_bytes=nbytes,
                     frames_per_s=round(B * T / (r["render_meshes_ms"] * 1e-3)),
                     frames_kernel_GBps=round(img.numel() / (r["frames_ms"] * 1e-3) / 1e9, 1),
                     fill_GBps=round(img.numel() / (r["fill_ms"] * 1e-3) / 1e9, 1), body_share_of_mid_frame=round(covered, 4))
            out["runs"].append(r)
        del verts, ws, img
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
