"""SMPL meshes to video frames on the GPU: the drawing half of the reference's visualize/render_final.py (`render`, :79-89 and
:169-251).  The reference hands every frame to pyrender (OSMesa / EGL) and reads a 960 x 960 RGBA image back; here a batch of posed
meshes becomes [B, T, H, W, 4] uint8 frames on the device in three launches (csrc/mst_mesh.h) with no GL context, `pyrender`,
`trimesh`, `shapely` or `imageio`.

  MeshTopology             faces and the vertex -> faces adjacency (CSR), built once per face array; `SMPLBody.topology`
  mesh_camera              the reference's camera in closed form: pose (:234-241) and glTF's infinite perspective
  weak_perspective_camera  the matrix of the reference's `WeakPerspectiveCamera` (:21-43)
  render_meshes            vertices -> frames (and the float image / the face-index image when asked)
  save_mesh_frames,        .npy, .png, .gif through PIL, .mp4 through an `ffmpeg` on PATH (utils/plot_script.py's writers)
  render_meshes_to_file

The camera is computed on the HOST in float64 from `k_mesh_bounds`' output (one small copy and one synchronisation a call when
`camera=None`) and handed down as float32 matrices, one a clip.

The silhouette and the camera are the reference's; the colours inside the silhouette are not.  Stated deviations:
  * shading is Lambert plus ambient, s = ambient + (1 - ambient) max(0, n . l) on smooth vertex normals, not pyrender's
    metallic-roughness BRDF (metallicFactor 0.5) under three lights of intensity 300;
  * only the nearest surface is blended over the background (pyrender's BLEND mode also blends the surfaces behind it);
  * there is no near-plane clipping: a face with a vertex at w <= 0 is dropped whole;
  * anti-aliasing is this package's sample grid (`samples` x `samples` points a pixel), not a GL multisample pattern.
The drawing rules are stated in full in include/mst_engine.h and restated in numpy in tests/mesh_fixture.py.

Nothing here has a CPU path; the topology, the cameras, the colour ramp, the chunk planner and every argument check need no GPU."""
import ctypes as C
import math

import numpy as np
import torch

from .. import _native as N
from ..utils import plot_script as ps

_NO_CPU = "{} runs on the GPU only (no CPU fallback); move the vertices to cuda"
DEFAULT_BG = (1.0, 1.0, 1.0, 0.8)                # render_final.py:169
DEFAULT_AMBIENT = 0.4                            # :197
DEFAULT_LIGHT = (0.0, 0.0, 1.0)                  # :221-229: three lights posed by translation only shine along -z
DEFAULT_BUDGET = 4 << 30


def limits():
    lib = N.lib()
    return {"vertices": lib.mst_mesh_max_vertices(), "faces": lib.mst_mesh_max_faces(), "side": lib.mst_mesh_max_side(),
            "samples": lib.mst_mesh_max_samples(), "chunk": lib.mst_mesh_chunk()}


# ------------------------------------------------------------------------------------------ topology
class MeshTopology:
    """faces [F, 3] (0-based) and the adjacency the normals are summed in: `adj_offsets` [V + 1], `adj_faces` [3 F] -- the faces naming
    vertex v in ascending order, a face once for each time it names v.  Host arrays are kept (the C ABI checks them on every call);
    device copies are made once per device."""

    def __init__(self, faces, num_vertices=None):
        f = np.asarray(faces.detach().cpu() if torch.is_tensor(faces) else faces)
        if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1 or not np.issubdtype(f.dtype, np.integer):
            raise ValueError(f"MeshTopology: faces of shape {f.shape} and type {f.dtype}, expected integers [F >= 1, 3]")
        V = int(f.max()) + 1 if num_vertices is None else int(num_vertices)
        if f.min() < 0 or f.max() >= V:
            raise ValueError(f"MeshTopology: faces name vertex {int(f.min() if f.min() < 0 else f.max())}, outside 0..{V - 1}")
        self.faces = np.ascontiguousarray(f, dtype=np.int32)
        self.num_faces, self.num_vertices = int(f.shape[0]), V
        flat = self.faces.reshape(-1)
        order = np.argsort(flat, kind="stable")              # by vertex, then by position: ascending face index within a vertex
        self.adj_faces = np.ascontiguousarray(order // 3, dtype=np.int32)
        self.adj_offsets = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=V))]).astype(np.int32)
        self._dev = {}

    def on(self, device):
        """-> (faces, adj_offsets, adj_faces) int32 tensors on `device`."""
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(a).to(device) for a in (self.faces, self.adj_offsets, self.adj_faces))
            torch.cuda.current_stream(device).synchronize()  # once: any stream may read them afterwards
        return self._dev[key]


def _topology(what, faces, V):
    topo = faces if isinstance(faces, MeshTopology) else getattr(faces, "topology", None)
    if topo is None:
        topo = MeshTopology(faces, V)
    if topo.num_vertices != V:
        if topo.faces.max() >= V:
            raise ValueError(f"{what}: faces name vertex {int(topo.faces.max())}, the mesh has {V}")
        topo = MeshTopology(topo.faces, V)
    return topo


# ------------------------------------------------------------------------------------------ cameras
def mesh_affine(width, height):
    """Normalised device coordinates -> pixels, y up: x = (ndc_x + 1) W / 2, y = (ndc_y + 1) H / 2."""
    return np.array([[width / 2.0, 0.0, width / 2.0], [0.0, height / 2.0, height / 2.0]])


def mesh_camera(bounds, yfov=math.pi / 3.0, znear=0.05, aspect=1.0):
    """bounds [..., 6 or 8] (MINS xyz, MAXS xyz: `k_mesh_bounds`' rows) -> proj [..., 4, 4] float64, rows x, y, depth, w: the
    reference's camera.  Pose (:234-241): a rotation about x by -pi / 6 placed at ((minx + maxx) / 2, 1.5, max(4, minz + (1.5 -
    MINS[1]) * 2, maxx - minx)) with minx, maxx, minz padded by 0.5 (:86-89); projection: glTF's infinite perspective matrix, which
    pyrender's PerspectiveCamera(yfov) gives when zfar is None (znear 0.05 is its default).  Depth is NDC z: -1 at znear, towards 1
    far away; smaller is nearer.  Computed on the host in float64."""
    b = np.asarray(bounds, np.float64)
    if b.shape[-1] not in (6, 8):
        raise ValueError(f"mesh_camera: bounds of shape {b.shape}, expected [..., 6] or [..., 8]")
    if not (0 < yfov < math.pi and znear > 0 and aspect > 0):
        raise ValueError("mesh_camera: 0 < yfov < pi, znear > 0, aspect > 0")
    minx, maxx, minz = b[..., 0] - 0.5, b[..., 3] + 0.5, b[..., 2] - 0.5
    cx, cy = (minx + maxx) / 2.0, 1.5
    cz = np.maximum(np.maximum(4.0, minz + (1.5 - b[..., 1]) * 2.0), maxx - minx)
    c, s = math.cos(-math.pi / 6.0), math.sin(-math.pi / 6.0)
    t = math.tan(yfov / 2.0)
    out = np.zeros(b.shape[:-1] + (4, 4))
    # view = R^T (p - centre), R = [[1, 0, 0], [0, c, -s], [0, s, c]]
    vy = np.stack([np.zeros_like(cx), np.full_like(cx, c), np.full_like(cx, s), -(c * cy + s * cz)], -1)
    vz = np.stack([np.zeros_like(cx), np.full_like(cx, -s), np.full_like(cx, c), -(-s * cy + c * cz)], -1)
    out[..., 0, 0] = 1.0 / (aspect * t)
    out[..., 0, 3] = -cx / (aspect * t)
    out[..., 1, :] = vy / t
    out[..., 2, :] = -vz
    out[..., 2, 3] += -2.0 * znear
    out[..., 3, :] = -vz
    return out


def weak_perspective_camera(scale, translation):
    """The matrix `WeakPerspectiveCamera(scale, translation).get_projection_matrix()` returns (:36-43): rows x, y, depth, w."""
    P = np.eye(4)
    P[0, 0], P[1, 1] = scale[0], scale[1]
    P[0, 3], P[1, 3] = translation[0] * scale[0], -translation[1] * scale[1]
    P[2, 2] = -1
    return P


def default_colors(frames):
    """The reference's colour of frame n (:184), [255, 145 + 0.8 n, 33 + 0.5 n] / 255 with alpha 0.9 -> [frames, 4] float64, each
    channel clamped to 1 (green passes 255 at n = 138; GL clamps it on output)."""
    n = np.arange(int(frames), dtype=np.float64)
    return np.stack([np.ones_like(n), np.minimum((145 + 0.8 * n) / 255.0, 1.0), np.minimum((33 + 0.5 * n) / 255.0, 1.0), np.full_like(n, 0.9)], 1)


# ------------------------------------------------------------------------------------------ planning
def frame_bytes(batch, vertices, height, width, return_float=False, return_ids=False):
    """Bytes one output frame of every clip needs: workspace, image, and the float and face-index images when asked."""
    ws = (5 * vertices + 4 * ((vertices + 255) // 256)) * 4
    return batch * (ws + height * width * (4 + (16 if return_float else 0) + (4 if return_ids else 0)))


def plan_frame_chunks(t0, t1, per_frame_bytes, budget=DEFAULT_BUDGET):
    """[t0, t1) cut into runs of at most max(1, budget // per_frame_bytes) frames -> [(s, e), ...]."""
    if not (t0 < t1 and per_frame_bytes > 0 and budget > 0):
        raise ValueError("plan_frame_chunks: t0 < t1, positive sizes")
    n = max(1, int(budget) // int(per_frame_bytes))
    return [(s, min(s + n, t1)) for s in range(t0, t1, n)]


# ------------------------------------------------------------------------------------------ the renderer
def render_meshes(vertices, faces_or_topology, lengths=None, *, width=960, height=960, samples=2, camera=None, colors=None,
                  bg=DEFAULT_BG, light=DEFAULT_LIGHT, ambient=DEFAULT_AMBIENT, frames=None, layout="reference", out=None,
                  return_float=False, return_ids=False, ids_sample=0, stream=None, budget=DEFAULT_BUDGET):
    """vertices [B, V, 3, T] (layout='reference', as `Rotation2xyz` writes them) or [B, T, V, 3] (layout='frames') on a CUDA device,
    read where they lie -> frames uint8 [B, t1 - t0, H, W, 4] on the same device; with return_float / return_ids a tuple with the
    float32 image before quantisation and / or the int32 image of the winning face at sub-sample `ids_sample` (-1: none).

    faces_or_topology: a `MeshTopology`, an object with `.topology` (an `SMPLBody`), or faces [F, 3].  lengths [B]: a clip's own
    frames, 1 <= len <= T; frames at and behind it are exact zeros.  camera: None -- `mesh_camera` of every clip's own bounds with
    `mesh_affine(width, height)` -- or (proj [4, 4] or [B, 4, 4], affine [2, 3]).  colors: [T, 4] or [B, T, 4] RGBA floats per frame
    instead of the reference's ramp.  light: the direction towards the light, normalised here.  frames=(t0, t1) renders only those
    frames, bit-equal to the same frames of a full render.  The frame range is cut into chunks so that workspace plus the chunk's
    outputs stay under `budget` bytes; chunking changes no bit.  stream: a torch.cuda.Stream instead of the current one."""
    what = "render_meshes"
    if not torch.is_tensor(vertices):
        raise TypeError(f"{what}: vertices is a tensor")
    if layout not in ("reference", "frames"):
        raise ValueError(f"{what}: layout {layout!r} is neither 'reference' ([B, V, 3, T]) nor 'frames' ([B, T, V, 3])")
    axis = 2 if layout == "reference" else 3
    if vertices.dim() != 4 or vertices.shape[axis] != 3:
        raise ValueError(f"{what}: vertices of shape {tuple(vertices.shape)}, expected {'[B, V, 3, T]' if layout == 'reference' else '[B, T, V, 3]'}")
    B, T, V = (vertices.shape[0], vertices.shape[3], vertices.shape[1]) if layout == "reference" else tuple(vertices.shape[:3])
    if B < 1 or T < 1 or V < 1:
        raise ValueError(f"{what}: {B} clips of {T} frames and {V} vertices")
    W, H, S = int(width), int(height), int(samples)
    if not (16 <= H <= 1024 and 16 <= W <= 1024):
        raise ValueError(f"{what}: image {H} x {W}: each side 16..1024")
    if not 1 <= S <= 4:
        raise ValueError(f"{what}: samples {S} outside 1..4")
    if not 0 <= int(ids_sample) < S * S:
        raise ValueError(f"{what}: ids_sample {ids_sample} outside 0..{S * S - 1}")
    t0, t1 = (0, T) if frames is None else (int(frames[0]), int(frames[1]))
    if not 0 <= t0 < t1 <= T:
        raise ValueError(f"{what}: frames ({t0}, {t1}) is not 0 <= t0 < t1 <= {T}")
    host_len = None
    if lengths is not None:
        host_len = (lengths.detach().cpu().numpy() if torch.is_tensor(lengths) else np.asarray(lengths)).reshape(-1).astype(np.int64)
        if host_len.shape[0] != B or host_len.min() < 1 or host_len.max() > T:
            raise ValueError(f"{what}: lengths {host_len.tolist()[:8]} for {B} clips of {T} frames (1 <= len <= T)")
    topo = _topology(what, faces_or_topology, V)
    li = np.asarray(light, np.float64).reshape(-1)
    if li.shape[0] != 3 or not np.isfinite(li).all() or not np.linalg.norm(li) > 0:
        raise ValueError(f"{what}: light is a finite direction of 3 values, not zero")
    li = li / np.linalg.norm(li)
    bgc = np.asarray(bg, np.float64).reshape(-1)
    if bgc.shape[0] != 4 or not np.isfinite(bgc).all() or not math.isfinite(ambient):
        raise ValueError(f"{what}: bg is 4 finite values (RGBA) and ambient finite")
    col = None
    if colors is not None:
        col = np.asarray(colors.detach().cpu() if torch.is_tensor(colors) else colors, np.float32)
        if col.shape not in ((T, 4), (B, T, 4)) or not np.isfinite(col).all():
            raise ValueError(f"{what}: colors of shape {col.shape}, expected finite [{T}, 4] or [{B}, {T}, 4]")
        col = np.ascontiguousarray(np.broadcast_to(col, (B, T, 4)), dtype=np.float32)
    affine = mesh_affine(W, H)
    proj = None
    if camera is not None:
        proj, affine = np.asarray(camera[0], np.float64), np.asarray(camera[1], np.float64)
        if proj.shape not in ((4, 4), (B, 4, 4)) or affine.shape != (2, 3) or not (np.isfinite(proj).all() and np.isfinite(affine).all()):
            raise ValueError(f"{what}: camera is finite (proj [4, 4] or [{B}, 4, 4], affine [2, 3]); got {proj.shape} and {affine.shape}")
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != (B, t1 - t0, H, W, 4)
                            or not out.is_contiguous()):
        raise ValueError(f"{what}: out is a contiguous uint8 tensor [{B}, {t1 - t0}, {H}, {W}, 4]")
    if not vertices.is_cuda or (out is not None and out.device != vertices.device):
        raise RuntimeError(_NO_CPU.format(what))
    lim = limits()
    if V > lim["vertices"] or topo.num_faces > lim["faces"] or T > 65535 or B > 65535:
        raise RuntimeError(f"{what}: {V} vertices, {topo.num_faces} faces; the kernels take {lim['vertices']} and {lim['faces']} (65535 clips and frames)")
    dev = vertices.device
    f_dev, off_dev, adj_dev = topo.on(dev)
    ld = None if host_len is None else torch.from_numpy(host_len.astype(np.int32)).to(dev)
    col_dev = None if col is None else torch.from_numpy(col).to(dev)
    src = vertices.detach()
    if src.dtype != torch.float32 or any(s < 1 and n > 1 for s, n in zip(src.stride(), src.shape)):
        src = src.float().contiguous()                       # on the caller's current stream, where the vertices were made
    st = tuple(max(s, 1) for s in src.stride())              # a dimension of one element is never stepped over: any stride serves
    sB, sT, sV, sC = (st[0], st[3], st[1], st[2]) if layout == "reference" else st
    scene = N.MstMeshScene(src.data_ptr(), sB, sT, sV, sC, None if ld is None else ld.data_ptr(), B, T, V, topo.num_faces,
                           topo.faces.ctypes.data, f_dev.data_ptr(), topo.adj_offsets.ctypes.data, off_dev.data_ptr(),
                           topo.adj_faces.ctypes.data, adj_dev.data_ptr())
    lib = N.lib()
    cur = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.device(dev), torch.cuda.stream(cur):
        sp = C.c_void_p(cur.cuda_stream)
        if proj is None:
            bounds = torch.empty(B, 8, dtype=torch.float32, device=dev)
            N.check(lib.mst_mesh_bounds(C.byref(scene), N.ptr(bounds), sp))
            proj = mesh_camera(bounds.cpu().numpy(), aspect=W / H)           # synchronises: the camera is formed on the host
        proj32 = np.ascontiguousarray(proj.reshape(-1, 16), dtype=np.float32)
        proj32[~np.isfinite(proj32).all(1)] = 0.0            # a clip with no finite vertex has no camera: w = 0 draws nothing
        proj_dev = torch.from_numpy(proj32).to(dev)
        view = N.MstMeshView()
        view.proj_host, view.proj_dev, view.proj_batch = proj32.ctypes.data, proj_dev.data_ptr(), proj32.shape[0]
        view.affine = (C.c_float * 6)(*[float(x) for x in affine.reshape(-1)])
        view.width, view.height, view.samples = W, H, S
        view.light = (C.c_float * 3)(*[float(x) for x in li])
        view.ambient = float(ambient)
        view.colors_dev = None if col_dev is None else col_dev.data_ptr()
        view.background = (C.c_float * 4)(*[float(x) for x in bgc])
        view.ids_sample = int(ids_sample)
        n_out = t1 - t0
        res = out if out is not None else torch.empty(B, n_out, H, W, 4, dtype=torch.uint8, device=dev)
        resf = torch.empty(B, n_out, H, W, 4, dtype=torch.float32, device=dev) if return_float else None
        resi = torch.empty(B, n_out, H, W, dtype=torch.int32, device=dev) if return_ids else None
        plan = plan_frame_chunks(t0, t1, frame_bytes(B, V, H, W, return_float, return_ids), budget)
        ws = torch.empty(int(lib.mst_mesh_workspace_bytes(B, plan[0][1] - plan[0][0], V)) // 4, dtype=torch.float32, device=dev)
        for s, e in plan:
            view.t0, view.t1 = s, e
            whole = len(plan) == 1
            direct = whole or B == 1                                         # one clip: a chunk is a contiguous slice of the result
            if direct:
                parts = [None if r is None else (r if whole else r[:, s - t0:e - t0]) for r in (res, resf, resi)]
            else:
                parts = [None if r is None else torch.empty((B, e - s) + tuple(r.shape[2:]), dtype=r.dtype, device=dev) for r in (res, resf, resi)]
            nbytes = int(lib.mst_mesh_workspace_bytes(B, e - s, V))
            N.check(lib.mst_mesh_vertices(C.byref(scene), C.byref(view), N.ptr(ws), nbytes, sp))
            N.check(lib.mst_mesh_frames(C.byref(scene), C.byref(view), N.ptr(ws), nbytes, N.ptr(parts[0]), N.ptr(parts[1]), N.ptr(parts[2]), sp))
            if not direct:
                for r, part in zip((res, resf, resi), parts):
                    if r is not None:
                        r[:, s - t0:e - t0].copy_(part)
    extra = tuple(r for r in (resf, resi) if r is not None)
    return (res,) + extra if extra else res


# ------------------------------------------------------------------------------------------ files
def save_mesh_frames(path, frames, fps=20, chunk=32):
    """frames uint8 [T, H, W, 4] -> a file chosen by the extension, through `plot_script.save_frames`: .npy and .png (numbered files)
    keep the alpha channel; .gif and .mp4 have none to speak of, so the colours are written as they are, without it."""
    return ps.save_frames(path, frames, fps, chunk)


def render_meshes_to_file(path, vertices, faces_or_topology, fps=20, chunk=32, **kw):
    """One clip rendered `chunk` frames at a time through `frames=` and handed to the writer piece by piece.  kw: `render_meshes`'."""
    if not torch.is_tensor(vertices) or vertices.dim() != 4 or vertices.shape[0] != 1:
        raise ValueError("render_meshes_to_file: vertices is one clip, a tensor [1, V, 3, T] or [1, T, V, 3]")
    if "frames" in kw or kw.get("return_float") or kw.get("return_ids") or kw.get("out") is not None:
        raise ValueError("render_meshes_to_file: frames=, out=, return_float= and return_ids= are not taken")
    T = vertices.shape[1] if kw.get("layout", "reference") == "frames" else vertices.shape[3]
    if kw.get("lengths") is not None:
        T = int(np.asarray(kw["lengths"].cpu() if torch.is_tensor(kw["lengths"]) else kw["lengths"]).reshape(-1)[0])
    if kw.get("camera") is None:                             # the clip's own camera, not a chunk's: formed once
        kw = dict(kw, camera=(_clip_camera(vertices, kw), mesh_affine(kw.get("width", 960), kw.get("height", 960))))
    pieces = (render_meshes(vertices, faces_or_topology, frames=(s, min(s + chunk, T)), **kw)[0] for s in range(0, T, chunk))
    return ps.save_frames(path, pieces, fps, chunk)


def _clip_camera(vertices, kw):
    layout = kw.get("layout", "reference")
    v = vertices.detach().float()
    v = v.permute(0, 3, 1, 2) if layout == "reference" else v                # [1, T, V, 3]
    if kw.get("lengths") is not None:
        v = v[:, :int(np.asarray(kw["lengths"].cpu() if torch.is_tensor(kw["lengths"]) else kw["lengths"]).reshape(-1)[0])]
    b = torch.empty(1, 8, dtype=torch.float32, device=vertices.device)
    if any(s < 1 and n > 1 for s, n in zip(v.stride(), v.shape)):
        v = v.contiguous()
    st = tuple(max(s, 1) for s in v.stride())
    scene = N.MstMeshScene(v.data_ptr(), st[0], st[1], st[2], st[3], None, 1, v.shape[1], v.shape[2], 0, None, None, None, None, None, None)
    with torch.cuda.device(vertices.device):
        N.check(N.lib().mst_mesh_bounds(C.byref(scene), N.ptr(b), N.stream_ptr(vertices.device)))
    return mesh_camera(b.cpu().numpy()[0], aspect=kw.get("width", 960) / kw.get("height", 960))
