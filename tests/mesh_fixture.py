"""numpy restatement of the image `render_meshes` draws (include/mst_engine.h, "Meshes to video frames"): the scene of the reference's
visualize/render_final.py `render` under this package's own drawing rules -- bounds, vertex normals, shade, projection, coverage,
winner, interpolation, compositing, supersampling, quantisation.

Nothing here imports the reference, pyrender or trimesh.  Every function takes a dtype and runs in it, operation by operation in the
order the header states, so one set of inputs is evaluated in float64 (the oracle) and in float32 (the arithmetic of the kernels).
Nothing is culled: the winner is a plain loop over the faces in ascending order, vectorised over the sample points only.  The camera
is an operand.  The meshes are synthetic: no SMPL file is needed."""
import numpy as np

FLOOR = 1e-6
FLIP_CAP = 0.01                                  # of the pixels any face covers
AMBIENT, LIGHT, BG, ALPHA = 0.4, (0.0, 0.0, 1.0), (1.0, 1.0, 1.0, 0.8), 0.9


def bar(own):
    """4 x the float32 restatement's own distance from float64, floor 1e-6."""
    return max(4.0 * float(own), FLOOR)


def distance(a, b, mask=None):
    """max |a - b| over the pixels of `mask` [..., H, W] (images [..., H, W, 4] live in [0, 1], so the distance is absolute)."""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    if mask is not None:
        d = d[mask]
    return float(d.max()) if d.size else 0.0


# ------------------------------------------------------------------------------------------ meshes
def triangle():
    return np.array([[-0.6, -0.5, 0.0], [0.7, -0.4, 0.1], [0.0, 0.65, -0.1]], np.float32), np.array([[0, 1, 2]], np.int32)


def quad():
    """Two triangles sharing the diagonal 0 - 2."""
    v = np.array([[-0.6, -0.6, 0.0], [0.6, -0.6, 0.2], [0.6, 0.6, 0.0], [-0.6, 0.6, -0.2]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def icosphere(level=1, radius=0.8):
    """An icosahedron subdivided `level` times: 12 / 42 / 162 vertices, 20 / 80 / 320 faces, wound outwards."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius).astype(np.float32), np.array(f, np.int32)


def blob(V, F, seed=3, radius=0.8):
    """A seeded soup: V points around a sphere, F faces over random triples (distinct vertices a face) -> overlapping slivers at every
    depth, V and F whatever the caller needs."""
    g = np.random.default_rng([seed, V, F])
    p = g.normal(size=(V, 3))
    p = p / np.linalg.norm(p, axis=1, keepdims=True) * g.uniform(0.5, 1.0, (V, 1)) * radius
    a = g.integers(0, V, F)
    b = (a + g.integers(1, V, F)) % V
    c = g.integers(0, V, F)
    bad = (c == a) | (c == b)
    while bad.any():
        c[bad] = g.integers(0, V, int(bad.sum()))
        bad = (c == a) | (c == b)
    return p.astype(np.float32), np.stack([a, b, c], 1).astype(np.int32)


def repeat_mesh(v, f, n, step=(0.05, 0.03, -0.2)):
    """n shifted copies of a mesh as one."""
    vs = np.concatenate([v + np.float32(k) * np.asarray(step, np.float32) for k in range(n)])
    fs = np.concatenate([f + k * len(v) for k in range(n)])
    return vs.astype(np.float32), fs.astype(np.int32)


def animate(v, B, T, seed=1):
    """[V, 3] -> [B, T, V, 3] float32: the mesh turning about y and drifting a little, another phase a clip."""
    g = np.random.default_rng([seed, B, T])
    out = np.zeros((B, T) + v.shape, np.float32)
    for b in range(B):
        ph, drift = g.uniform(0, 2 * np.pi), g.normal(0, 0.05, 3)
        for t in range(T):
            a = ph + 0.35 * t
            R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
            out[b, t] = (v.astype(np.float64) @ R.T + drift * t).astype(np.float32)
    return out


def flat_camera(W, H, scale=None):
    """x right, y up, the mesh's unit square over the smaller side, w = 1, depth = -z (nearer is larger z): (proj, affine)."""
    k = (min(W, H) / 2.0) if scale is None else scale
    P = np.diag([1.0, 1.0, -1.0, 1.0])
    return P, np.array([[k, 0.0, W / 2.0], [0.0, k, H / 2.0]])


def adjacency(faces, V):
    """The CSR the kernels read, brute force: for every vertex the faces naming it, ascending, once for each time it is named."""
    rows = [[] for _ in range(V)]
    for fi, f in enumerate(np.asarray(faces)):
        for v in f:
            rows[int(v)].append(fi)
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return off, np.array([x for r in rows for x in r], np.int32)


# ------------------------------------------------------------------------------------------ the image
def bounds(verts, lengths, dtype):
    """-> [B, 6]: MINS xyz, MAXS xyz over each clip's live frames (fmin / fmax pass over NaN)."""
    B, T = verts.shape[:2]
    out = np.zeros((B, 6), dtype)
    for b in range(B):
        n = T if lengths is None else int(lengths[b])
        v = verts[b, :n].astype(dtype).reshape(-1, 3)
        out[b, :3] = np.fmin.reduce(v, 0)
        out[b, 3:] = np.fmax.reduce(v, 0)
    return out


def default_colors(T, dtype):
    n = np.arange(T).astype(dtype)
    one = dtype(1)
    c = np.empty((T, 4), dtype)
    c[:, 0] = one
    c[:, 1] = np.fmin((dtype(145) + dtype(0.8) * n) / dtype(255), one)
    c[:, 2] = np.fmin((dtype(33) + dtype(0.5) * n) / dtype(255), one)
    c[:, 3] = dtype(ALPHA)
    return c


def vertex_stage(v, faces, M, A, light, ambient):
    """One frame's vertices [V, 3] (already in dtype) -> px, py, depth, 1 / w, shade, each [V]; NaN where the vertex is not drawn."""
    dtype = v.dtype.type
    V = len(v)
    n = np.zeros((V, 3), dtype)
    with np.errstate(all="ignore"):
        for f in faces:                                      # ascending face order: the adjacency's order at every vertex
            a = v[f[0]]
            u, w = v[f[1]] - a, v[f[2]] - a
            c = np.array([u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]], dtype)
            for k in f:                                      # a face naming a vertex twice adds twice (its cross product is zero)
                n[k] = n[k] + c
        l = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        good = (l > 0) & (l < np.inf)
        n = np.where(good[:, None], n / np.where(good, l, dtype(1))[:, None], dtype(0))
        d = (n[:, 0] * light[0] + n[:, 1] * light[1]) + n[:, 2] * light[2]
        shade = ambient + (dtype(1) - ambient) * np.fmax(d, dtype(0))
        x, y, z = v[:, 0], v[:, 1], v[:, 2]
        X = ((M[0, 0] * x + M[0, 1] * y) + M[0, 2] * z) + M[0, 3]
        Y = ((M[1, 0] * x + M[1, 1] * y) + M[1, 2] * z) + M[1, 3]
        Z = ((M[2, 0] * x + M[2, 1] * y) + M[2, 2] * z) + M[2, 3]
        Wc = ((M[3, 0] * x + M[3, 1] * y) + M[3, 2] * z) + M[3, 3]
        xn, yn, dep, iw = X / Wc, Y / Wc, Z / Wc, dtype(1) / Wc
        qx = (A[0, 0] * xn + A[0, 1] * yn) + A[0, 2]
        qy = (A[1, 0] * xn + A[1, 1] * yn) + A[1, 2]
        ok = (np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & np.isfinite(Wc) & (Wc > 0) & np.isfinite(qx) & np.isfinite(qy)
              & np.isfinite(dep) & np.isfinite(iw))
    nan = dtype(np.nan)
    return [np.where(ok, a, nan) for a in (qx, qy, dep, iw, shade)]


def _weights(x, y, SX, SY):
    """x, y: the pixels of L, M, H -> wl, wm, wh, sum and the coverage mask at the sample points."""
    qlx, qly, qmx, qmy = SX - x[0], SY - y[0], SX - x[1], SY - y[1]
    wh = (x[1] - x[0]) * qly - (y[1] - y[0]) * qlx
    wm = -((x[2] - x[0]) * qly - (y[2] - y[0]) * qlx)
    wl = (x[2] - x[1]) * qmy - (y[2] - y[1]) * qmx
    s = (wl + wm) + wh
    inbox = (SX >= min(x)) & (SX <= max(x)) & (SY >= min(y)) & (SY <= max(y))
    same = ((wl >= 0) & (wm >= 0) & (wh >= 0)) | ((wl <= 0) & (wm <= 0) & (wh <= 0))
    return wl, wm, wh, s, inbox & same & (s != 0)


def frame_stage(px, py, dep, iw, shade, faces, W, H, S, rgba, bg):
    """One frame -> (image [H, W, 4] before the clamp's quantisation, ids [S * S, H, W], covered [H, W]: any face covers any sample)."""
    dtype = px.dtype.type
    sub = (np.arange(S).astype(dtype) + dtype(0.5)) / dtype(S)
    # sample arrays [S (j), S (i), H, W]
    SX = (np.arange(W).astype(dtype)[None, None, None, :] + sub[None, :, None, None]) + np.zeros((S, 1, H, 1), dtype)
    SY = ((H - np.arange(H)).astype(dtype)[None, None, :, None] - sub[:, None, None, None]) + np.zeros((1, S, 1, W), dtype)
    best = np.full(SX.shape, np.inf, dtype)
    ids = np.full(SX.shape, -1, np.int32)
    num = np.zeros(SX.shape, dtype)
    with np.errstate(all="ignore"):
        for fi, f in enumerate(faces):
            o = np.sort(np.asarray(f))
            x, y = px[o], py[o]
            if not (np.isfinite(x).all()):
                continue
            area2 = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
            if not (area2 != 0 and np.isfinite(area2)):
                continue
            wl, wm, wh, s, cov = _weights(x, y, SX, SY)
            d = ((wl * dep[o[0]] + wm * dep[o[1]]) + wh * dep[o[2]]) / s
            win = cov & (d < best)                           # ascending faces: an exact tie stays with the lower index; NaN never wins
            al, am, ah = wl * iw[o[0]], wm * iw[o[1]], wh * iw[o[2]]
            sh = ((al * shade[o[0]] + am * shade[o[1]]) + ah * shade[o[2]]) / ((al + am) + ah)
            best = np.where(win, d, best)
            ids = np.where(win, np.int32(fi), ids)
            num = np.where(win, sh, num)
    a = rgba[3]
    om = dtype(1) - a
    hit = ids >= 0
    img = np.empty(SX.shape + (4,), dtype)
    with np.errstate(all="ignore"):
        for ch in range(3):
            img[..., ch] = np.where(hit, a * (rgba[ch] * num) + om * bg[ch], bg[ch])
        img[..., 3] = np.where(hit, a + om * bg[3], bg[3])
    flat = img.reshape((S * S,) + img.shape[2:])
    c = flat[0]
    for k in range(1, S * S):
        c = c + flat[k]
    c = np.fmin(np.fmax(c / dtype(S * S), dtype(0)), dtype(1))
    return c, ids.reshape(S * S, H, W), hit.any((0, 1)), flat


def render(verts, faces, lengths=None, *, dtype, proj, affine, W, H, samples=2, colors=None, bg=BG, light=LIGHT, ambient=AMBIENT,
           frames=None, parts=False):
    """verts [B, T, V, 3] -> dict: img [B, t1 - t0, H, W, 4] in `dtype`, ids int32 [B, t1 - t0, S * S, H, W] (-1: no face; dead
    frames -1), covered bool [B, t1 - t0, H, W].  proj [4, 4] or [B, 4, 4]; colors [B, T, 4] or None (the reference's ramp);
    frames (t0, t1).  parts=True adds sub [B, t1 - t0, S * S, H, W, 4]: the composited sub-sample images."""
    B, T, V = verts.shape[:3]
    t0, t1 = (0, T) if frames is None else frames
    P = np.asarray(proj, np.float64)
    P = np.broadcast_to(P, (B, 4, 4)).astype(dtype)
    A = np.asarray(affine).astype(dtype)
    li, am, bgc = np.asarray(light).astype(dtype), dtype(ambient), np.asarray(bg).astype(dtype)
    S = samples
    out = dict(img=np.zeros((B, t1 - t0, H, W, 4), dtype), ids=np.full((B, t1 - t0, S * S, H, W), -1, np.int32),
               covered=np.zeros((B, t1 - t0, H, W), bool))
    if parts:
        out["sub"] = np.zeros((B, t1 - t0, S * S, H, W, 4), dtype)
    ramp = default_colors(T, dtype)
    for b in range(B):
        n = T if lengths is None else int(lengths[b])
        for t in range(t0, min(t1, n)):
            rgba = ramp[t] if colors is None else np.asarray(colors)[b, t].astype(dtype)
            vs = vertex_stage(verts[b, t].astype(dtype), faces, P[b], A, li, am)
            c, ids, cov, flat = frame_stage(*vs, faces, W, H, S, rgba, bgc)
            out["img"][b, t - t0], out["ids"][b, t - t0], out["covered"][b, t - t0] = c, ids, cov
            if parts:
                out["sub"][b, t - t0] = flat
    return out


def quantise(f):
    """floor(255 f + 0.5) in the image's own type -> uint8."""
    t = f.dtype.type
    return np.floor(t(255) * f + t(0.5)).astype(np.uint8)


def agreement(ids_a, ids_b, covered):
    """-> (mask [..., H, W] of the pixels whose winners agree at every sub-sample given, flips / covered pixels).  ids [..., K, H, W]."""
    agree = (ids_a == ids_b).all(-3)
    n = int(covered.sum())
    return agree, (float((~agree).sum()) / n if n else 0.0)


# ------------------------------------------------------------------------------------------ the cases every test shares
def cases(chunk):
    """name -> dict(verts [B, T, V, 3], faces, size (H, W), samples, camera (proj, affine) or 'mesh', lengths, strict): the smallest
    shapes at which each mechanism can go wrong.  strict: no winner may flip between float32 and float64."""
    c = {}
    v, f = triangle()
    c["b1_t1_16"] = dict(verts=v[None, None], faces=f, size=(16, 16), samples=1, strict=True)
    v, f = quad()
    c["b1_t2_37x29"] = dict(verts=animate(v, 1, 2, 2), faces=f, size=(29, 37), samples=2)
    # two coplanar overlapping triangles at z = 0: every covered sample of the overlap is an exact tie
    v = np.array([[-0.7, -0.5, 0], [0.5, -0.5, 0], [-0.1, 0.6, 0], [-0.4, -0.6, 0], [0.75, -0.3, 0], [0.2, 0.5, 0]], np.float32)
    c["tie_32"] = dict(verts=v[None, None], faces=np.array([[3, 4, 5], [0, 1, 2]], np.int32), size=(32, 32), samples=2, strict=True)
    # two triangles sharing an edge that runs through pixel centres: the vertical x = 0 -> pixel x = 16.5 at 33 pixels
    v = np.array([[0, -0.5, 0], [0, 0.5, 0], [-0.5, 0, 0.1], [0.5, 0.125, -0.1]], np.float32)
    c["shared_edge_33"] = dict(verts=v[None, None], faces=np.array([[0, 1, 2], [1, 0, 3]], np.int32), size=(33, 33), samples=1,
                               camera=flat_camera(33, 33, 16.0))
    # one vertex behind the camera (w <= 0 there): the face is dropped whole, the other is drawn
    v, f = quad()
    P, A = flat_camera(32, 32)
    P = P.copy()
    P[3] = (0.0, 1.0, 0.0, 0.7)                              # w = y + 0.7: vertex 0 at y = -0.6 keeps w = 0.1, vertex 1, moved below, has w < 0
    vb = v.copy()
    vb[1, 1] = -0.9
    c["behind_32"] = dict(verts=vb[None, None], faces=f[::-1].copy(), size=(32, 32), samples=2, camera=(P, A))
    # a zero-area face (two equal vertices) among real ones
    v, f = quad()
    v = np.concatenate([v, v[1:2]])
    c["zero_area_32"] = dict(verts=v[None, None], faces=np.concatenate([f, [[1, 4, 2]], [[0, 0, 3]]]).astype(np.int32), size=(32, 32), samples=2)
    v, f = blob(131, chunk + 1)
    c["chunk_plus_1"] = dict(verts=v[None, None], faces=f, size=(37, 29), samples=1)
    iv, jf = icosphere(2)
    rv, rf_ = repeat_mesh(iv, jf, -(-2 * chunk // len(jf)))
    c["two_chunks"] = dict(verts=rv[None, None], faces=rf_[:2 * chunk].copy(), size=(37, 29), samples=1)
    for s in (1, 2, 3):
        c[f"ico_96_s{s}"] = dict(verts=iv[None, None], faces=jf, size=(96, 96), samples=s)
    iv1, jf1 = icosphere(1)
    c["b3_t9"] = dict(verts=animate(iv1, 3, 9, 4), faces=jf1, size=(48, 48), samples=2, lengths=[9, 4, 1])
    c["b33_t9_37x29"] = dict(verts=animate(iv1, 33, 9, 5), faces=jf1, size=(29, 37), samples=2, lengths=[9 - (b % 4) for b in range(33)])
    c["mesh_camera_300"] = dict(verts=animate(iv + np.float32([0.0, 0.9, 0.0]), 1, 2, 6), faces=jf, size=(300, 300), samples=2, camera="mesh")
    return c


def case_camera(c, mesh_camera, mesh_affine):
    """The (proj, affine) a case is seen through: its own, the package's `mesh_camera` of its float64 bounds, or `flat_camera`."""
    H, W = c["size"]
    cam = c.get("camera")
    if cam is None:
        return flat_camera(W, H)
    if isinstance(cam, str):
        return mesh_camera(bounds(c["verts"], c.get("lengths"), np.float64), aspect=W / H), mesh_affine(W, H)
    return cam


def restate(c, dtype, mesh_camera, mesh_affine, **kw):
    H, W = c["size"]
    P, A = case_camera(c, mesh_camera, mesh_affine)
    return render(c["verts"], c["faces"], c.get("lengths"), dtype=dtype, proj=P, affine=A, W=W, H=H, samples=c["samples"], **kw)
