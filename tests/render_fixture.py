"""numpy restatement of the image `render_motion` draws (include/mst_engine.h, "Clips to video frames"): the scene of the reference's
`explicit_plot_3d_motion` (data_loaders/humanml/utils/plot_script.py:168-311) under this package's own drawing rules.

Nothing here imports the reference or matplotlib.  Every function takes a dtype and runs in it, operation by operation in the order
the header states, so one set of inputs is evaluated in float64 (the oracle) and in float32 (the arithmetic of the kernel).  Nothing is
culled: a polyline's distance is a plain loop over its segments, vectorised over the pixels only.  The camera is an operand."""
import numpy as np

import ik_fixture as ikf

FLOOR = 1e-6
PALETTE_NAMES = ("blue", "orange", "purple", "upper_body")
_HEX = {"blue": ["#4D84AA", "#5B9965", "#61CEB9", "#34C1E2", "#80B79A"], "orange": ["#DD5A37", "#D69E00", "#B75A39", "#FF6D00", "#DDB50E"],
        "purple": ["#6B31DB", "#AD40A8", "#AF2B79", "#9B00FF", "#D836C1"]}
_HEX["upper_body"] = _HEX["blue"][:2] + _HEX["orange"][2:]
PALETTE = np.array([[[int(h[i:i + 2], 16) for i in (1, 3, 5)] for h in _HEX[n]] for n in PALETTE_NAMES], np.uint8)     # [4, 5, 3]
CHAINS_DRAWN = 5
ROOT_HORIZONTAL, ROOT, JOINT = 0, 1, 2


def bar(own):
    """4 x the float32 restatement's own distance from float64, floor 1e-6."""
    return max(4.0 * float(own), FLOOR)


def distance(a, b):
    """max |a - b|: images live in [0, 1], so the distance is absolute."""
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) if np.size(a) else 0.0


# ------------------------------------------------------------------------------------------ clips
def chains_of(J, seed=5):
    """The five chains of tests/ik_fixture.py's humanoid of J joints (J >= 19)."""
    return ikf.humanoid(seed, J)[0]


def walk(seed, B, T, J):
    """Seeded walks -> joints [B, T, J, 3] float32: a root that wanders over the ground at about 0.9 and the humanoid's bones hung off
    it with a little noise a frame."""
    g = np.random.default_rng([seed, B, T, J])
    _, parents, off = ikf.humanoid(5, J)
    rest = np.zeros((J, 3))
    for j in range(1, J):
        rest[j] = rest[parents[j]] + off[j] * 0.8
    step = g.normal(0.0, 0.04, (B, T, 3)) + np.array([0.03, 0.0, 0.02])
    step[..., 1] *= 0.2
    root = np.cumsum(step, 1) + np.array([0.0, 0.9, 0.0]) + g.normal(0.0, 0.3, (B, 1, 3)) * np.array([1.0, 0.1, 1.0])
    return (root[:, :, None] + rest + g.normal(0.0, 0.02, (B, T, J, 3))).astype(np.float32)


# ------------------------------------------------------------------------------------------ the image
def bounds(joints, lengths, scale, dtype, joints2=None):
    """-> [B, 6]: MINS xyz, MAXS xyz of scale * joints over each clip's live frames and both skeletons (fmin / fmax pass over NaN)."""
    B, T = joints.shape[:2]
    out = np.zeros((B, 6), dtype)
    for b in range(B):
        n = T if lengths is None else int(lengths[b])
        v = dtype(scale) * joints[b, :n].astype(dtype).reshape(-1, 3)
        if joints2 is not None:
            v = np.concatenate([v, dtype(scale) * joints2[b, :n].astype(dtype).reshape(-1, 3)])
        out[b, :3] = np.fmin.reduce(v, 0)
        out[b, 3:] = np.fmax.reduce(v, 0)
    return out


def project(x, y, z, M, A):
    """(x, y, z) arrays -> pixels; NaN where the point is not drawn."""
    with np.errstate(all="ignore"):
        X = ((M[0, 0] * x + M[0, 1] * y) + M[0, 2] * z) + M[0, 3]
        Y = ((M[1, 0] * x + M[1, 1] * y) + M[1, 2] * z) + M[1, 3]
        Wc = ((M[3, 0] * x + M[3, 1] * y) + M[3, 2] * z) + M[3, 3]
        xn, yn = X / Wc, Y / Wc
        qx = (A[0, 0] * xn + A[0, 1] * yn) + A[0, 2]
        qy = (A[1, 0] * xn + A[1, 1] * yn) + A[1, 2]
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & np.isfinite(Wc) & (Wc > 0) & np.isfinite(qx) & np.isfinite(qy)
    nan = np.asarray(np.nan, qx.dtype)
    return np.where(ok, qx, nan), np.where(ok, qy, nan)


def _blend(c, col, a):
    return c * (1 - a)[..., None] + col * a[..., None]


def _polyline_d2(px, py, CX, CY):
    dtype = CX.dtype.type
    d2 = np.full(np.broadcast(CX, CY).shape, np.inf, dtype)
    for s in range(len(px) - 1):
        ax, ay, bx, by = px[s], py[s], px[s + 1], py[s + 1]
        if not (np.isfinite(ax) and np.isfinite(bx)):
            continue
        dx, dy = bx - ax, by - ay
        l2 = dx * dx + dy * dy
        ex, ey = CX - ax, CY - ay
        with np.errstate(all="ignore"):
            u = np.clip((ex * dx + ey * dy) / l2, dtype(0), dtype(1)) if l2 > 0 else dtype(0)
            rx, ry = ex - u * dx, ey - u * dy
            d2 = np.fmin(d2, rx * rx + ry * ry)
    return d2


def _line_layer(c, d2, reach, col):
    cov = np.clip(reach - np.sqrt(d2), d2.dtype.type(0), d2.dtype.type(1))
    return _blend(c, col, cov)


def _quad_layer(c, qx, qy, CX, CY):
    dtype = CX.dtype.type
    area2 = dtype(0)
    for k in range(4):
        area2 = area2 + (qx[k] * qy[(k + 1) & 3] - qx[(k + 1) & 3] * qy[k])
    area = dtype(0.5) * area2
    if not abs(area) >= dtype(1e-12):
        return c
    sgn = dtype(1) if area > 0 else dtype(-1)
    dmin = np.full(np.broadcast(CX, CY).shape, np.inf, dtype)
    for k in range(4):
        ex, ey = qx[(k + 1) & 3] - qx[k], qy[(k + 1) & 3] - qy[k]
        el = np.sqrt(ex * ex + ey * ey)
        if el > 0:
            fx, fy = CX - qx[k], CY - qy[k]
            dmin = np.fmin(dmin, sgn * ((ex * fy - ey * fx) / el))
    with np.errstate(all="ignore"):
        cov = np.where(dmin < np.inf, np.clip(dtype(0.5) + dmin, dtype(0), dtype(1)), dtype(0))
    return _blend(c, np.full(3, 0.5, dtype), dtype(0.5) * cov)


def render(joints, chains, lengths=None, *, dtype, proj, affine, W, H, joints2=None, palette=None, traces=(), scale=1.3, dpi=100.0,
           overlay=None, frames=None):
    """joints [B, T, J, 3] -> the float image [B, t1 - t0, H, W, 3] in `dtype`.  traces: (kind, joint) pairs; palette: int [B, T] or
    None (orange); overlay: uint8 [1 or B, H, W]; frames: (t0, t1)."""
    B, T = joints.shape[:2]
    t0, t1 = (0, T) if frames is None else frames
    M, A = np.asarray(proj).astype(dtype), np.asarray(affine).astype(dtype)
    sc = dtype(scale)
    reach = [dtype(pt * float(np.float32(dpi)) / 72.0) * dtype(0.5) + dtype(0.5) for pt in (4.0, 2.0)]
    bd = bounds(joints, lengths, scale, dtype, joints2)
    CX = (np.arange(W).astype(dtype) + dtype(0.5))[None, :]
    CY = ((H - np.arange(H)).astype(dtype) - dtype(0.5))[:, None]
    colours = PALETTE.astype(dtype) / dtype(255)
    out = np.zeros((B, t1 - t0, H, W, 3), dtype)
    for b in range(B):
        n = T if lengths is None else int(lengths[b])
        mins, maxs = bd[b, :3], bd[b, 3:]
        skel = [joints[b].astype(dtype)] + ([] if joints2 is None else [joints2[b].astype(dtype)])
        for t in range(t0, min(t1, n)):
            tx, tz = sc * skel[0][t, 0, 0], sc * skel[0][t, 0, 2]

            def seen(sk, k, j, flat=False):
                x = sc * sk[k, j, 0] - tx
                y = np.zeros_like(x) if flat else sc * sk[k, j, 1] - mins[1]
                z = sc * sk[k, j, 2] - tz
                return project(x, y, z, M, A)

            c = np.ones((H, W, 3), dtype)
            qx, qy = project(np.array([mins[0], mins[0], maxs[0], maxs[0]]) - tx, np.zeros(4, dtype),
                             np.array([mins[2], maxs[2], maxs[2], mins[2]]) - tz, M, A)
            c = _quad_layer(c, qx, qy, CX, CY)
            pal = 1 if palette is None else int(np.clip(palette[b, t], 0, len(PALETTE) - 1))
            for ci, chain in enumerate(chains[:CHAINS_DRAWN]):
                for sk in skel:
                    if len(chain) >= 2:
                        px, py = seen(sk, t, np.asarray(chain))
                        c = _line_layer(c, _polyline_d2(px, py, CX, CY), reach[0], colours[pal, ci])
            for kind, j in traces:
                ks = np.arange(t + 1 if kind == JOINT else t)
                if len(ks) >= 2:
                    px, py = seen(skel[0], ks, j if kind == JOINT else 0, flat=kind == ROOT_HORIZONTAL)
                    c = _line_layer(c, _polyline_d2(px, py, CX, CY), reach[1], colours[pal, 0])
            if overlay is not None:
                a = overlay[0 if overlay.shape[0] == 1 else b].astype(dtype) / dtype(255)
                c = _blend(c, np.zeros(3, dtype), a)
            out[b, t - t0] = c
    return out


def quantise(f):
    """floor(255 f + 0.5) in the image's own type -> uint8."""
    t = f.dtype.type
    return np.floor(t(255) * f + t(0.5)).astype(np.uint8)
