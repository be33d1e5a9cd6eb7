"""What the SMPL tests share: a seeded synthetic body of any vertex count, a torch restatement of the standard SMPL `lbs` and of the
reference's Rotation2xyz pipeline that runs in float64 (the oracle) or float32 (the arithmetic the reference runs), and seeded poses.

Nothing here is a real SMPL body: the template is a seeded point cloud, the blend shapes are noise at 1e-2 of its extent, the joint
regressor and the skinning weights are seeded sparse rows that sum to 1.  The kinematic tree is SMPL's public one."""
import numpy as np
import torch

PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21]
NJ, NB, NIDS, NEXTRA = 24, 10, 21, 9
FEATS = {"rot6d": 6, "rotmat": 9, "rotquat": 4, "rotvec": 3}
JOINTSTYPES = ("vertices", "smpl", "vibe", "a2m", "a2mpl")


def synthetic_body(V, seed=7, dense=False):
    """-> dict of float64 / int64 arrays under the names SMPLBody.from_arrays takes."""
    assert V >= NIDS
    g = np.random.default_rng([seed, V, int(dense)])
    vt = g.uniform(-1.0, 1.0, (V, 3)) * np.array([0.5, 1.0, 0.3])
    extent = float(np.abs(vt).max())
    shapedirs = g.standard_normal((V, 3, NB)) * 1e-2 * extent
    posedirs = g.standard_normal((9 * (NJ - 1), 3 * V)) * 1e-2 * extent

    def sparse_rows(rows, cols, nnz):
        m = np.zeros((rows, cols))
        for r in range(rows):
            idx = g.choice(cols, size=min(nnz, cols), replace=False)
            w = g.uniform(0.1, 1.0, idx.shape[0])
            m[r, idx] = w / w.sum()
        return m
    if dense:
        w = g.uniform(0.05, 1.0, (V, NJ))
        weights = w / w.sum(1, keepdims=True)
    else:
        weights = sparse_rows(V, NJ, 4)
    faces = np.stack([g.choice(V, size=3, replace=False) for _ in range(2 * V)]).astype(np.int64)
    return {"v_template": vt, "shapedirs": shapedirs, "posedirs": posedirs, "J_regressor": sparse_rows(NJ, V, 8), "parents": np.array(PARENTS),
            "lbs_weights": weights, "faces": faces, "J_regressor_extra": sparse_rows(NEXTRA, V, 12),
            "vertex_ids": g.choice(V, size=NIDS, replace=False).astype(np.int64)}


# ------------------------------------------------------------------------------------------ conversions, restated
def rot6d_to_matrix(d6):
    x_raw, y_raw = d6[..., 0:3], d6[..., 3:6]
    x = x_raw / torch.norm(x_raw, dim=-1, keepdim=True)
    z = torch.cross(x, y_raw, dim=-1)
    z = z / torch.norm(z, dim=-1, keepdim=True)
    y = torch.cross(z, x, dim=-1)
    return torch.stack([x, y, z], dim=-1)


def quat_to_matrix(q):
    r, i, j, k = torch.unbind(q, -1)
    s = 2.0 / (q * q).sum(-1)
    o = torch.stack((1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r),
                     s * (i * j + k * r), 1 - s * (i * i + k * k), s * (j * k - i * r),
                     s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j)), -1)
    return o.reshape(q.shape[:-1] + (3, 3))


def rotvec_to_matrix(a):
    ang = torch.norm(a, dim=-1, keepdim=True)
    half = 0.5 * ang
    small = ang.abs() < 1e-6
    safe = torch.where(small, torch.ones_like(ang), ang)
    s = torch.where(small, 0.5 - ang * ang / 48, torch.sin(half) / safe)
    return quat_to_matrix(torch.cat([torch.cos(half), a * s], -1))


def to_matrix(pose_rep, f):
    if pose_rep == "rot6d":
        return rot6d_to_matrix(f)
    if pose_rep == "rotquat":
        return quat_to_matrix(f)
    if pose_rep == "rotvec":
        return rotvec_to_matrix(f)
    return f.reshape(f.shape[:-1] + (3, 3))


# ------------------------------------------------------------------------------------------ lbs, restated
def lbs(body, rot, betas, dtype=torch.float64):
    """rot [N, 24, 3, 3], betas [N, 10] -> (vertices [N, V, 3], joints [N, 54, 3]) in `dtype`: the standard SMPL forward pass
    (v_shaped, J, pose blend shapes, rigid chain, skinning), then the vertex-id joints and the extra regressor."""
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    rot, betas = rot.to(dtype), betas.to(dtype)
    n = rot.shape[0]
    vt, sd, pd = t(body["v_template"]), t(body["shapedirs"])[..., :NB], t(body["posedirs"])
    jr, w, ex = t(body["J_regressor"]), t(body["lbs_weights"]), t(body["J_regressor_extra"])
    v_shaped = vt[None] + torch.einsum("bl,mkl->bmk", betas, sd)
    J = torch.einsum("bik,ji->bjk", v_shaped, jr)
    pf = (rot[:, 1:] - torch.eye(3, dtype=dtype)).reshape(n, -1)
    v_posed = v_shaped + torch.matmul(pf, pd).reshape(n, -1, 3)
    parents = [int(p) for p in body["parents"]]
    GR, Gt = [rot[:, 0]], [J[:, 0]]
    for j in range(1, NJ):
        p = parents[j]
        GR.append(torch.matmul(GR[p], rot[:, j]))
        Gt.append(torch.matmul(GR[p], (J[:, j] - J[:, p])[..., None])[..., 0] + Gt[p])
    GR, Gt = torch.stack(GR, 1), torch.stack(Gt, 1)                       # [N, 24, 3, 3], [N, 24, 3]
    At = Gt - torch.matmul(GR, J[..., None])[..., 0]
    A = torch.cat([GR, At[..., None]], -1)                               # [N, 24, 3, 4]
    T = torch.matmul(w, A.reshape(n, NJ, 12)).reshape(n, -1, 3, 4)
    verts = torch.matmul(T[..., :3], v_posed[..., None])[..., 0] + T[..., 3]
    ids = torch.as_tensor(np.asarray(body["vertex_ids"]), dtype=torch.long)
    joints = torch.cat([Gt, verts[:, ids], torch.einsum("bik,ji->bjk", verts, ex)], 1)
    return verts, joints


def rotation2xyz(body, maps, roots, x, mask, pose_rep, translation, glob, jointstype, vertstrans, betas=None, beta=0.0, glob_rot=None,
                 dtype=torch.float64):
    """The reference's Rotation2xyz.__call__ over `lbs`, every step in `dtype`.  x [B, rows, feats, T] (any float type); -> [B, n, 3, T]."""
    x = x.to(dtype)
    B, _, _, T = x.shape
    if mask is None:
        mask = torch.ones(B, T, dtype=torch.bool)
    xr = (x[:, :-1] if translation else x).permute(0, 3, 1, 2)
    rot = to_matrix(pose_rep, xr[mask])
    if not glob:
        g = to_matrix("rotvec", torch.as_tensor(np.asarray(glob_rot), dtype=dtype).reshape(1, 1, 3)).expand(rot.shape[0], 1, 3, 3)
        rot = torch.cat([g, rot], 1)
    n = rot.shape[0]
    if betas is None:
        betas = torch.zeros(n, NB, dtype=dtype)
        betas[:, 1] = beta
    verts, joints = lbs(body, rot, torch.as_tensor(betas), dtype)
    sel = verts if jointstype == "vertices" else joints[:, torch.as_tensor(np.asarray(maps[jointstype]), dtype=torch.long)]
    out = torch.zeros(B, T, sel.shape[1], 3, dtype=dtype)
    out[mask] = sel
    out = out.permute(0, 2, 3, 1).contiguous()
    if jointstype != "vertices":
        out = out - out[:, [roots[jointstype]]]
    if translation and vertstrans:
        tr = x[:, -1, :3]
        out = out + (tr - tr[:, :, [0]])[:, None]
    return out


# ------------------------------------------------------------------------------------------ seeded inputs
def lengths_mask(lengths, T):
    return torch.arange(T)[None, :] < torch.as_tensor(lengths)[:, None]


def sample(pose_rep, B, T, rows=25, seed=3):
    """x [B, rows, feats, T] float32: seeded rotations of every row but the last, whose features :3 are a translation.  6D inputs stay
    off the reference's unguarded divisions: first vector of norm >= 0.1, cross product of norm >= 0.1 (checked)."""
    g = np.random.default_rng([seed, B, T, rows, FEATS[pose_rep]])
    f = FEATS[pose_rep]
    x = g.standard_normal((B, rows, f, T))
    if pose_rep == "rot6d":
        for _ in range(64):
            a, b = x[:, :, :3], x[:, :, 3:]
            na = np.linalg.norm(a, axis=2)
            nc = np.linalg.norm(np.cross(a / na[:, :, None], b, axis=2), axis=2)
            bad = (na < 0.1) | (nc < 0.1)
            if not bad.any():
                break
            x = np.where(bad[:, :, None, :], g.standard_normal(x.shape), x)
        a, b = x[:, :, :3], x[:, :, 3:]
        na = np.linalg.norm(a, axis=2)
        assert na.min() >= 0.1 and np.linalg.norm(np.cross(a / na[:, :, None], b, axis=2), axis=2).min() >= 0.1
    elif pose_rep == "rotmat":
        q = g.standard_normal((B, rows, 4, T))
        m = quat_to_matrix(torch.as_tensor(np.moveaxis(q, 2, -1))).numpy()          # [B, rows, T, 3, 3]
        x = np.moveaxis(m.reshape(B, rows, T, 9), -1, 2)
    elif pose_rep == "rotquat":
        assert np.linalg.norm(x, axis=2).min() > 1e-3
    elif pose_rep == "rotvec":
        x = x * 0.8
        x[0, 1, :, 0] = 0.0                                   # the small-angle branch: exactly zero, and below 1e-6
        if T > 1:
            x[0, 2, :, 1] = np.array([3e-7, -2e-7, 1e-7])
    x[:, -1] = 0.0
    x[:, -1, :3] = g.standard_normal((B, 3, T)) * 0.5
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32)


def given_betas(n, seed=5):
    return torch.as_tensor(np.random.default_rng([seed, n]).standard_normal((n, NB)) * 0.8, dtype=torch.float32)


GLOB_ROT = [0.3, -1.1, 0.4]


def distance(a, b):
    """max |a - b| over the largest magnitude of b."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)) if b.size else 0.0
