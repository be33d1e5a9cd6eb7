"""The SMPL stage: what a sampler batch costs.  64 clips x (25, 6, 196) -- 24 6D rotations and a translation row, every frame live --
through Rotation2xyz on a seeded synthetic body of the real vertex count (6890; no SMPL file is bundled and none is needed to time
the arithmetic) to
  (a) vertices   [64, 6890, 3, 196]: mst_smpl_pose + mst_smpl_skin, 1.04 GB stored
  (b) smpl       [64, 24, 3, 196]:   mst_smpl_pose alone
  (c) vibe       [64, 49, 3, 196]:   pose, skin into the workspace, mst_smpl_regress
beside the same layer written in torch ops on the same device in the same run (fp32 matmul / bmm / einsum: conversions, blend
shapes, the chain as 23 dependent bmm, skinning, the [B, n, 3, T] permute and the translation), interleaved.  The two big products
(pose blend shapes, weights x transforms) are matmuls; the per-vertex and per-joint 3 x 3 transforms are broadcast multiplies and
sums, NOT batched matmuls: at this size those would be 86 million (frames x vertices) and 301 thousand (frames x joints) tiny
problems in one BLAS call, far past the 65535 a batched launch takes in one grid dimension.  One untimed warm-up each (synchronised
leg by leg, progress on stderr), then `--reps` timed runs each, alternating, device events around a synchronised call; medians.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21]


def synthetic_body(V, seed=1):
    import numpy as np
    g = np.random.default_rng(seed)

    def rows(r, c, nnz):
        m = np.zeros((r, c))
        for i in range(r):
            idx = g.choice(c, nnz, replace=False)
            w = g.uniform(0.1, 1.0, nnz)
            m[i, idx] = w / w.sum()
        return m
    return dict(v_template=g.uniform(-1, 1, (V, 3)), shapedirs=g.standard_normal((V, 3, 10)) * 1e-2, posedirs=g.standard_normal((207, 3 * V)) * 1e-2,
                J_regressor=rows(24, V, 8), parents=np.array(PARENTS), lbs_weights=rows(V, 24, 4), faces=np.zeros((1, 3), np.int64),
                J_regressor_extra=rows(9, V, 12), vertex_ids=g.choice(V, 21, replace=False))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=196)
    ap.add_argument("--vertices", type=int, default=6890)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    import mst_amd  # noqa: F401
    from mst_amd.model import smpl
    from mst_amd.model.rotation2xyz import Rotation2xyz

    dev = torch.device("cuda:0")
    B, T, V = args.clips, args.frames, args.vertices
    arrays = synthetic_body(V)
    body = smpl.SMPLBody.from_arrays(**arrays, device=dev)
    r2x = Rotation2xyz(dev, body=body)
    x = torch.from_numpy(np.random.default_rng(2).standard_normal((B, 25, 6, T)).astype(np.float32)).to(dev)
    kw = dict(mask=None, pose_rep="rot6d", translation=True, glob=True, vertstrans=True, beta=0.7)

    up = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device=dev)
    vt, sd, pd, jr, w, ex = (up(arrays[k]) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights", "J_regressor_extra"))
    ids = torch.as_tensor(arrays["vertex_ids"], device=dev)
    maps = {k: torch.as_tensor(v, device=dev) for k, v in smpl.joint_maps().items()}
    eye = torch.eye(3, device=dev)

    def torch_layer(jointstype):
        """The reference's arithmetic (rotation2xyz.py:38-88 over smplx's lbs) in torch ops on the device."""
        r = x[:, :-1].permute(0, 3, 1, 2).reshape(B * T, 24, 6)
        a = r[..., :3] / torch.norm(r[..., :3], dim=-1, keepdim=True)
        z = torch.cross(a, r[..., 3:], dim=-1)
        z = z / torch.norm(z, dim=-1, keepdim=True)
        rot = torch.stack([a, torch.cross(z, a, dim=-1), z], -1)
        n = rot.shape[0]
        betas = torch.zeros(n, 10, device=dev)
        betas[:, 1] = 0.7
        v_shaped = vt[None] + torch.einsum("bl,mkl->bmk", betas, sd)
        J = torch.einsum("bik,ji->bjk", v_shaped, jr)
        GR, Gt = [rot[:, 0]], [J[:, 0]]
        for j in range(1, 24):
            p = PARENTS[j]
            GR.append(torch.bmm(GR[p], rot[:, j]))
            Gt.append(torch.bmm(GR[p], (J[:, j] - J[:, p])[..., None])[..., 0] + Gt[p])
        GR, Gt = torch.stack(GR, 1), torch.stack(Gt, 1)
        if jointstype == "smpl":
            sel = Gt
        else:
            v_posed = v_shaped + torch.matmul((rot[:, 1:] - eye).reshape(n, -1), pd).reshape(n, -1, 3)
            A = torch.cat([GR, (Gt - (GR * J[:, :, None, :]).sum(-1))[..., None]], -1)
            Tm = torch.matmul(w, A.reshape(n, 24, 12)).reshape(n, -1, 3, 4)
            verts = (Tm[..., :3] * v_posed[:, :, None, :]).sum(-1) + Tm[..., 3]
            sel = verts if jointstype == "vertices" else torch.cat([Gt, verts[:, ids], torch.einsum("bik,ji->bjk", verts, ex)], 1)[:, maps[jointstype]]
        out = sel.reshape(B, T, -1, 3).permute(0, 2, 3, 1).contiguous()
        if jointstype != "vertices":
            out = out - out[:, [smpl.JOINTSTYPE_ROOT[jointstype]]]
        tr = x[:, -1, :3]
        return out + (tr - tr[:, :, [0]])[:, None]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    legs = {}
    for jt in ("vertices", "smpl", "vibe"):
        legs[f"{jt}_kernels"] = lambda jt=jt: r2x(x, jointstype=jt, **kw)
        legs[f"{jt}_torch_ops"] = lambda jt=jt: torch_layer(jt)
    worst = {}
    for jt in ("vertices", "smpl", "vibe"):                  # also the warm-up; the two must agree
        a = legs[f"{jt}_kernels"]()
        torch.cuda.synchronize()
        print(f"warm-up: {jt} kernels done", file=sys.stderr, flush=True)
        b = legs[f"{jt}_torch_ops"]()
        torch.cuda.synchronize()
        print(f"warm-up: {jt} torch ops done", file=sys.stderr, flush=True)
        worst[jt] = float((a - b).abs().max() / b.abs().max())
        del a, b
    ms = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    med = {k: round(statistics.median(v), 4) for k, v in ms.items()}
    print(json.dumps({"tool": "smpl_bench", "clips": B, "frames": T, "vertices": V, "reps": args.reps, "median_ms": med,
                      "all_ms": {k: [round(t, 4) for t in v] for k, v in ms.items()}, "max_difference_over_max_magnitude": worst,
                      "pose_blend_gflop": round(2 * B * T * 207 * 3 * V / 1e9, 1), "stored_gb": round(B * T * V * 12 / 1e9, 3)}))


if __name__ == "__main__":
    main()
