"""Pose tracks: what the fused video path costs beside the same computation in torch ops on the same device.  64 tracks x 300 frames of
24 quaternions at 30 fps (rate 3/2: 200 output frames a track), a standing figure's joint table, translation on.

  track_joints       `track_joints_batch` (k_track_joints: one launch)            vs  batched slerp, q2axangle, Rodrigues, J0 + Jdirs beta, the
                                                                                      22-joint chain as a Python loop of batched matmuls, lerp
                                                                                      of the translation, re-axing: float32 torch ops
  track_to_features  the above, then `retarget_joints` and `encode_joints` ("hml") vs  the torch joints through the same two native stages
  from the host      `track_to_features` and `track_joints` on a list of PoseTracks of numpy arrays: padding, one upload and the launches

The two sides of a pair are interleaved: each is called once untimed, then `--reps` (5) rounds of native, torch, each event-timed around
a synchronised call; medians, in ms per batch.  The largest difference between the two sets of joints is printed with them (relative to
the largest magnitude).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tracks", type=int, default=64)
    ap.add_argument("--frames", type=int, default=300)
    args = ap.parse_args()
    from fractions import Fraction
    import numpy as np
    import torch
    import mst_amd  # noqa: F401
    import track_fixture as tf
    from mst_amd.utils import pose_track as pt
    from mst_amd.utils.motion_process import encode_joints, retarget_joints

    dev = torch.device("cuda:0")
    B, T, rate = args.tracks, args.frames, pt.parse_rate(fps=30)
    up, down = pt.up_down(rate)
    K = int(pt.out_frames(T, rate))

    # ---- a standing figure in the estimator's camera axes, small joint rotations over a root that drifts
    sk = tf.human()
    rest = np.zeros((22, 3))
    for j in range(1, 22):
        rest[j] = rest[tf.PARENTS22[j]] + sk.offsets[j]
    g = np.random.default_rng(11)
    body = pt.BodyJoints(tf.reaxis(rest + np.array([0.0, 0.9, 0.0])), g.standard_normal((22, 3, 10)) * 1e-3, np.eye(22), tf.PARENTS22)
    q = np.empty((B, T, 24, 4))
    q[:, 0] = tf.random_quats(g, (B, 24), (0.02, 0.25))
    for t in range(1, T):
        q[:, t] = tf.qmul(tf.random_quats(g, (B, 24), (0.005, 0.03)), q[:, t - 1])
    rot = torch.from_numpy(q.astype(np.float32)).to(dev)
    transl = torch.from_numpy(np.cumsum(np.abs(g.standard_normal((B, T, 3))) * np.array([0.02, 0.0, 0.002]), 1).astype(np.float32)).to(dev)
    betas = torch.from_numpy((g.standard_normal((B, 10)) * 0.3).astype(np.float32)).to(dev)
    raw = sk.raw
    tgt = (sk.offsets * 1.1).astype(np.float32)

    # ---- the torch side
    pos = np.arange(K, dtype=np.int64) * down
    idx = torch.from_numpy(pos // up).to(dev)
    tpar = torch.from_numpy(((pos % up) / up)).to(dev)
    J0, Jd = body.tables(dev)
    parents = [int(p) for p in body.parents]

    def qmul(a, b):
        aw, ax, ay, az = a.unbind(-1)
        bw, bx, by, bz = b.unbind(-1)
        return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                            aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)

    def torch_joints():
        t32 = tpar.to(torch.float32)[None, :, None, None]
        q0, q1 = rot[:, idx, :22], rot[:, idx + 1, :22]
        q0, q1 = q0 / q0.norm(dim=-1, keepdim=True), q1 / q1.norm(dim=-1, keepdim=True)
        rel = qmul(q1, q0 * q0.new_tensor([1, -1, -1, -1]))
        rel = rel / rel.norm(dim=-1, keepdim=True)
        theta0 = torch.acos(rel[..., :1])
        theta0 = torch.where((theta0 <= 10e-10) & (theta0 >= -10e-10), torch.full_like(theta0, 10e-10), theta0)
        theta = t32 * theta0
        qs = qmul(torch.cat([torch.cos(theta), rel[..., 1:] / torch.sin(theta0) * torch.sin(theta)], -1), q0)
        qs = qs / qs.norm(dim=-1, keepdim=True)
        ang = torch.acos(qs[..., :1]) * 2
        s = torch.sin(ang / 2)
        aa = qs[..., 1:] / torch.where(s == 0, torch.full_like(s, 0.1), s) * ang
        a = (aa + 1e-8).norm(dim=-1, keepdim=True)
        d = aa / a
        zero = torch.zeros_like(d[..., 0])
        Km = torch.stack([zero, -d[..., 2], d[..., 1], d[..., 2], zero, -d[..., 0], -d[..., 1], d[..., 0], zero], -1).reshape(B, K, 22, 3, 3)
        R = torch.eye(3, device=dev) + torch.sin(a)[..., None] * Km + (1 - torch.cos(a))[..., None] * (Km @ Km)
        J = J0[None] + torch.einsum("jcn,bn->bjc", Jd, betas)
        GR, Gt = [R[:, :, 0]], [J[:, None, 0].expand(B, K, 3)]
        for j in range(1, 22):
            p = parents[j]
            GR.append(GR[p] @ R[:, :, j])
            Gt.append((GR[p] @ (J[:, None, j] - J[:, None, p])[..., None])[..., 0] + Gt[p])
        t64 = tpar[None, :, None]
        tr = transl[:, idx].double() + t64 * (transl[:, idx + 1].double() - transl[:, idx].double())
        out = torch.stack(Gt, 2).double() + tr[:, :, None]
        return torch.stack([out[..., 2], -out[..., 1], out[..., 0]], -1).float()

    def native_joints():
        return pt.track_joints_batch(rot, transl, betas, body, rate=rate, with_trans=True)[0]

    lens = torch.full((B,), K, dtype=torch.int32, device=dev)

    def features(joints):
        moved = retarget_joints(joints, tgt, raw, pt.T2M_CHAINS, pt.T2M_LEGS, pt.T2M_FACE, lengths=lens)
        return encode_joints(moved, chains=pt.T2M_CHAINS, raw_offsets=raw, face_joint_indx=pt.T2M_FACE, fid_l=pt.T2M_FID_L, fid_r=pt.T2M_FID_R,
                             mode="hml", lengths=lens)[0]

    def pair(native, other):
        native(), other()
        torch.cuda.synchronize()
        ms = ([], [])
        for _ in range(args.reps):
            for k, fn in enumerate((native, other)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                ms[k].append(a.elapsed_time(b))
        return round(statistics.median(ms[0]), 4), round(statistics.median(ms[1]), 4)

    a, b = native_joints(), torch_joints()
    diff = float((a - b).abs().max() / b.abs().max())
    tj = pair(native_joints, torch_joints)
    tf_ms = pair(lambda: features(native_joints()), lambda: features(torch_joints()))
    host = [pt.PoseTrack(transl[i].cpu().numpy(), betas[i].cpu().numpy(), rotations=rot[i].cpu().numpy(), fps=30) for i in range(B)]
    from_host = pair(lambda: pt.track_to_features(host, body, tgt_offsets=tgt, raw_offsets=raw, with_trans=True),
                     lambda: pt.track_joints(host, body, with_trans=True))
    print(json.dumps({"tracks": B, "frames": T, "fps": 30, "out_frames": K, "reps": args.reps,
                      "track_joints_ms": tj[0], "torch_joints_ms": tj[1], "joints_retarget_encode_ms": tf_ms[0],
                      "torch_joints_retarget_encode_ms": tf_ms[1], "track_to_features_from_host_ms": from_host[0],
                      "track_joints_from_host_ms": from_host[1], "native_vs_torch_joints": diff,
                      "rate": str(Fraction(rate))}))


if __name__ == "__main__":
    main()
