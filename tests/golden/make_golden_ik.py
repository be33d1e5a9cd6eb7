"""Golden vectors of the joint-rotation fit: the reference's `InverseKinematics_hmlvec` (data_loaders/humanml/common/Kinematics.py:30-91)
over `Skeleton.forward_kinematics_real_cont6d` (common/skeleton.py:200-222), stepped as `fit_joints_bvh` steps it
(common/bvh_utils.py:1811-1846), and that function's conversion to quaternions, on the seeded skeletons and clips of tests/ik_fixture.py.
Run in the authoring container only (imports the reference checkout that make_golden.py puts on the path):  python tests/golden/make_golden_ik.py -> ik.npz

Stored: the reference's outputs only (inputs are rebuilt from the seed) -- per case (ik_fixture.GOLDEN_CASES) the final cont6d, r_pos and
r_rot_quat, the positions of the last forward pass's successor (FK of the final parameters), the quaternions, the first and last loss, the
gradients of the first step, in fp32 and, with every tensor cast, in float64 (the losses of every case, everything of the short cases); the seconds per clip of 100 fp32 iterations.

Asserted here, before anything is written: the fixture's float64 gradients equal the reference's float64 autograd gradients to 1e-12
relative; the fixture's fp32 results are no further from the reference's fp32 results than the reference's fp32 is from its own float64.
Both distances are printed."""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
from make_golden import SEED  # noqa: E402
import ik_fixture as ik  # noqa: E402

KEYS = ("cont6d", "r_pos", "r_rot_quat", "positions", "joint_quats")


def reference_fit(mods, chains, off, data, target, iters, dtype):
    """fit_joints_bvh up to the point where it builds the animation, in `dtype`.  -> dict of numpy arrays, seconds."""
    K, S, R = mods
    torch.set_default_dtype(dtype)
    plain_float = torch.Tensor.float
    if dtype == torch.float64:                  # the reference's qrot / qmultipy end in .float(): under the cast that means "the working type"
        torch.Tensor.float = lambda self, *a, **k: self.to(torch.float64)
    try:
        skel = S.Skeleton(torch.from_numpy(off), chains, "cpu")
        skel._raw_offset = skel._raw_offset.to(dtype)
        solver = K.InverseKinematics_hmlvec(torch.from_numpy(data.copy()).to(dtype), len(off), skel, off.astype(np.float64),
                                            torch.from_numpy(target.copy()).to(dtype))      # (the solver steps a view of its input in place)
        assert solver.offset.dtype == dtype and solver.cont6d_params.dtype == dtype and solver.r_rot_quat.dtype == dtype
        losses, grads = [], None
        t0 = time.perf_counter()
        for it in range(iters):
            losses.append(solver.step())
            if it == 0:
                grads = [solver.cont6d_params.grad.clone(), solver.r_pos.grad.clone(), solver.r_rot_quat.grad.clone()]
        seconds = time.perf_counter() - t0
        c, rp, q = solver.cont6d_params.detach(), solver.r_pos.detach(), solver.r_rot_quat.detach()
        quats = R.cont6d2q(c)
        quats[..., 0, :] = R.qmultipy(R.qnorm(q), quats[..., 0, :]).to(dtype)
        pos = skel.forward_kinematics_real_cont6d(c, rp, q, solver.offset)
        out = dict(cont6d=c, r_pos=rp, r_rot_quat=q, positions=pos, joint_quats=quats)
        out = {k: v.numpy().copy() for k, v in out.items()}
        out["loss"] = np.array([losses[0], losses[-1]], np.float64)
        out["grad"] = ik.flat_grad([g.numpy() for g in grads])
        return out, seconds
    finally:
        torch.Tensor.float = plain_float
        torch.set_default_dtype(torch.float32)


def main():
    mg.install_shims()
    import importlib
    K = importlib.import_module("data_loaders.humanml.common.Kinematics")
    S = importlib.import_module("data_loaders.humanml.common.skeleton")
    R = importlib.import_module("data_loaders.humanml.common.rotation")
    mods = (K, S, R)
    torch.set_num_threads(8)
    out = {}
    for J, T, iters in ik.GOLDEN_CASES:
        chains, parents, off, data, target = ik.golden_inputs(SEED, J, T)
        assert S.Skeleton(torch.from_numpy(off), chains, "cpu")._parents == parents
        ref32, seconds = reference_fit(mods, chains, off, data, target, iters, torch.float32)
        ref64, _ = reference_fit(mods, chains, off, data, target, iters, torch.float64)
        assert ref32["cont6d"].dtype == np.float32 and ref64["cont6d"].dtype == np.float64
        ik.assert_angles_clear(ref64["cont6d"])
        mine64 = ik.solve(data[None], parents, off, target[None], iters, np.float64)
        mine32 = ik.solve(data[None], parents, off, target[None], iters, np.float32)
        # the gradient of the first step, float64 against float64 autograd
        g64 = ik.solve(data[None], parents, off, target[None], 1, np.float64)["grad"][0]
        gref = reference_fit(mods, chains, off, data, target, 1, torch.float64)[0]["grad"]
        gdev = float(np.abs(g64 - gref).max() / np.abs(gref).max())
        true64 = ik.solve(data[None], parents, off, target[None], 1, np.float64, true_gradient=True)["grad"][0]
        print(f"J{J} T{T} it{iters}: fixture f64 gradient vs autograd f64 {gdev:.2e} (largest entry {np.abs(gref).max():.3g}; "
              f"the true gradient differs by {np.abs(true64 - gref).max():.3g})")
        assert gdev <= 1e-12
        lv = [j for j in ik.leaves(parents)]
        assert not ref32["grad"].reshape(T, -1)[:, :6 * J].reshape(T, J, 6)[:, lv].any()
        for k in KEYS:
            own, fix = ik.rel(ref32[k], ref64[k]), ik.rel(mine32[k][0], ref32[k])
            print(f"J{J} T{T} it{iters} {k}: reference fp32 vs its float64 {own:.2e}; fixture fp32 vs reference fp32 {fix:.2e}; "
                  f"fixture f64 vs reference f64 {ik.rel(mine64[k][0], ref64[k]):.2e}")
            assert fix <= own or fix == 0.0, (J, T, iters, k, fix, own)
        assert ik.rel(mine64["loss"][[0, -1]], ref64["loss"]) <= 1e-12
        assert all(ik.rel(mine64[k][0], ref64[k]) <= 1e-14 for k in KEYS)
        key = f"J{J}T{T}I{iters}"
        for k in KEYS + ("loss", "grad"):
            out[f"{key}|{k}|f32"] = ref32[k].astype(np.float32 if k != "loss" else np.float64)
            if k == "loss" or T <= 7:                 # float64 of the long cases: the fixture's float64 reproduces it to 1e-15 (asserted above)
                out[f"{key}|{k}|f64"] = ref64[k]
        out[f"{key}|seconds"] = np.array(seconds * 100.0 / iters)
        print(f"J{J} T{T} it{iters}: {seconds:.2f} s for {iters} iterations")
    path = os.path.join(HERE, "ik.npz")
    np.savez_compressed(path, **out)
    print("ik.npz", os.path.getsize(path) // 1024, "KiB;", len(out), "arrays")
    assert os.path.getsize(path) < 500 * 1024


if __name__ == "__main__":
    main()
