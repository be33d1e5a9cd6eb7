"""Golden vectors of the SMPLify stage: the reference's own visualize/joints2smpl/src/smplify.py, customloss.py, prior.py and config.py,
imported unmodified and run for real on the seeded cases of tests/smplify_fixture.py.  Run in the authoring container only (the
reference checkout on the path):
    python tests/golden/make_golden_smplify.py -> smplify.npz

What is the reference's and what is not.  `smplx` and a SMPL body file do not exist here, so `smplx` is stubbed in sys.modules and the
model handed to SMPLify3D is tests/smplify_fixture.py's `smpl_forward` (smplx's Rodrigues form as recalled, over tests/smpl_fixture.py's
`lbs` on the synthetic 83-vertex body); config.GMM_MODEL_DIR points at a temporary synthetic gmm_08.pkl.  Everything above that layer is
the reference's code as it stands: the prior's buffers, the loss functions, guess_init_3d and the whole two-stage schedule.  A float64
run is the same float32 prior buffers cast to double (`pose_prior.double()`), so both runs minimise the same objective.

Stored:
  `tables|<name>`                     config.py's index tables
  `prior|means / precisions / nll_weights / weights / mean`   MaxMixturePrior(dtype=float32)'s buffers and get_mean()
  `body|N<frames>|nj<joints>|<vec/one>|loss, g_pose, g_betas, g_orient, g_cam`   body_fitting_loss_3d (joint weight 600, preserve 5) and
                                      its autograd gradients in float64 at every parity point, confidences a vector with a zero or 1.0
  `camera|N..|nj..|loss, g_orient, g_cam`   camera_fitting_loss_3d likewise
  `init|nj<joints>`                   guess_init_3d at the end-to-end start
  `fit|nj<joints>|f64 / f32|loss, err, pose, betas, cam`   SMPLify3D.__call__ at num_iters=30 on 4 frames, run in float64 and in float32:
                                      final loss, mean joint error, parameters
  `fit|spread|loss`, `fit|spread|err` the largest relative float32-float64 difference over the stored fits
Asserted before anything is written: the fixture's float64 restatement equals every reference loss and gradient to 1e-12, the package's
tables and prior buffers equal the reference's, the two runs of every fit agree within 2 % on final loss, the file is below 1 MB."""
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import smpl_fixture as sf  # noqa: E402
import smplify_fixture as xf  # noqa: E402

REF = os.environ.get("MST_REFERENCE", "/root/reference")


class StubModel:
    """What SMPLify3D asks of an smplx model: faces_tensor and a call that returns .joints [N, 45, 3] and .vertices."""

    def __init__(self, dtype):
        self.dtype = dtype
        self.faces_tensor = torch.as_tensor(xf.body83()["faces"])

    def __call__(self, global_orient=None, body_pose=None, betas=None, **kwargs):
        o = types.SimpleNamespace()
        o.vertices, o.joints = xf.smpl_forward(xf.body83(), global_orient, body_pose, betas, self.dtype)
        return o


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "gmm_08.pkl"), "wb") as fh:
            pickle.dump(xf.GMM, fh)
        sys.modules["smplx"] = types.ModuleType("smplx")
        sys.path.insert(0, REF)
        from visualize.joints2smpl.src import config as rconfig
        rconfig.GMM_MODEL_DIR = tmp
        from visualize.joints2smpl.src import smplify as rsmplify
        import customloss as rloss                     # smplify.py puts its own folder on the path and imports these by bare name
        import prior as rprior
        for m in (rconfig, rsmplify, rloss, rprior):
            assert m.__file__.startswith(REF), m.__file__

        # ---- tables and the prior's buffers
        import mst_amd  # noqa: F401
        from mst_amd.visualize.joints2smpl.src import config as mine
        from mst_amd.visualize.joints2smpl.src.prior import MaxMixturePrior
        for name in ("JOINT_MAP", "AMASS_JOINT_MAP"):
            assert getattr(mine, name) == getattr(rconfig, name), name
            out[f"tables|{name}|names"] = np.array(sorted(getattr(rconfig, name)))
            out[f"tables|{name}"] = np.array([getattr(rconfig, name)[k] for k in sorted(getattr(rconfig, name))], np.int64)
        for name in ("full_smpl_idx", "key_smpl_idx", "amass_idx", "amass_smpl_idx"):
            assert list(getattr(mine, name)) == list(getattr(rconfig, name)), name
            out[f"tables|{name}"] = np.array(list(getattr(rconfig, name)), np.int64)
        rp = rprior.MaxMixturePrior(prior_folder=tmp, num_gaussians=8, dtype=torch.float32)
        mp = MaxMixturePrior.from_pkl(os.path.join(tmp, "gmm_08.pkl"))
        for name in ("means", "precisions", "nll_weights", "weights"):
            ref = getattr(rp, name).numpy()
            assert np.array_equal(ref, getattr(mp, name).numpy()) and np.array_equal(ref, xf.PRIOR[name]), name
            out[f"prior|{name}"] = ref
        assert np.array_equal(rp.get_mean().numpy(), mp.get_mean().numpy())
        out["prior|mean"] = rp.get_mean().numpy()
        rp64 = rprior.MaxMixturePrior(prior_folder=tmp, num_gaussians=8, dtype=torch.float32).double()

        # ---- the parity points: the reference's losses and autograd gradients in float64
        model64 = StubModel(torch.float64)
        worst = 0.0
        for N, nj in xf.PARITY:
            c = xf.make_case(N, nj)
            xf.check_case(c)
            cat = "AMASS" if nj == 22 else "orig"
            idx = list(range(nj))
            for stage, confs in (("body", ("vec", "one")), ("camera", ("",))):
                for cf in confs:
                    leaf = {k: c[k].double().clone().requires_grad_(True) for k in ("pose", "orient", "betas", "cam")}
                    o = model64(global_orient=leaf["orient"], body_pose=leaf["pose"], betas=leaf["betas"])
                    cam = leaf["cam"].unsqueeze(1)
                    if stage == "body":
                        conf = c["conf"].double() if cf == "vec" else 1.0
                        loss = rloss.body_fitting_loss_3d(leaf["pose"], c["preserve"].double(), leaf["betas"], o.joints[:, idx], cam,
                                                          c["target"].double()[:, idx], rp64, joints3d_conf=conf, joint_loss_weight=600.0,
                                                          pose_preserve_weight=5.0)
                        key, groups = f"body|N{N}|nj{nj}|{cf}", xf.GROUPS
                    else:
                        loss = rloss.camera_fitting_loss_3d(o.joints, cam, c["cam_est"].double().unsqueeze(1), c["target"].double(), cat)
                        key, groups = f"camera|N{N}|nj{nj}", ("g_orient", "g_cam")
                    loss.backward()
                    ref = {"loss": loss.detach().numpy(), "g_pose": leaf["pose"].grad, "g_betas": leaf["betas"].grad,
                           "g_orient": leaf["orient"].grad, "g_cam": leaf["cam"].grad}
                    got = xf.evaluate(c, stage, torch.float64, conf=None if cf in ("vec", "") else 1.0)
                    for g in ("loss",) + tuple(groups):
                        r = np.asarray(ref[g].numpy() if torch.is_tensor(ref[g]) else ref[g], np.float64)
                        d = sf.distance(got[g], r)
                        worst = max(worst, d)
                        assert d < 1e-12, (key, g, d)
                        out[f"{key}|{g}"] = r
        print(f"fixture float64 vs reference: worst distance {worst:.3e}")

        # ---- the end-to-end fit, in float64 and in float32
        spread = {"loss": 0.0, "err": 0.0}
        for nj in (22, 24):
            cat = "AMASS" if nj == 22 else "orig"
            init_pose, init_betas, j3d = xf.fit_inputs(nj)
            res = {}
            for name, dtype in (("f64", torch.float64), ("f32", torch.float32)):
                model = StubModel(dtype)
                fit = rsmplify.SMPLify3D(smplxmodel=model, batch_size=xf.FIT_FRAMES, joints_category=cat, num_iters=xf.FIT_ITERS,
                                         device=torch.device("cpu"))
                if dtype == torch.float64:
                    fit.pose_prior = fit.pose_prior.double()
                if name == "f64":
                    o = model(global_orient=init_pose[:, :3].to(dtype), body_pose=init_pose[:, 3:].to(dtype), betas=init_betas.to(dtype))
                    out[f"init|nj{nj}"] = rsmplify.guess_init_3d(o.joints, j3d.to(dtype), cat).numpy()
                verts, joints, pose, betas, cam, loss = fit(init_pose.to(dtype), init_betas.to(dtype), torch.zeros(1, 3, dtype=dtype), j3d.to(dtype),
                                                            conf_3d=torch.ones(nj, dtype=dtype))
                err = xf.joint_error(joints.detach().numpy(), cam.detach().numpy(), j3d.numpy(), nj)
                res[name] = (float(loss), err)
                for k, v in (("loss", float(loss)), ("err", err), ("pose", pose.detach().numpy()), ("betas", betas.detach().numpy()),
                             ("cam", cam.detach().numpy())):
                    out[f"fit|nj{nj}|{name}|{k}"] = np.asarray(v, np.float64)
                print(f"fit nj {nj} {name}: final loss {float(loss):.4f}, mean joint error {err:.4e}")
            rl = abs(res["f32"][0] - res["f64"][0]) / res["f64"][0]
            re = abs(res["f32"][1] - res["f64"][1]) / res["f64"][1]
            assert rl < 0.02, f"nj {nj}: the float32 and float64 runs differ by {rl:.3%} on final loss; raise FIT_ITERS"
            spread["loss"], spread["err"] = max(spread["loss"], rl), max(spread["err"], re)
        out["fit|spread|loss"], out["fit|spread|err"] = np.float64(spread["loss"]), np.float64(spread["err"])
        print(f"largest float32-float64 spread: loss {spread['loss']:.3e}, joint error {spread['err']:.3e}")
    path = os.path.join(HERE, "smplify.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"{path}: {len(out)} arrays, {size} bytes")
    assert size < 1_000_000


if __name__ == "__main__":
    main()
