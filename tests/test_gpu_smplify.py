"""SMPLify on the GPU (csrc/mst_smplify.h, visualize/joints2smpl/src/, visualize/simplify_loc2rot.py, visualize/vis_utils.py).

Yardsticks.  tests/smplify_fixture.py restates the reference's objective in torch; tests/golden/make_golden_smplify.py holds that
restatement to the reference's own functions at 1e-12 (tests/test_smplify_cpu.py re-checks it against the stored values).  Precision is
the project's bar, `held` of tests/test_gpu_smpl.py: the kernel's distance from the float64 restatement is at most 4 x the float32
restatement's distance, floor 1e-6 -- applied separately to the loss, the per-frame losses and each gradient group, each relative to its
own largest entry.  `-s` prints every ratio.

End to end.  The reference's own fit (4 frames, num_iters=30) was recorded in float64 and in float32; the native fit must end no worse
than the float64 run plus 4 x the largest relative float32-float64 spread of the stored runs (loss 4.9e-4, mean joint error 3.4e-2),
i.e. final loss <= 1.00196 x and mean joint error <= 1.136 x the float64 run's.  Measured on an MI355X: precision ratios (error over
bar) at most 0.47 in the body stage and 0.39 in the camera stage; the fits below."""
import os

import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
import smpl_fixture as sf
import smplify_fixture as xf
from conftest import GOLDEN
from mst_amd.model import smpl
from mst_amd.model.rotation2xyz import Rotation2xyz
from mst_amd.visualize.joints2smpl.src.prior import MaxMixturePrior
from mst_amd.visualize.joints2smpl.src.smplify import SMPLify3D, guess_init_3d
from mst_amd.visualize.simplify_loc2rot import joints2smpl

pytestmark = pytest.mark.gpu

NAMES = {"g_pose": "body_pose", "g_betas": "betas", "g_orient": "global_orient", "g_cam": "camera_translation"}
_STATE = {}


def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def parts():
    """-> (SMPLBody on the 83-vertex fixture body, MaxMixturePrior on the fixture mixture), built once."""
    if "parts" not in _STATE:
        _STATE["parts"] = (smpl.SMPLBody.from_arrays(**xf.body83(), device=dev()), MaxMixturePrior.from_arrays(**xf.GMM))
    return _STATE["parts"]


def fitter(nj, **kw):
    body, prior = parts()
    return SMPLify3D(body, joints_category="AMASS" if nj == 22 else "orig", device=dev(), pose_prior=prior, **kw)


def oracle(N, nj, stage, conf):
    """The float64 and float32 restatements of one parity point, computed once."""
    key = (N, nj, stage, conf)
    if key not in _STATE:
        c = xf.make_case(N, nj)
        xf.check_case(c)
        _STATE[key] = (c, xf.evaluate(c, stage, torch.float64, conf=conf), xf.evaluate(c, stage, torch.float32, conf=conf))
    return _STATE[key]


def native(fit, c, stage, conf=None, want=("body_pose", "betas", "global_orient", "camera_translation"), out=None, rows=None):
    t = lambda k: (c[k] if rows is None else c[k][rows]).to(dev()).contiguous()
    kw = dict(conf_3d=c["conf"].to(dev()) if conf is None else conf, preserve_pose=t("preserve")) if stage == "body" else dict(camera_estimate=t("cam_est"))
    loss, per, g = fit.objective(stage, t("pose"), t("orient"), t("betas"), t("cam"), t("target"), want=want, out=out, **kw)
    res = {"loss": loss, "per_frame": per}
    res.update({k: g[v] for k, v in NAMES.items() if v in g})
    return res


def held(name, got, f64, f32):
    err, ref = sf.distance(got, f64), sf.distance(f32, f64)
    bar = max(4 * ref, 1e-6)
    print(f"{name}: kernel {err:.3e}  float32 restatement {ref:.3e}  bar {bar:.3e}  ratio {err / bar:.3f}")
    assert err <= bar, f"{name}: {err:.3e} from float64, bar {bar:.3e} (float32 restatement: {ref:.3e})"
    return err / bar


# ------------------------------------------------------------------------------------------ precision
@pytest.mark.parametrize("N,nj", xf.PARITY)
def test_body_stage_precision(N, nj):
    fit = fitter(nj)
    # the confidence vector (one entry zero) with every gradient; the scalar confidence without the betas gradient
    for conf, want in ((None, ("body_pose", "betas", "global_orient", "camera_translation")), (1.0, ("body_pose", "global_orient", "camera_translation"))):
        c, f64, f32 = oracle(N, nj, "body", conf)
        got = native(fit, c, "body", conf, want)
        assert ("g_betas" in got) == ("betas" in want)
        for k in ("loss", "per_frame") + tuple(g for g in xf.GROUPS if g in got):
            held(f"body|N{N}|nj{nj}|{'vec' if conf is None else 'one'}|{k}", got[k].cpu().numpy(), f64[k], f32[k])


@pytest.mark.parametrize("N,nj", xf.PARITY)
def test_camera_stage_precision(N, nj):
    c, f64, f32 = oracle(N, nj, "camera", None)
    got = native(fitter(nj), c, "camera")
    assert "g_pose" not in got and "g_betas" not in got
    for k in ("loss", "per_frame", "g_orient", "g_cam"):
        held(f"camera|N{N}|nj{nj}|{k}", got[k].cpu().numpy(), f64[k], f32[k])


def test_rotations_and_joints_come_back():
    c, _, _ = oracle(17, 24, "body", None)
    fit = fitter(24)
    t = lambda k: c[k].to(dev())
    _, _, g = fit.objective("body", t("pose"), t("orient"), t("betas"), t("cam"), t("target"), conf_3d=1.0, preserve_pose=t("preserve"), want=(),
                            rotations=True, joints=True, total=False)
    theta = torch.cat([c["orient"][:, None], c["pose"].reshape(17, 23, 3)], 1).double()
    assert sf.distance(g["rotations"].cpu().numpy(), xf.rodrigues(theta).numpy()) < 1e-6
    assert torch.equal(g["rotations"][1], torch.eye(3, device=dev()).expand(24, 3, 3))           # the all-zero frame: exactly I
    _, joints = xf.smpl_forward(xf.body83(), c["orient"], c["pose"], c["betas"], torch.float64)
    assert sf.distance(g["joints"].cpu().numpy(), joints[:, :24].numpy()) < 2e-6


# ------------------------------------------------------------------------------------------ bits
def test_a_frame_is_the_same_bits_anywhere():
    c, _, _ = oracle(33, 22, "body", None)
    fit = fitter(22)
    for stage in ("body", "camera"):
        for f in (0, 1, 20):                                   # 1: the all-zero pose
            alone = native(fit, c, stage, rows=[f])
            for B, positions in ((3, (0, 2)), (17, (0, 15, 16)), (33, (0, 16, 32))):
                for pos in positions:
                    rows = [(f + 1 + i) % 33 for i in range(B)]
                    rows[pos] = f
                    got = native(fit, c, stage, rows=rows)
                    for k, v in alone.items():
                        if k != "loss":
                            assert torch.equal(got[k][pos], v[0]), (stage, f, B, pos, k)
                    # NaN in every input of every other frame
                    cn = {k: (v[rows].clone() if torch.is_tensor(v) and v.dim() > 1 else v) for k, v in c.items()}
                    for k in ("pose", "orient", "betas", "cam", "target", "preserve", "cam_est"):
                        keep = cn[k][pos].clone()
                        cn[k][:] = float("nan")
                        cn[k][pos] = keep
                    got = native(fit, cn, stage)
                    for k, v in alone.items():
                        if k != "loss":
                            assert torch.equal(got[k][pos], v[0]), (stage, f, B, pos, k, "nan")
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                again = native(fit, c, stage, rows=[f])
            side.synchronize()
            for k, v in alone.items():
                assert torch.equal(again[k], v), (stage, f, k, "side stream")
            assert torch.equal(alone["loss"], alone["per_frame"][0])


def test_total_is_the_ordered_double_sum():
    c, _, _ = oracle(33, 22, "body", None)
    got = native(fitter(22), c, "body")
    s = 0.0
    for v in got["per_frame"].cpu().double().tolist():
        s += v
    assert got["loss"].item() == np.float32(s)


def test_a_null_betas_gradient_leaves_the_buffer_untouched():
    c, _, _ = oracle(17, 24, "body", None)
    fit = fitter(24)
    full = native(fit, c, "body")
    sentinel = torch.full((17, 10), -7.5, device=dev())
    bufs = {"betas": sentinel, "body_pose": torch.zeros(17, 69, device=dev())}
    got = native(fit, c, "body", want=("body_pose", "global_orient", "camera_translation"), out=bufs)
    torch.cuda.synchronize()
    assert torch.equal(sentinel, torch.full((17, 10), -7.5, device=dev()))
    assert got["g_pose"] is bufs["body_pose"]
    for k in ("per_frame", "loss", "g_pose", "g_orient", "g_cam"):
        assert torch.equal(got[k], full[k]), k


# ------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "smplify.npz"))


def bars(gold, nj):
    return (float(gold[f"fit|nj{nj}|f64|loss"]) * (1 + 4 * float(gold["fit|spread|loss"])),
            float(gold[f"fit|nj{nj}|f64|err"]) * (1 + 4 * float(gold["fit|spread|err"])))


@pytest.mark.parametrize("nj", (22, 24))
def test_fit_matches_the_reference(gold, nj):
    """The native fit against the reference's recorded float64 run (its float32 run beside it), 4 frames, num_iters=30.
    Measured on an MI355X, as ratios to the float64 run's (the reference's own float32 run in brackets):
      AMASS (22 joints)  final loss 18100.21, ratio 1.00044 (1.00049), bar 1.00196;  mean joint error 1.124e-3, ratio 1.013 (1.015), bar 1.136
      orig  (24 joints)  final loss 18233.81, ratio 1.00040 (1.00035), bar 1.00196;  mean joint error 1.183e-3, ratio 1.044 (1.034), bar 1.136"""
    init_pose, init_betas, j3d = xf.fit_inputs(nj)
    fit = fitter(nj, num_iters=xf.FIT_ITERS, batch_size=xf.FIT_FRAMES)
    cat = "AMASS" if nj == 22 else "orig"
    _, _, g = fit.objective("camera", init_pose[:, 3:].to(dev()).contiguous(), init_pose[:, :3].to(dev()).contiguous(), init_betas.to(dev()),
                            torch.zeros(4, 3, device=dev()), j3d.to(dev()), camera_estimate=torch.zeros(4, 3, device=dev()), want=(), joints=True)
    assert sf.distance(guess_init_3d(g["joints"], j3d.to(dev()), cat).cpu().numpy(), gold[f"init|nj{nj}"]) < 1e-5
    verts, joints, pose, betas, cam, loss = fit(init_pose.to(dev()), init_betas.to(dev()), torch.zeros(1, 3, device=dev()), j3d.to(dev()),
                                                conf_3d=torch.ones(nj, device=dev()))
    assert verts.shape == (4, 83, 3) and joints.shape == (4, 45, 3) and pose.shape == (4, 72) and betas.shape == (4, 10) and cam.shape == (4, 1, 3)
    err = xf.joint_error(joints.cpu().numpy(), cam.cpu().numpy(), j3d.numpy(), nj)
    l64, e64 = float(gold[f"fit|nj{nj}|f64|loss"]), float(gold[f"fit|nj{nj}|f64|err"])
    l32, e32 = float(gold[f"fit|nj{nj}|f32|loss"]), float(gold[f"fit|nj{nj}|f32|err"])
    lbar, ebar = bars(gold, nj)
    print(f"fit nj {nj}: final loss {float(loss):.4f} (reference float64 {l64:.4f}, float32 {l32:.4f}; ratio {float(loss) / l64:.5f}, bar {lbar / l64:.5f})  "
          f"mean joint error {err:.4e} (float64 {e64:.4e}, float32 {e32:.4e}; ratio {err / e64:.4f}, bar {ebar / e64:.4f})")
    # the returned joints and vertices are those of the returned parameters
    v64, j64 = xf.smpl_forward(xf.body83(), pose[:, :3].cpu(), pose[:, 3:].cpu(), betas.cpu(), torch.float64)
    assert sf.distance(joints.cpu().numpy(), j64.numpy()) < 5e-6 and sf.distance(verts.cpu().numpy(), v64.numpy()) < 5e-6
    assert float(loss) <= lbar, f"final loss {float(loss):.4f} above {lbar:.4f}"
    assert err <= ebar, f"mean joint error {err:.4e} above {ebar:.4e}"


def test_adam_path_lowers_the_loss_and_keeps_the_shape():
    init_pose, init_betas, j3d = xf.fit_inputs(22)
    init_betas = init_betas + 0.1
    fit = fitter(22, num_iters=xf.FIT_ITERS, use_lbfgs=False)
    d = dev()
    bp, go, be, tg = init_pose[:, 3:].to(d).contiguous(), init_pose[:, :3].to(d).contiguous(), init_betas.to(d), j3d.to(d)
    _, _, g = fit.objective("camera", bp, go, be, torch.zeros(4, 3, device=d), tg, camera_estimate=torch.zeros(4, 3, device=d), want=(), joints=True)
    cam0 = guess_init_3d(g["joints"], tg, "AMASS")
    start, _, _ = fit.objective("body", bp, go, be, cam0, tg, weights={"keep": 0.0}, want=())
    _, _, pose, betas, _, loss = fit(init_pose.to(d), be, torch.zeros(1, 3, device=d), tg, seq_ind=1)
    print(f"adam: loss {float(start):.1f} -> {float(loss):.1f}")
    assert float(loss) < float(start)
    assert torch.equal(betas, be) and not torch.equal(pose, init_pose.to(d))


# ------------------------------------------------------------------------------------------ the surface
def make_j2s(frames, iters=xf.FIT_ITERS):
    body, prior = parts()
    init_pose, _, _ = xf.fit_inputs(22)
    return joints2smpl(frames, 0, num_smplify_iters=iters, body=body, pose_prior=prior, mean_pose=init_pose[0].numpy(), mean_shape=np.zeros(10, np.float32))


def test_joint2smpl_and_npy2obj(gold, tmp_path):
    from mst_amd.visualize import vis_utils
    body, _ = parts()
    _, _, j3d = xf.fit_inputs(22)
    motion = np.zeros((2, 22, 3, 4), np.float32)
    motion[1] = j3d.numpy().transpose(1, 2, 0)
    np.save(tmp_path / "xyz.npy", {"motion": motion, "lengths": np.array([4, 4]), "num_samples": 2, "num_repetitions": 1, "text": ["a", "b"]})
    o = vis_utils.npy2obj(str(tmp_path / "xyz.npy"), 1, 0, body=body, device=0, smplify=make_j2s)
    assert o.vertices.shape == (1, 83, 3, 4) and o.real_num_frames == 4 and o.nfeats == 6 and o.njoints == 25
    thetas = torch.as_tensor(o.motions["motion"])
    assert thetas.shape == (1, 25, 6, 4)
    assert torch.equal(thetas[0, 24, :3], j3d[:, 0].T) and not thetas[0, 24, 3:].any()            # the root row: cat(root, zeros)
    assert sorted(o.opt_dict) == ["betas", "cam", "pose"] and o.opt_dict["pose"].shape == (72,)
    assert o.opt_dict["betas"].shape == (4, 10) and o.opt_dict["cam"].shape == (4, 1, 3)
    # the 6D output back through Rotation2xyz: root-relative joints, made absolute by the root's rest position and the fitted camera
    r2x = Rotation2xyz(dev(), body=body)
    rel = r2x(thetas.to(dev()), None, pose_rep="rot6d", translation=True, glob=True, jointstype="smpl", vertstrans=False, betas=o.opt_dict["betas"])
    a = xf.body83()
    betas = o.opt_dict["betas"].cpu().double().numpy()
    root = a["J_regressor"][0] @ (a["v_template"][None] + np.einsum("vci,ni->nvc", a["shapedirs"], betas))           # [4, 3]
    joints = rel[0].permute(2, 0, 1).cpu().double().numpy() + root[:, None]
    err = xf.joint_error(joints, o.opt_dict["cam"].cpu().numpy(), j3d.numpy(), 22)
    print(f"npy2obj round trip: mean joint error {err:.4e}, bar {bars(gold, 22)[1]:.4e}")
    assert err <= bars(gold, 22)[1]
    with pytest.raises(NotImplementedError, match="SMPLify"):
        vis_utils.npy2obj(str(tmp_path / "xyz.npy"), 1, 0, body=body)
    j2s = make_j2s(4, 2)
    same, d = j2s.joint2smpl(j3d.numpy())
    assert same.shape == (1, 25, 6, 4) and sorted(d) == ["betas", "cam", "pose"]
    with pytest.raises(ValueError, match="expected"):
        j2s.joint2smpl(j3d.numpy()[:3])


def test_joints2rotation_applies_the_height_offset():
    from mst_amd.visualize import vis_utils
    _, _, j3d = xf.fit_inputs(22)
    joints = j3d.numpy().copy()
    low = joints[:, :, 1].min()
    assert abs(low) > 1e-2
    out = vis_utils.joints2rotation(joints, 2, smplify=make_j2s)
    assert out.shape == (1, 25, 6, 4)
    assert joints[:, :, 1].min() == 0.0 and np.array_equal(joints[:, :, 1], j3d.numpy()[:, :, 1] - low)      # in place, as the reference
    assert np.array_equal(out[0, 24, :3].cpu().numpy(), joints[:, 0].T)
