"""SMPLify without a GPU: the fixture's restatement against the reference's recorded losses and gradients (tests/golden/smplify.npz), the
prior's buffers and validation, the index tables, and what the C ABI and the classes refuse before any device is touched."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
import smpl_fixture as sf
import smplify_fixture as xf
from conftest import GOLDEN
from mst_amd import _native
from mst_amd.model import smpl
from mst_amd.visualize.joints2smpl.src import config
from mst_amd.visualize.joints2smpl.src.prior import MaxMixturePrior
from mst_amd.visualize.joints2smpl.src.smplify import SMPLify3D, guess_init_3d
from mst_amd.visualize import simplify_loc2rot


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "smplify.npz"))


# ------------------------------------------------------------------------------------------ the fixture is the reference's objective
@pytest.mark.parametrize("N,nj", xf.PARITY)
def test_fixture_equals_the_reference(gold, N, nj):
    c = xf.make_case(N, nj)
    picked = xf.check_case(c)
    if N >= 4:
        assert not c["pose"][1].any() and not c["orient"][1].any()                  # the all-zero frame
        assert len(set(picked.tolist())) >= 3
    for conf, tag in ((None, "vec"), (1.0, "one")):
        got = xf.evaluate(c, "body", torch.float64, conf=conf)
        assert np.isclose(got["per_frame"].sum(), got["loss"], rtol=1e-14)
        for g in ("loss",) + xf.GROUPS:
            assert sf.distance(got[g], gold[f"body|N{N}|nj{nj}|{tag}|{g}"]) < 1e-12, (tag, g)
    got = xf.evaluate(c, "camera", torch.float64)
    for g in ("loss", "g_orient", "g_cam"):
        assert sf.distance(got[g], gold[f"camera|N{N}|nj{nj}|{g}"]) < 1e-12, g
    assert (c["conf"] == 0).sum() == 1


def test_recorded_fits_agree_with_each_other(gold):
    for nj in (22, 24):
        l64, l32 = float(gold[f"fit|nj{nj}|f64|loss"]), float(gold[f"fit|nj{nj}|f32|loss"])
        assert abs(l32 - l64) / l64 < 0.02
        assert abs(l32 - l64) / l64 <= float(gold["fit|spread|loss"])
    assert xf.FIT_ITERS >= 30


def test_rodrigues_form_at_zero_and_its_gradient():
    th = torch.zeros(2, 3, dtype=torch.float64, requires_grad=True)
    R = xf.rodrigues(th)
    assert torch.equal(R.detach(), torch.eye(3, dtype=torch.float64).expand(2, 3, 3))
    (R[:, 2, 1] - R[:, 1, 2]).sum().backward()                 # d/dtheta_x of the x generator's entries: 2
    assert torch.allclose(th.grad, torch.tensor([[2.0, 0.0, 0.0]] * 2, dtype=torch.float64), atol=1e-6)


# ------------------------------------------------------------------------------------------ the prior
def test_prior_buffers_are_the_references(gold, tmp_path):
    with open(tmp_path / "gmm_08.pkl", "wb") as fh:
        pickle.dump(xf.GMM, fh)
    p = MaxMixturePrior.from_pkl(str(tmp_path / "gmm_08.pkl"))
    q = MaxMixturePrior.from_arrays(**xf.GMM)
    for name in ("means", "precisions", "nll_weights", "weights"):
        assert np.array_equal(getattr(p, name).numpy(), gold[f"prior|{name}"]), name
        assert torch.equal(getattr(p, name), getattr(q, name)) and getattr(p, name).dtype == torch.float32
    assert np.array_equal(p.get_mean().numpy(), gold["prior|mean"]) and p.get_mean().shape == (1, 69)
    sym = p.symmetric_precisions()
    assert sym.dtype == np.float32 and np.array_equal(sym, sym.transpose(0, 2, 1))
    assert np.abs(sym - p.precisions.numpy()).max() <= 1e-6 * np.abs(sym).max()
    # the symmetric part gives the same quadratic form and autograd's gradient of the asymmetric one
    d = torch.as_tensor(np.random.default_rng(3).standard_normal(69))
    P = p.precisions[2].double()
    assert torch.allclose(0.5 * (P + P.T) @ d, 0.5 * (P @ d + P.T @ d), rtol=1e-15)


def test_prior_validation(tmp_path):
    g = xf.GMM
    with pytest.raises(ValueError, match="means of shape"):
        MaxMixturePrior.from_arrays(means=g["means"][:6], covars=g["covars"], weights=g["weights"])
    with pytest.raises(ValueError, match="covars of shape"):
        MaxMixturePrior.from_arrays(means=g["means"], covars=g["covars"][:, :60, :60], weights=g["weights"])
    with pytest.raises(ValueError, match="weights"):
        MaxMixturePrior.from_arrays(means=g["means"], covars=g["covars"], weights=g["weights"][:7])
    bad = g["weights"].copy()
    bad[3] = 0.0
    with pytest.raises(ValueError, match="positive"):
        MaxMixturePrior.from_arrays(means=g["means"], covars=g["covars"], weights=bad)
    cov = g["covars"].copy()
    cov[1] = -cov[1]
    with pytest.raises(ValueError, match="positive definite"):
        MaxMixturePrior.from_arrays(means=g["means"], covars=cov, weights=g["weights"])
    nan = g["means"].copy()
    nan[0, 0] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        MaxMixturePrior.from_arrays(means=nan, covars=g["covars"], weights=g["weights"])
    with open(tmp_path / "list.pkl", "wb") as fh:
        pickle.dump([1, 2], fh)
    with pytest.raises(ValueError, match="dict form"):
        MaxMixturePrior.from_pkl(str(tmp_path / "list.pkl"))
    with open(tmp_path / "short.pkl", "wb") as fh:
        pickle.dump({"means": g["means"]}, fh)
    with pytest.raises(KeyError, match="covars"):
        MaxMixturePrior.from_pkl(str(tmp_path / "short.pkl"))


# ------------------------------------------------------------------------------------------ tables
def test_index_tables(gold):
    for name in ("JOINT_MAP", "AMASS_JOINT_MAP"):
        table = getattr(config, name)
        assert sorted(table) == [str(s) for s in gold[f"tables|{name}|names"]]
        assert [table[k] for k in sorted(table)] == gold[f"tables|{name}"].tolist()
    for name in ("full_smpl_idx", "key_smpl_idx", "amass_idx", "amass_smpl_idx"):
        assert list(getattr(config, name)) == gold[f"tables|{name}"].tolist()
    assert [config.JOINT_MAP[j] for j in config.TORSO_JOINTS] == xf.SEL == [config.AMASS_JOINT_MAP[j] for j in config.TORSO_JOINTS]
    j3d, joints = torch.arange(2 * 22 * 3.0).reshape(2, 22, 3), torch.ones(2, 45, 3)
    assert torch.equal(guess_init_3d(joints, j3d, "AMASS"), j3d[:, xf.SEL].mean(1) - 1)


# ------------------------------------------------------------------------------------------ refusals without a GPU
def _objective(lib, stage=1, nj=22, frames=4, parents=None, null=(), w=True):
    """mst_smplify_objective on made-up non-null addresses: every refusal below happens before a pointer is read."""
    a = {k: C.c_void_p(4096) for k in ("pose", "orient", "betas", "cam", "target", "conf", "preserve", "est", "j0", "jdirs", "prior", "ws", "per")}
    for k in null:
        a[k] = None
    par = (C.c_int32 * 24)(*(sf.PARENTS if parents is None else parents))
    wt = _native.MstSmplifyWeights(100.0, 600.0, 7.17, 15.2, 5.0, 5.0, 0.0)
    return lib.mst_smplify_objective(stage, nj, frames, a["pose"], a["orient"], a["betas"], a["cam"], a["target"], a["conf"], a["preserve"], a["est"],
                                     a["j0"], a["jdirs"], par, a["prior"], C.byref(wt) if w else None, a["ws"], a["per"], None, None, None, None,
                                     None, None, None)


def test_abi_refusals():
    import __graft_entry__ as g
    g.build()
    lib = _native.lib()
    assert lib.mst_smplify_packed_prior_bytes() == (8 * 5 * 9 * 64 * 2 + 8 * 72 + 8) * 4
    assert lib.mst_smplify_workspace_bytes(196) >= 196 * 24 * 3 * 4 and lib.mst_smplify_workspace_bytes(196) % 256 == 0
    assert lib.mst_smplify_workspace_bytes(0) == -1 and b"frames" in lib.mst_last_error()
    assert lib.mst_smplify_pack_prior(None, C.c_void_p(4096), C.c_void_p(4096), C.c_void_p(4096), None) != 0 and b"null" in lib.mst_last_error()
    for kw, word in ((dict(stage=2), b"stage"), (dict(stage=-1), b"stage"), (dict(nj=23), b"target joints"), (dict(nj=45), b"target joints"),
                     (dict(frames=0), b"frames"), (dict(null=("pose",)), b"null"), (dict(null=("target",)), b"null"), (dict(null=("ws",)), b"null"),
                     (dict(w=False), b"null"), (dict(null=("prior",)), b"body stage"), (dict(null=("conf",)), b"body stage"),
                     (dict(stage=0, null=("est",)), b"camera stage"),
                     (dict(parents=[0] + sf.PARENTS[1:]), b"parents[0]"), (dict(parents=sf.PARENTS[:5] + [7] + sf.PARENTS[6:]), b"earlier joint"),
                     (dict(parents=sf.PARENTS[:5] + [-1] + sf.PARENTS[6:]), b"earlier joint")):
        assert _objective(lib, **kw) != 0, kw
        assert word in lib.mst_last_error(), (kw, lib.mst_last_error())
    # a body-pose gradient asked of the camera stage
    a, par = C.c_void_p(4096), (C.c_int32 * 24)(*sf.PARENTS)
    wt = _native.MstSmplifyWeights()
    assert lib.mst_smplify_objective(0, 22, 4, a, a, a, a, a, None, None, a, a, a, par, None, C.byref(wt), a, a, None, a, None, None, None, None, None) != 0
    assert b"camera stage has no" in lib.mst_last_error()
    assert C.sizeof(_native.MstSmplifyWeights) == 7 * 4


def test_class_refusals():
    body = smpl.SMPLBody.from_arrays(**xf.body83(), device="cuda")
    prior = MaxMixturePrior.from_arrays(**xf.GMM)
    with pytest.raises(NotImplementedError, match="mesh_intersection"):
        SMPLify3D(body, use_collision=True, pose_prior=prior)
    with pytest.raises(TypeError, match="smplxmodel"):
        SMPLify3D(object(), pose_prior=prior)
    with pytest.raises(TypeError, match="MaxMixturePrior"):
        SMPLify3D(body, pose_prior=None)
    with pytest.raises(ValueError, match="joints_category"):
        SMPLify3D(body, joints_category="H36M", pose_prior=prior)
    with pytest.raises(TypeError):
        SMPLify3D(body)                                                              # the prior is the caller's: no default
    fit = SMPLify3D(smpl.SMPL(body), 1e-2, 4, 30, False, True, "AMASS", torch.device("cuda:0"), pose_prior=prior)
    assert fit.num_joints == 22 and fit.num_iters == 30 and fit.use_lbfgs and list(fit.smpl_index) == list(config.amass_smpl_idx)
    z = lambda *s: torch.zeros(*s)
    with pytest.raises(ValueError, match="stage"):
        fit.objective("hands", z(4, 69), z(4, 3), z(4, 10), z(4, 3), z(4, 22, 3))
    with pytest.raises(RuntimeError, match="GPU only"):
        fit.objective("body", z(4, 69), z(4, 3), z(4, 10), z(4, 3), z(4, 22, 3))
    with pytest.raises(RuntimeError, match="GPU only"):
        fit(z(4, 72), z(4, 10), z(1, 3), z(4, 22, 3))
    with pytest.raises(ValueError, match="joints_category"):
        guess_init_3d(z(4, 45, 3), z(4, 22, 3), "H36M")
    kw = dict(body=body, pose_prior=prior, mean_pose=np.zeros(72), mean_shape=np.zeros(10))
    with pytest.raises(TypeError, match="body="):
        simplify_loc2rot.joints2smpl(4, 0, **dict(kw, body=None))
    with pytest.raises(TypeError, match="pose_prior="):
        simplify_loc2rot.joints2smpl(4, 0, **dict(kw, pose_prior=7))
    with pytest.raises(ValueError, match="expected 72 and 10"):
        simplify_loc2rot.joints2smpl(4, 0, **dict(kw, mean_pose=np.zeros(69)))
    with pytest.raises(TypeError, match="mean_pose="):
        simplify_loc2rot.joints2smpl(4, 0, **dict(kw, mean_shape=None))


def test_mean_parameter_files(tmp_path):
    np.savez(tmp_path / "mean.npz", pose=np.arange(72.0), shape=np.arange(10.0))
    pose, shape = simplify_loc2rot.load_mean_params(str(tmp_path / "mean.npz"))
    assert pose.dtype == np.float32 and np.array_equal(pose, np.arange(72.0)) and np.array_equal(shape, np.arange(10.0))
    try:
        import h5py  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="h5py"):
            simplify_loc2rot.load_mean_params(str(tmp_path / "neutral_smpl_mean_params.h5"))


def test_conversions_of_the_output():
    a = torch.as_tensor(np.random.default_rng(2).standard_normal((6, 3)))
    a[0] = 0.0
    m = simplify_loc2rot.axis_angle_to_matrix(a)
    assert sf.distance(m.numpy(), sf.rotvec_to_matrix(a).numpy()) < 1e-15
    d6 = simplify_loc2rot.matrix_to_rotation_6d(m)
    assert torch.equal(d6, torch.cat([m[:, :, 0], m[:, :, 1]], -1))                 # the first two columns
    assert sf.distance(sf.rot6d_to_matrix(d6).numpy(), m.numpy()) < 1e-14           # the inverse of the package's 6D decoding
