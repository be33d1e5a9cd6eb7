"""The pose-track path without a GPU: tests/track_fixture.py's restatement against what the reference's own functions returned
(tests/golden/track.npz, written by tests/golden/make_golden_track.py), the output-frame rule, `shortest`, the rates, the file readers,
the joint table and every argument check of utils/pose_track.py, utils/process_smpl_from_hybrik.py, `read_bvh_resampled` and the C ABI.

Bars.  A float32 output of the reference is compared with the float64 restatement under the suite's rule: 4 x the float32 restatement's
own distance from float64 on the same inputs (max |a - b| over the largest magnitude), floor 1e-6.  The reference's translations and
point tracks are float64 and `lerp64(..., as_reference=True)` restates their arithmetic operation by operation: 1e-12."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
import bvh_fixture as bf
import track_fixture as tf
from conftest import GOLDEN
from mst_amd import _native
from mst_amd.utils import bvh, pose_track as pt
from mst_amd.utils import process_smpl_from_hybrik as psh

TABLE = tf.joint_table(tf.body())


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "track.npz")) as z:
        return {k: z[k] for k in z.files}


def within(key, ref, a32, a64, dist=tf.distance):
    own, got = dist(a32, a64), dist(ref, a64)
    print(f"{key}: reference vs restatement f64 {got:.3e}; restatement f32 vs f64 {own:.3e}; bar {tf.bar(own):.3e}")
    assert got <= tf.bar(own), (key, got, own)


# ------------------------------------------------------------------------------------------ the goldens
@pytest.mark.parametrize("T,rate", list(tf.COUNTS))
def test_downsample_restatement_equals_the_reference(gold, T, rate):
    tr = tf.track(tf.SEED, T, flips=T == 9)
    key = f"ds|T{T}|{rate.numerator}_{rate.denominator}"
    rot, pos, joints = gold[key + "|rot"], gold[key + "|pos"], gold[key + "|joints"]
    assert rot.dtype == np.float32 and pos.dtype == np.float64 and joints.dtype == np.float64
    assert len(rot) == len(pos) == len(joints) == tf.COUNTS[(T, rate)] == tf.out_frames(T, rate) == int(pt.out_frames(T, rate))
    within(key, rot, tf.resample_quats(tr["quats"], rate, np.float32), tf.resample_quats(tr["quats"], rate, np.float64))
    assert tf.distance(pos, tf.lerp64(tr["transl"], rate, as_reference=True)) < 1e-12
    assert tf.distance(joints, tf.lerp64(tr["joints"], rate, as_reference=True)) < 1e-12
    # the kernels' lerp forms the difference in double too: within one float32 rounding of the reference's
    assert tf.distance(tf.lerp64(tr["transl"], rate), pos) < 2.0 ** -23


def file_case(gold, name, reference_signs):
    kind, T, fps, with_trans, cut = tf.GOLDEN_FILES[name]
    tr, extra = tf.golden_track(name)
    n = cut or T
    case = {"betas": tr["betas"], "transl": extra if cut else tr["transl"]}
    if "joints" in tr:
        case["joints"] = tr["joints"][:n]
    if kind == "pkl":
        case["quats"] = tr["quats"]
    elif reference_signs:
        case["quats"] = gold[f"file|{name}|rotm2q"]
    else:
        case["mats"] = tr["mats"][:n]
    return case, Fraction(fps, 20), with_trans, n


@pytest.mark.parametrize("name", list(tf.GOLDEN_FILES))
def test_amass_to_pose_restatement_equals_the_reference(gold, name):
    """The reference's formula on the reference's own quaternions (for matrices: what its rotm2q returned, LAPACK's signs included)."""
    case, rate, with_trans, n = file_case(gold, name, True)
    f32, f64 = (tf.track_joints(case, TABLE, rate, dt, with_trans) for dt in (np.float32, np.float64))
    assert gold[f"file|{name}|model"].shape == (tf.out_frames(n, rate), 22, 3)
    within(name + " model", gold[f"file|{name}|model"], f32[0], f64[0])
    if f"file|{name}|est" in gold:
        within(name + " estimator", gold[f"file|{name}|est"], f32[1], f64[1])
    else:
        assert f64[1] is None


@pytest.mark.parametrize("name", [n for n, c in tf.GOLDEN_FILES.items() if c[0] != "pkl"])
def test_matrix_input_equals_the_reference_where_t_is_zero(gold, name):
    """Closed-form quaternion and the shorter arc: the frames that fall on a source frame do not depend on the sign LAPACK chose.
    The bar is the reference's own float32 error there, not the closed form's: where LAPACK returned w < 0 the reference's `q2axangle`
    works at an angle near 2 pi, where float32 loses more (measured: 2.7e-6 against the closed form's 1.5e-7 on pk25) -- so the float32
    restatement whose distance from float64 sets the bar is the one of the reference's formula on the reference's recorded signs."""
    rq = gold[f"file|{name}|rotm2q"]
    case, rate, with_trans, n = file_case(gold, name, False)
    assert tf.quat_distance(tf.rotm2q(case["mats"].astype(np.float64)), rq) < 1e-5
    assert (rq[..., 0] < 0).any()                          # the recorded signs are not all the closed form's
    f32, f64 = (tf.track_joints(case, TABLE, rate, dt, with_trans) for dt in (np.float32, np.float64))
    ref_case = file_case(gold, name, True)[0]
    r32, r64 = (tf.track_joints(ref_case, TABLE, rate, dt, with_trans) for dt in (np.float32, np.float64))
    _, t = tf.frame_params(n, rate)
    on = np.flatnonzero(t == 0)
    assert 0 < len(on) < len(t)
    assert tf.distance(f64[0][on], r64[0][on]) < 1e-6       # the two statements agree where t is 0, to the recorded quaternions' float32 ...
    assert tf.distance(f64[0], r64[0]) > 1e-2               # ... and nowhere else: the reference's in-between frames follow LAPACK's sign
    own = max(tf.distance(r32[0][on], r64[0][on]), tf.distance(f32[0][on], f64[0][on]))
    got = tf.distance(gold[f"file|{name}|model"][on], f64[0][on])
    print(f"{name} model, t = 0: reference vs closed form f64 {got:.3e}; the reference's formula f32 vs f64 {own:.3e}")
    assert got <= tf.bar(own), (name, got, own)
    within(name + " estimator", gold[f"file|{name}|est"], f32[1], f64[1])        # no rotation enters: every frame


def test_the_references_formula_takes_the_longer_arc_on_flipped_signs():
    """0.4 rad apart: slerp(q0, -q1, 0.5) has w = 0.0998 where slerp(q0, q1, 0.5) has 0.995; `shortest` gives the latter for both."""
    q0 = np.array([[1.0, 0, 0, 0]])
    q1 = np.array([[np.cos(0.2), np.sin(0.2), 0, 0]])
    t = np.array([[0.5]])
    assert abs(tf.qslerp(q0, q1, t)[0, 0] - 0.995) < 1e-3 and abs(tf.qslerp(q0, -q1, t)[0, 0] - 0.0998) < 1e-3
    assert np.allclose(tf.qslerp(q0, -q1, t, shortest=True), tf.qslerp(q0, q1, t), atol=1e-15)


def test_shortest_is_invariant_to_negating_any_input_quaternion():
    tr = tf.track(5, 9)
    q = tr["quats"].astype(np.float64)
    rate = Fraction(5, 4)
    want = tf.resample_quats(q, rate, np.float64, shortest=True)
    g = np.random.default_rng(3)
    for _ in range(4):
        sign = np.where(g.integers(0, 2, q.shape[:2] + (1,)) == 0, -1.0, 1.0)
        got = tf.resample_quats(q * sign, rate, np.float64, shortest=True)
        assert tf.quat_distance(got, want) < 1e-13        # the same rotations; a frame's sign follows its interval's first end
        assert tf.distance(tf.resample_quats(q * sign, rate, np.float64), tf.resample_quats(q, rate, np.float64)) > 0.1
        case = {"quats": (q * sign).astype(np.float32), "transl": tr["transl"], "betas": tr["betas"]}
        base = dict(case, quats=tr["quats"])
        assert tf.distance(tf.track_joints(case, TABLE, rate, np.float64, shortest=True)[0],
                           tf.track_joints(base, TABLE, rate, np.float64, shortest=True)[0]) < 1e-6     # the Rodrigues form's 1e-8 in the angle


def test_hml_rows_and_bvh_restatements_equal_the_reference(gold):
    within("pos2hmlrep", gold["hml|rows"], tf.hml_rows(gold["hml|joints"], gold["hml|tgt_offsets"], np.float32),
           tf.hml_rows(gold["hml|joints"], gold["hml|tgt_offsets"], np.float64))
    sk, ch = bvh_case()
    f32, f64 = bf.decode(ch, sk, np.float32), bf.decode(ch, sk, np.float64)
    rate = Fraction(3, 2)
    for key, keep in (("bvh|r15", sk.not_end_index), ("bvh|r15e", list(range(sk.joints)))):
        within(key + " quats", gold[key + "|quats"], *(tf.resample_quats(f["rotations"], rate, dt)[:, keep] for f, dt in ((f32, np.float32), (f64, np.float64))))
        within(key + " pos", gold[key + "|pos"], *(tf.resample_points(f["local_positions"], rate, dt)[:, keep] for f, dt in ((f32, np.float32), (f64, np.float64))))


def bvh_case():
    fsk = bf.file_skeleton(bf.SEED, "track/r15", 9, "all6", "zyx")
    return bvh.parse_bvh(bvh.format_bvh(fsk, bf.channels(bf.SEED, "track/r15", fsk, 9)[0]))


# ------------------------------------------------------------------------------------------ rates and the output-frame rule
def test_output_frame_rule():
    for (T, rate), count in tf.COUNTS.items():
        assert int(pt.out_frames(T, rate)) == count
        i, t = tf.frame_params(T, rate)
        assert len(i) == count and (i + 1 <= T - 1).all() and (t >= 0).all() and (t < 1).all()
    assert pt.out_frames(np.array([2, 9, 1]), Fraction(5, 4)).tolist() == [1, 7, 0]
    assert pt.up_down(Fraction(5, 4)) == (4, 5)


def test_rate_parsing():
    assert pt.parse_rate(fps=24) == Fraction(6, 5)
    assert pt.parse_rate(24 / 20) == Fraction(6, 5)                       # the reference's Fraction(24 / 20) has a 16-digit numerator
    assert Fraction(24 / 20).numerator == 5404319552844595
    assert pt.parse_rate(1.25) == Fraction(5, 4) and pt.parse_rate(fps=25) == Fraction(5, 4) and pt.parse_rate(fps=30) == Fraction(3, 2)
    assert pt.parse_rate((3, 2)) == Fraction(3, 2) and pt.parse_rate(Fraction(7, 3)) == Fraction(7, 3) and pt.parse_rate(2) == 2
    assert pt.parse_rate(fps=29.97, target_fps=20) == Fraction(2997, 2000)
    assert pt.decimal_to_fraction(1.5) == Fraction(3, 2) and pt.decimal_to_fraction("1.25") == Fraction(5, 4)
    assert pt.decimal_to_fraction(0.3) == Fraction(3, 10) and pt.parse_rate("2.5") == Fraction(5, 2)
    for bad in (dict(), dict(rate=1.5, fps=30), dict(rate=0), dict(rate=-1.5), dict(rate=(3, 0)), dict(rate=(1.5, 2)), dict(rate=float("nan")),
                dict(rate=Fraction(100001, 7))):
        with pytest.raises(ValueError):
            pt.parse_rate(**bad)


# ------------------------------------------------------------------------------------------ files and the joint table
@pytest.mark.parametrize("name", list(tf.GOLDEN_FILES))
def test_readers_round_trip(tmp_path, name):
    kind, T, fps, with_trans, cut = tf.GOLDEN_FILES[name]
    tr, extra = tf.golden_track(name)
    path = str(tmp_path / f"{name}.{kind}")
    tf.write_track(path, tr, kind)
    trans_path = ""
    if cut:
        trans_path = str(tmp_path / "trans.pkl")
        tf.write_trans(trans_path, extra)
    got = pt.read_pose_track(path, trans_path, fps=fps)
    n = cut or T
    assert got.frames == n and got.fps == fps
    assert np.array_equal(got.transl, extra if cut else tr["transl"])
    assert np.allclose(got.betas, tr["shape"].mean(0), atol=1e-7) and np.asarray(got.betas).shape == (10,)
    if kind == "pkl":
        assert got.matrices is None and got.joints is None and np.array_equal(got.rotations, tr["quats"])
    else:
        assert got.rotations is None and np.array_equal(got.matrices, tr["mats"][:n]) and np.array_equal(got.joints, tr["joints"][:n])
    case = tf.as_case(got)
    assert set(case) == ({"transl", "betas", "quats"} if kind == "pkl" else {"transl", "betas", "mats", "joints"})


def test_reader_cuts_the_longer_translation_and_refuses_other_suffixes(tmp_path):
    tr, _ = tf.golden_track("pk25")
    path = str(tmp_path / "a.pk")
    tf.write_track(path, tr, "pk")
    tf.write_trans(str(tmp_path / "long.pkl"), np.zeros((12, 3)))
    got = pt.read_pose_track(path, str(tmp_path / "long.pkl"))
    assert got.frames == 9 and got.transl.shape == (9, 3) and got.joints.shape == (9, 24, 3)
    with pytest.raises(ValueError, match="'pt', 'pk', 'pkl'"):
        pt.read_pose_track(str(tmp_path / "a.npz"))
    assert "TRUSTED" in pt.read_pose_track.__doc__


def test_body_joints(tmp_path):
    body = tf.body()
    np.savez(tmp_path / "model.npz", **body)
    bj = pt.BodyJoints.from_npz(tmp_path / "model.npz")
    assert np.array_equal(bj.J0, TABLE[0]) and np.array_equal(bj.Jdirs, TABLE[1]) and bj.parents.tolist() == tf.PARENTS22
    six = pt.BodyJoints.from_npz(tmp_path / "model.npz", num_betas=6)
    assert np.array_equal(six.Jdirs[..., :6], TABLE[1][..., :6]) and not six.Jdirs[..., 6:].any()
    import smpl_fixture as sf
    from mst_amd.model.smpl import SMPLBody
    whole = sf.synthetic_body(40)
    shared = pt.BodyJoints.from_body(SMPLBody.from_arrays(**whole))
    direct = pt.BodyJoints(whole["v_template"], whole["shapedirs"], whole["J_regressor"], whole["parents"])
    assert np.array_equal(shared.J0, direct.J0) and np.array_equal(shared.Jdirs, direct.Jdirs) and shared.parents.tolist() == tf.PARENTS22
    # an SMPL-H body: 52 joints, the same first 22
    g = np.random.default_rng(1)
    more = g.uniform(0, 1, (28, 40))
    h = dict(body, J_regressor=np.concatenate([body["J_regressor"][:24], more / more.sum(1, keepdims=True)]),
             kintree_table=np.stack([np.array([2 ** 32 - 1] + tf.SMPL_PARENTS[1:] + [20] * 28, np.int64), np.arange(52)]))
    np.savez(tmp_path / "smplh.npz", **h)
    assert np.array_equal(pt.BodyJoints.from_npz(tmp_path / "smplh.npz").J0, TABLE[0])
    for key, bad, err in (("v_template", body["v_template"][:, :2], "v_template"), ("shapedirs", body["shapedirs"][..., :4], "shapedirs"),
                          ("J_regressor", body["J_regressor"][:20], "J_regressor"), ("J_regressor", body["J_regressor"] * 1.01, "sums to 1"),
                          ("v_template", np.where(np.arange(40)[:, None] == 3, np.nan, body["v_template"]), "not finite")):
        np.savez(tmp_path / "bad.npz", **dict(body, **{key: bad}))
        with pytest.raises(ValueError, match=err):
            pt.BodyJoints.from_npz(tmp_path / "bad.npz")
    kin = body["kintree_table"].copy()
    kin[0, 5] = 7
    np.savez(tmp_path / "bad.npz", **dict(body, kintree_table=kin))
    with pytest.raises(ValueError, match="earlier joint"):
        pt.BodyJoints.from_npz(tmp_path / "bad.npz")
    np.savez(tmp_path / "bad.npz", v_template=body["v_template"])
    with pytest.raises(KeyError, match="shapedirs"):
        pt.BodyJoints.from_npz(tmp_path / "bad.npz")
    with pytest.raises(ValueError, match="num_betas"):
        pt.BodyJoints.from_npz(tmp_path / "model.npz", num_betas=11)


# ------------------------------------------------------------------------------------------ argument checks, no GPU
def test_python_argument_checks_raise_on_the_host():
    q, p = torch.zeros(2, 5, 3, 4), torch.zeros(2, 5, 3, 3)
    for kw, err in ((dict(rotations=None, points=None, rate=1.5), ValueError), (dict(rotations=q, rate=None), ValueError),
                    (dict(rotations=q[0], rate=1.5), ValueError), (dict(rotations=q.numpy(), rate=1.5), TypeError),
                    (dict(rotations=q, points=p[:, :4], rate=1.5), ValueError), (dict(rotations=q[:, :1], rate=1.5), ValueError),
                    (dict(points=torch.zeros(2, 5, 3, 4), rate=1.5), ValueError), (dict(rotations=q, rate=1.5, lengths=[5]), ValueError),
                    (dict(rotations=q, rate=1.5, lengths=[5, 1]), ValueError), (dict(rotations=q, rate=1.5, lengths=[5, 6]), ValueError),
                    (dict(rotations=q, rate=1.5), RuntimeError)):                  # a CPU tensor: there is no CPU path
        with pytest.raises(err):
            pt.resample_tracks(**kw)
    body = pt.BodyJoints(TABLE[0], TABLE[1], np.eye(22), tf.PARENTS22)          # the table itself: one vertex per joint
    rot, tr, be = torch.zeros(2, 5, 24, 4), torch.zeros(2, 5, 3), torch.zeros(2, 10)
    r = Fraction(5, 4)
    for args, kw, err in (((rot, tr, be, object()), dict(rate=r), TypeError), ((rot, tr, be, body), dict(rate=1.25), TypeError),
                          ((rot[:, :, :21], tr, be, body), dict(rate=r), ValueError), ((rot[..., :3], tr, be, body), dict(rate=r), ValueError),
                          ((rot[:, :1], tr[:, :1], be, body), dict(rate=r), ValueError), ((rot, None, be, body), dict(rate=r, with_trans=True), ValueError),
                          ((rot, tr[:, :4], be, body), dict(rate=r), ValueError), ((rot, tr, be[:, :9], body), dict(rate=r), ValueError),
                          ((rot, tr, be, body), dict(rate=r, joints=torch.zeros(2, 5, 21, 3)), ValueError),
                          ((rot, tr, be, body), dict(rate=r, lengths=[1, 5]), ValueError), ((rot, tr, be, body), dict(rate=r), RuntimeError)):
        with pytest.raises(err):
            pt.track_joints_batch(*args, **kw)
    one = tf.track(1, 4)
    good = pt.PoseTrack(one["transl"], one["betas"], rotations=one["quats"], joints=one["joints"], fps=30)
    mat = pt.PoseTrack(one["transl"], one["betas"], matrices=tf.q2rotm(one["quats"]), joints=one["joints"], fps=25)
    for tracks, kw, err in (([], {}, ValueError), ([good, object()], {}, TypeError), ([good, mat], dict(fps=30), ValueError),
                            ([good, mat], {}, ValueError),                             # two stated frame rates
                            ([pt.PoseTrack(one["transl"], one["betas"])], {}, ValueError),
                            ([pt.PoseTrack(one["transl"][:2], one["betas"], rotations=one["quats"])], {}, ValueError),
                            ([pt.PoseTrack(one["transl"], one["betas"], rotations=one["quats"][:, :20])], {}, ValueError),
                            ([pt.PoseTrack(one["transl"], one["betas"], rotations=one["quats"][:1])], {}, ValueError),
                            ([good], dict(lengths=[5]), ValueError), ([good], dict(device="cpu"), RuntimeError)):
        with pytest.raises(err):
            pt.track_joints(tracks, body, **kw)
    with pytest.raises(TypeError):
        pt.track_joints([good], tf.body())
    with pytest.raises(ValueError, match="source"):
        pt.track_to_features([good], body, tgt_offsets=np.zeros((22, 3)), raw_offsets=np.zeros((22, 3)), source="both")


def test_drop_in_module_loads_nothing_and_asks_for_configure(tmp_path, monkeypatch):
    monkeypatch.setattr(psh, "_state", {"body": None, "tgt_offsets": None, "raw_offsets": None, "chains": pt.T2M_CHAINS})
    for name in ("downsample", "joints_downsample", "amass_to_pose", "pos2hmlrep", "configure"):
        assert callable(getattr(psh, name))
    assert psh.ex_fps == 20
    with pytest.raises(RuntimeError, match="configure"):
        psh.amass_to_pose(str(tmp_path / "x.pk"))
    with pytest.raises(RuntimeError, match="configure"):
        psh.pos2hmlrep(np.zeros((4, 22, 3), np.float32))
    with pytest.raises(ValueError, match="tgt_offsets"):
        psh.configure(tgt_offsets=np.zeros((21, 3)))
    with pytest.raises(TypeError):
        psh.configure(body=3)
    np.savez(tmp_path / "model.npz", **tf.body())
    psh.configure(body=str(tmp_path / "model.npz"), tgt_offsets=np.ones((22, 3)), raw_offsets=tf.human().raw)
    assert np.array_equal(psh._state["body"].J0, TABLE[0]) and psh._state["tgt_offsets"].dtype == np.float32


def test_read_bvh_resampled_checks_on_the_host(tmp_path):
    sk, ch = bvh_case()
    path = tmp_path / "one.bvh"
    path.write_text(bvh.format_bvh(sk, ch[:1]))
    with pytest.raises(ValueError, match="2 frames"):
        bvh.read_bvh_resampled(str(path), 1.5)
    with pytest.raises(ValueError):
        bvh.read_bvh_resampled(str(path), -1.5)
    with pytest.raises(NotImplementedError, match="fractional"):        # read_bvh keeps refusing; its docstring points here
        bvh.read_bvh(str(path), downsample_rate=1.5)
    assert "read_bvh_resampled" in bvh.__doc__


def test_abi_argument_checks_need_no_gpu():
    lib = _native.lib()
    ok = C.c_void_p(64)                                     # never dereferenced: every call below is refused first
    par = (C.c_int32 * 22)(*tf.PARENTS22)
    bad_par = (C.c_int32 * 22)(*([-1] + [5] * 21))

    def resample(quats=ok, points=None, batch=1, frames=5, joints=3, npoints=0, up=2, down=3, qo=C.c_void_p(128), po=None):
        return lib.mst_track_resample(quats, points, None, batch, frames, joints, npoints, up, down, 0, qo, po, None)

    def joints(rot=ok, mat=0, rj=24, transl=ok, betas=ok, est=None, ej=0, batch=1, frames=5, up=4, down=5, with_trans=0, parents=par,
               out=C.c_void_p(128), eo=None):
        return lib.mst_track_joints(rot, mat, rj, transl, betas, est, ej, None, batch, frames, up, down, 0, with_trans, ok, ok, parents, out, eo,
                                    None)

    for call, word in ((lambda: resample(batch=0), b"batch"), (lambda: resample(frames=1), b"frames"), (lambda: resample(frames=16385), b"frames"),
                       (lambda: resample(up=0), b"rate"), (lambda: resample(down=100001), b"rate"), (lambda: resample(joints=-1), b"joints"),
                       (lambda: resample(joints=0, quats=None, qo=None), b"neither"), (lambda: resample(quats=None), b"null"),
                       (lambda: resample(npoints=2), b"points"), (lambda: resample(qo=ok), b"input"),
                       (lambda: joints(batch=0), b"batch"), (lambda: joints(batch=65536), b"batch"), (lambda: joints(frames=1), b"frames"),
                       (lambda: joints(up=0), b"rate"), (lambda: joints(rj=21), b"rotations"), (lambda: joints(betas=None), b"null"),
                       (lambda: joints(transl=None, with_trans=1), b"with_trans"), (lambda: joints(est=ok), b"together"),
                       (lambda: joints(est=ok, eo=C.c_void_p(256), ej=21), b"estimator"), (lambda: joints(parents=bad_par), b"earlier"),
                       (lambda: joints(parents=(C.c_int32 * 22)(*([0] * 22))), b"parents[0]")):
        assert call() != 0
        assert word in lib.mst_last_error(), (word, lib.mst_last_error())
    assert lib.mst_track_max_frames(22) == 16384 and lib.mst_track_max_frames(0) == -1 and lib.mst_track_max_frames(4097) == -1
    assert pt.max_frames() == 16384
