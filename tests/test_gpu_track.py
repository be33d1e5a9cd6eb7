"""k_track_resample and k_track_joints (csrc/mst_track.h) on the GPU against tests/track_fixture.py's float64 restatement, and the layers
above them: utils/pose_track.py, the drop-in names of utils/process_smpl_from_hybrik.py against tests/golden/track.npz, `read_bvh_resampled`.

The bar is the suite's: per output array of a case, max |kernel - float64| over the largest magnitude of the float64 result is at most
4 x the float32 restatement's own such distance on the same inputs, floor 1e-6.  Where an output is compared with a recorded result of
the reference instead, both sides are within that bar of the float64 restatement (the reference's side is asserted by
tests/test_track_cpu.py), so they are within twice the bar of each other.  Every test prints its distances; `test_worst_fraction` prints
the largest fraction of the bar over all cases.

Measured on an MI355X: worst fraction 0.270 over 48 outputs (model joints of matrix tracks, 257 frames at 3/2: 9.7e-7 against the float32
restatement's 9.0e-7); quaternion outputs 0.04 .. 0.19, points and the estimator's joints at most 0.06, the flipped-sign cases under the
reference's formula 0.26 of a bar that their own conditioning raises to 1.0e-5; the whole file takes about 4 s."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
import bvh_fixture as bf
import track_fixture as tf
from conftest import GOLDEN
from mst_amd.utils import bvh, pose_track as pt
from mst_amd.utils import process_smpl_from_hybrik as psh
from mst_amd.utils.motion_process import encode_joints, retarget_joints

pytestmark = pytest.mark.gpu
TABLE = tf.joint_table(tf.body())
WORST = {}


def cu(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def body_joints():
    return pt.BodyJoints(TABLE[0], TABLE[1], np.eye(22), tf.PARENTS22)         # the table itself: one vertex per joint


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "track.npz")) as z:
        return {k: z[k] for k in z.files}


def check(key, got, a32, a64, dist=tf.distance):
    own, d = dist(a32, a64), dist(got, a64)
    frac = d / tf.bar(own)
    WORST[key] = frac
    print(f"{key}: kernel vs f64 {d:.3e}; restatement f32 vs f64 {own:.3e}; bar {tf.bar(own):.3e}; fraction {frac:.3f}")
    assert d <= tf.bar(own), (key, d, own)


def batch_tracks(seed, B, T, J=24, **kw):
    """B seeded tracks of T frames and mixed lengths (the full clip first, a clip of 2 second)."""
    return [tf.track(seed + 17 * b, T, J, **kw) for b in range(B)], tf.lengths(seed, B, T)


def padded(rows, K):
    out = np.zeros((len(rows), K) + rows[0].shape[1:], rows[0].dtype)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


# ------------------------------------------------------------------------------------------ k_track_resample
RESAMPLE = [  # B, T, J, P, rate, flips, shortest
    (1, 2, 1, 1, Fraction(5, 4), False, False), (3, 3, 22, 24, Fraction(3, 2), False, False), (3, 9, 24, 22, Fraction(5, 4), True, False),
    (3, 9, 24, 1, Fraction(5, 4), True, True), (3, 9, 1, 24, Fraction(1, 2), False, True), (33, 9, 22, 22, Fraction(5, 4), True, True),
    (3, 65, 24, 24, Fraction(3, 2), False, False), (3, 257, 22, 1, Fraction(3, 2), True, True), (1, 6, 24, 24, Fraction(1), False, False)]


def restate_resample(tracks, lens, rate, J, P, dtype, shortest):
    K = tf.out_frames(len(tracks[0]["transl"]), rate)
    q = padded([tf.resample_quats(t["quats"][:, :J], rate, dtype, n, shortest) for t, n in zip(tracks, lens)], K)
    p = padded([tf.resample_points(t["joints"][:, :P], rate, dtype, n) for t, n in zip(tracks, lens)], K)
    return q, p


@pytest.mark.parametrize("B,T,J,P,rate,flips,shortest", RESAMPLE)
def test_resample_against_float64(B, T, J, P, rate, flips, shortest):
    tracks, lens = batch_tracks(100 + T, B, T, flips=flips)
    q = np.stack([t["quats"][:, :J] for t in tracks])
    p = np.stack([t["joints"][:, :P] for t in tracks])
    qo, po, out_len = pt.resample_tracks(cu(q), cu(p), rate=rate, lengths=lens, shortest=shortest)
    qo, po = qo.cpu().numpy(), po.cpu().numpy()
    K = tf.out_frames(T, rate)
    assert qo.shape == (B, K, J, 4) and po.shape == (B, K, P, 3)
    assert out_len.cpu().tolist() == [tf.out_frames(n, rate) for n in lens]
    for b, n in enumerate(out_len.cpu().tolist()):
        assert not qo[b, n:].any() and not po[b, n:].any()             # rows behind the output length: exact zeros
    (q32, p32), (q64, p64) = (restate_resample(tracks, lens, rate, J, P, dt, shortest) for dt in (np.float32, np.float64))
    key = f"resample B{B} T{T} J{J} P{P} {rate} flips={int(flips)} shortest={int(shortest)}"
    check(key + " quats", qo, q32, q64)
    check(key + " points", po, p32, p64)
    if flips and shortest:                                               # the rotations are those of the unflipped track
        plain, _ = batch_tracks(100 + T, B, T, flips=False)
        want = restate_resample(plain, lens, rate, J, P, np.float64, True)[0]
        assert tf.quat_distance(qo, want) <= tf.bar(tf.quat_distance(q32, q64))


def test_resample_without_one_of_the_tracks_and_only_points():
    tracks, lens = batch_tracks(7, 3, 9)
    q, p = np.stack([t["quats"] for t in tracks]), np.stack([t["joints"] for t in tracks])
    both = pt.resample_tracks(cu(q), cu(p), fps=25, lengths=lens)
    only_q = pt.resample_tracks(cu(q), None, fps=25, lengths=lens)
    only_p = pt.resample_tracks(None, cu(p), rate=(5, 4), lengths=lens)
    assert only_q[1] is None and only_p[0] is None
    assert torch.equal(both[0], only_q[0]) and torch.equal(both[1], only_p[1]) and torch.equal(both[2], only_p[2])


def test_equal_ends_and_a_half_turn():
    """Joint 0: both ends of every interval equal bit for bit (qpow's 10e-10 guard: the end itself comes back).  Joint 1: identity to a
    half turn about x, a relative quaternion with w = 0 exactly (theta0 = pi / 2, no sign decision under `shortest`).  Joint 2: free."""
    tr = tf.track(3, 4, 3)
    q = tr["quats"].copy()
    q[:, 0] = q[0, 0]
    q[:, 1] = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0]], np.float32)
    for shortest in (False, True):
        got = pt.resample_tracks(cu(q[None]), rate=Fraction(5, 4), shortest=shortest)[0][0].cpu().numpy()
        assert np.isfinite(got).all()
        q32, q64 = (tf.resample_quats(q, Fraction(5, 4), dt, shortest=shortest) for dt in (np.float32, np.float64))
        check(f"equal ends and half turn shortest={int(shortest)}", got, q32, q64)
        unit = q[0, 0].astype(np.float64) / np.linalg.norm(q[0, 0].astype(np.float64))
        assert np.abs(got[:, 0] - unit).max() < 2e-7
        k = 2                                                              # output frame 2: interval 2 (identity -> half turn) at t = 1/2
        assert np.abs(got[k, 1] - np.array([np.cos(np.pi / 4), np.sin(np.pi / 4), 0, 0])).max() < 2e-7


# ------------------------------------------------------------------------------------------ k_track_joints
JOINTS = [  # B, T, rot joints, rate, matrices, flips, shortest, with_trans, estimator
    (1, 2, 24, Fraction(5, 4), False, False, False, False, False), (3, 3, 22, Fraction(3, 2), False, False, False, True, True),
    (3, 9, 24, Fraction(5, 4), False, True, False, True, True), (3, 9, 24, Fraction(5, 4), False, True, True, False, True),
    (3, 9, 24, Fraction(1, 2), True, False, False, True, False), (33, 9, 24, Fraction(5, 4), True, False, False, True, True),
    (3, 65, 52, Fraction(3, 2), False, False, False, True, True), (3, 257, 24, Fraction(3, 2), True, False, False, False, True)]


def restate_joints(tracks, lens, rate, dtype, with_trans, shortest):
    K = tf.out_frames(len(tracks[0]["transl"]), rate)
    res = [tf.track_joints(t, TABLE, rate, dtype, with_trans, n, shortest) for t, n in zip(tracks, lens)]
    return padded([r[0] for r in res], K), (padded([r[1] for r in res], K) if res[0][1] is not None else None)


def launch_joints(tracks, lens, rate, with_trans, shortest, stream=None):
    key = "mats" if "mats" in tracks[0] else "quats"
    rot = cu(np.stack([t[key] for t in tracks]))
    tr, be = cu(np.stack([t["transl"] for t in tracks])), cu(np.stack([t["betas"] for t in tracks]))
    ej = cu(np.stack([t["joints"] for t in tracks])) if "joints" in tracks[0] else None
    ld = None if lens is None else cu(lens, torch.int32)
    if stream is None:
        return pt.track_joints_batch(rot, tr, be, body_joints(), rate=rate, joints=ej, with_trans=with_trans, lengths=ld, shortest=shortest)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        out = pt.track_joints_batch(rot, tr, be, body_joints(), rate=rate, joints=ej, with_trans=with_trans, lengths=ld, shortest=shortest)
    stream.synchronize()
    return out


@pytest.mark.parametrize("B,T,Jr,rate,matrices,flips,shortest,with_trans,estimator", JOINTS)
def test_track_joints_against_float64(B, T, Jr, rate, matrices, flips, shortest, with_trans, estimator):
    tracks, lens = batch_tracks(200 + T, B, T, Jr, flips=flips, matrices=matrices, estimator=estimator)
    model, est, out_len = launch_joints(tracks, lens, rate, with_trans, shortest)
    model = model.cpu().numpy()
    K = tf.out_frames(T, rate)
    assert model.shape == (B, K, 22, 3) and (est is None) == (not estimator)
    assert out_len.cpu().tolist() == [tf.out_frames(n, rate) for n in lens]
    (m32, e32), (m64, e64) = (restate_joints(tracks, lens, rate, dt, with_trans, shortest) for dt in (np.float32, np.float64))
    key = f"joints B{B} T{T} Jr{Jr} {rate} mats={int(matrices)} flips={int(flips)} shortest={int(shortest)} trans={int(with_trans)}"
    check(key + " model", model, m32, m64)
    for b, n in enumerate(out_len.cpu().tolist()):
        assert not model[b, n:].any()
    if estimator:
        est = est.cpu().numpy()
        check(key + " estimator", est, e32, e64)
        for b, n in enumerate(out_len.cpu().tolist()):
            assert not est[b, n:].any()


def test_matrix_input_does_not_depend_on_a_quaternions_sign():
    """The same rotations as matrices, as quaternions and as quaternions with flipped signs under `shortest`: one set of joints."""
    tracks, lens = batch_tracks(31, 3, 9, flips=True)
    mats = [dict(t, mats=tf.q2rotm(t["quats"].astype(np.float64)).astype(np.float32)) for t in tracks]
    for t in mats:
        del t["quats"]
    rate = Fraction(5, 4)
    a = launch_joints(tracks, lens, rate, True, True)[0].cpu().numpy()
    b = launch_joints(mats, lens, rate, True, False)[0].cpu().numpy()
    m32, m64 = (restate_joints(mats, lens, rate, dt, True, False)[0] for dt in (np.float32, np.float64))
    check("matrices of flipped quaternions", b, m32, m64)
    q32, q64 = (restate_joints(tracks, lens, rate, dt, True, True)[0] for dt in (np.float32, np.float64))
    check("flipped quaternions under shortest", a, q32, q64)
    # one motion: the two float64 statements differ by the matrices' rounding to float32 alone -- 2^-24 an entry, at most 9 joints deep
    # in a chain of bones below 1 in length, against joints of magnitude 3: a few 1e-7; ten times that is allowed
    assert tf.distance(q64, m64) < 3e-6
    assert tf.distance(a, b) <= tf.bar(tf.distance(q32, q64)) + tf.bar(tf.distance(m32, m64)) + 3e-6


# ------------------------------------------------------------------------------------------ a clip's bits
def test_a_clips_bits_do_not_depend_on_its_company():
    """Alone, at either end of a batch of 33, on a side stream, with NaN in every other clip and behind its own length."""
    rate, L = Fraction(5, 4), 7
    tracks, lens = batch_tracks(41, 33, 9)
    mine = tf.track(999, 9)
    K = tf.out_frames(L, rate)
    alone = dict((k, v[:L] if v.ndim > 1 and len(v) == 9 else v) for k, v in mine.items())
    ref_m, ref_e, n = launch_joints([alone], None, rate, True, False)
    assert n.cpu().tolist() == [K]
    rq, rp, _ = pt.resample_tracks(cu(alone["quats"][None]), cu(alone["joints"][None]), rate=rate)
    side = torch.cuda.Stream()
    for slot in (0, 32):
        for poison in (False, True):
            batch = [dict(t) for t in tracks]
            batch[slot] = {k: v.copy() for k, v in mine.items()}
            ln = lens.copy()
            ln[slot] = L
            if poison:
                for b, t in enumerate(batch):
                    for k in ("quats", "transl", "joints"):
                        if b != slot:
                            t[k] = np.full_like(t[k], np.nan)
                        else:
                            t[k][L:] = np.nan
            for stream in (None, side):
                m, e, out_len = launch_joints(batch, ln, rate, True, False, stream)
                assert out_len.cpu().tolist()[slot] == K
                assert torch.equal(m[slot, :K], ref_m[0]) and torch.equal(e[slot, :K], ref_e[0])
                assert not m[slot, K:].any() and not e[slot, K:].any()
            q = cu(np.stack([t["quats"] for t in batch]))
            p = cu(np.stack([t["joints"] for t in batch]))
            qo, po, _ = pt.resample_tracks(q, p, rate=rate, lengths=ln)
            assert torch.equal(qo[slot, :K], rq[0]) and torch.equal(po[slot, :K], rp[0])
            assert not qo[slot, K:].any() and not po[slot, K:].any()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                qs, ps, _ = pt.resample_tracks(q, p, rate=rate, lengths=ln)
            side.synchronize()
            assert torch.equal(qs[slot], qo[slot]) and torch.equal(ps[slot], po[slot])


# ------------------------------------------------------------------------------------------ the drop-in names
@pytest.fixture()
def configured(gold, monkeypatch):
    monkeypatch.setattr(psh, "_state", {"body": None, "tgt_offsets": None, "raw_offsets": None, "chains": pt.T2M_CHAINS})
    psh.configure(body=body_joints(), tgt_offsets=gold["hml|tgt_offsets"], raw_offsets=tf.human().raw)
    return psh


@pytest.mark.parametrize("T,rate", list(tf.COUNTS))
def test_downsample_drop_ins_against_the_reference(gold, T, rate):
    tr = tf.track(tf.SEED, T, flips=T == 9)
    key = f"ds|T{T}|{rate.numerator}_{rate.denominator}"
    rot, pos = psh.downsample(tr["quats"], tr["transl"], float(rate))
    joints = psh.joints_downsample(tr["joints"], float(rate))
    assert rot.shape == gold[key + "|rot"].shape and pos.shape == gold[key + "|pos"].shape and joints.shape == gold[key + "|joints"].shape
    own = tf.distance(tf.resample_quats(tr["quats"], rate, np.float32), tf.resample_quats(tr["quats"], rate, np.float64))
    d = tf.distance(rot, gold[key + "|rot"])
    print(f"{key}: rotations vs the reference {d:.3e}, twice the bar {2 * tf.bar(own):.3e}")
    assert d <= 2 * tf.bar(own)
    # the reference's float64 lerp and its float32 difference p1 - p0: one rounding each way
    assert tf.distance(pos, gold[key + "|pos"]) <= 2.0 ** -22 and tf.distance(joints, gold[key + "|joints"]) <= 2.0 ** -22


@pytest.mark.parametrize("name", list(tf.GOLDEN_FILES))
def test_amass_to_pose_against_the_reference(gold, configured, tmp_path, name):
    kind, T, fps, with_trans, cut = tf.GOLDEN_FILES[name]
    tr, extra = tf.golden_track(name)
    path = str(tmp_path / f"{name}.{kind}")
    tf.write_track(path, tr, kind)
    trans_path = ""
    if cut:
        trans_path = str(tmp_path / "trans.pkl")
        tf.write_trans(trans_path, extra)
    model, est = configured.amass_to_pose(path, fps=fps, trans_path=trans_path, with_trans=with_trans)
    ref = gold[f"file|{name}|model"]
    assert model.shape == ref.shape and model.dtype == np.float32
    n, rate = cut or T, Fraction(fps, 20)
    case = tf.as_case(pt.read_pose_track(path, trans_path))
    f32, f64 = (tf.track_joints(case, TABLE, rate, dt, with_trans) for dt in (np.float32, np.float64))
    check(f"amass_to_pose {name} model", model, f32[0], f64[0])
    if kind == "pkl":                                                      # quaternion input: the reference is well defined at every frame
        assert est is model
        assert tf.distance(model, ref) <= 2 * tf.bar(tf.distance(f32[0], f64[0]))
        return
    check(f"amass_to_pose {name} estimator", est, f32[1], f64[1])
    assert tf.distance(est, gold[f"file|{name}|est"]) <= 2 * tf.bar(tf.distance(f32[1], f64[1]))
    # matrix input: the frames on a source frame, with the reference's own float32 error there as the bar (tests/test_track_cpu.py)
    on = np.flatnonzero(tf.frame_params(n, rate)[1] == 0)
    ref_case = dict(case, quats=gold[f"file|{name}|rotm2q"])
    del ref_case["mats"]
    r32, r64 = (tf.track_joints(ref_case, TABLE, rate, dt, with_trans)[0][on] for dt in (np.float32, np.float64))
    own = max(tf.distance(r32, r64), tf.distance(f32[0][on], f64[0][on]))
    d = tf.distance(model[on], ref[on])
    print(f"{name}: model joints at t = 0 vs the reference {d:.3e}, twice the bar {2 * tf.bar(own):.3e}")
    assert d <= 2 * tf.bar(own)


def test_pos2hmlrep_against_the_reference(gold, configured):
    rows = configured.pos2hmlrep(gold["hml|joints"])
    assert rows.shape == gold["hml|rows"].shape == (8, 263)
    f32, f64 = (tf.hml_rows(gold["hml|joints"], gold["hml|tgt_offsets"], dt) for dt in (np.float32, np.float64))
    check("pos2hmlrep", rows, f32, f64)
    assert tf.distance(rows, gold["hml|rows"]) <= 2 * tf.bar(tf.distance(f32, f64))


def human_body():
    """A joint table whose rest pose is the fixture's standing figure in the estimator's camera axes (the re-axing stands it up)."""
    sk = tf.human()
    rest = np.zeros((22, 3))
    for j in range(1, 22):
        rest[j] = rest[tf.PARENTS22[j]] + sk.offsets[j]
    g = np.random.default_rng(5)
    return pt.BodyJoints(tf.reaxis(rest + np.array([0.0, 0.9, 0.0])), g.standard_normal((22, 3, 10)) * 1e-3, np.eye(22), tf.PARENTS22)


def gentle_track(seed, T, fps):
    """Small joint rotations over a root that drifts forward: a figure that stays upright, so that the encoder's input is a sane clip."""
    g = np.random.default_rng([seed, T])
    q = tf.random_quats(g, (1, 24), (0.02, 0.25)) * np.ones((T, 1, 1))
    for t in range(1, T):
        q[t] = tf.qmul(tf.random_quats(g, (24,), (0.005, 0.03)), q[t - 1])
    transl = np.cumsum(np.abs(g.standard_normal((T, 3))) * np.array([0.02, 0.0, 0.002]), 0)
    return pt.PoseTrack(transl.astype(np.float32), (g.standard_normal(10) * 0.3).astype(np.float32), rotations=q.astype(np.float32), fps=fps)


def test_track_to_features_is_the_composition_bit_for_bit(gold):
    body, raw, tgt = human_body(), tf.human().raw, gold["hml|tgt_offsets"]
    tracks = [gentle_track(1, 31, 30), gentle_track(2, 19, 30), gentle_track(3, 25, 30)]
    g = np.random.default_rng(9)
    mean, std = g.standard_normal(263).astype(np.float32), g.uniform(0.5, 2.0, 263).astype(np.float32)
    sample, lens = pt.track_to_features(tracks, body, tgt_offsets=tgt, raw_offsets=raw, with_trans=True, mean=mean, std=std, frames_out=24)
    model, est, out_len = pt.track_joints(tracks, body, with_trans=True)
    assert est is None and out_len.cpu().tolist() == [tf.out_frames(n, Fraction(3, 2)) for n in (31, 19, 25)]
    moved = retarget_joints(model, tgt, raw, pt.T2M_CHAINS, pt.T2M_LEGS, pt.T2M_FACE, lengths=out_len)
    want, want_len = encode_joints(moved, chains=pt.T2M_CHAINS, raw_offsets=raw, face_joint_indx=pt.T2M_FACE, fid_l=pt.T2M_FID_L,
                                   fid_r=pt.T2M_FID_R, feet_thre=0.002, mode="hml", lengths=out_len, mean=mean, std=std, frames_out=24)
    assert sample.shape == (3, 263, 1, 24) and torch.isfinite(sample).all()
    assert torch.equal(sample, want) and torch.equal(lens, want_len)
    assert lens.cpu().tolist() == [min(n - 1, 24) for n in out_len.cpu().tolist()]


def test_read_bvh_resampled_against_the_reference(gold, tmp_path):
    fsk = bf.file_skeleton(bf.SEED, "track/r15", 9, "all6", "zyx")
    path = tmp_path / "r15.bvh"
    path.write_text(bvh.format_bvh(fsk, bf.channels(bf.SEED, "track/r15", fsk, 9)[0]))
    sk, ch = bvh.parse_bvh(str(path))
    f32, f64 = bf.decode(ch, sk, np.float32), bf.decode(ch, sk, np.float64)
    rate = Fraction(3, 2)
    for key, ends, keep in (("bvh|r15", False, sk.not_end_index), ("bvh|r15e", True, list(range(sk.joints)))):
        got = bvh.read_bvh_resampled(str(path), 1.5, end_sites=ends)
        assert isinstance(got, list) and len(got) == 1
        a = got[0]
        assert a.quats.dtype == np.float32 and a.pos.dtype == np.float32 and a.end_offsets is None
        assert np.array_equal(a.offsets, gold[key + "|offsets"]) and list(a.parents) == gold[key + "|parents"].tolist()
        assert list(a.bones) == gold[key + "|bones"].tolist()
        q32, q64 = (tf.resample_quats(f["rotations"], rate, dt)[:, keep] for f, dt in ((f32, np.float32), (f64, np.float64)))
        p32, p64 = (tf.resample_points(f["local_positions"], rate, dt)[:, keep] for f, dt in ((f32, np.float32), (f64, np.float64)))
        check(key + " quats", a.quats, q32, q64)
        check(key + " pos", a.pos, p32, p64)
        assert tf.distance(a.quats, gold[key + "|quats"]) <= 2 * tf.bar(tf.distance(q32, q64))
        assert tf.distance(a.pos, gold[key + "|pos"]) <= 2 * tf.bar(tf.distance(p32, p64))
    again = bvh.read_bvh_resampled(str(path), Fraction(3, 2))[0]
    assert np.array_equal(again.quats, bvh.read_bvh_resampled(str(path), "1.5")[0].quats)


def test_worst_fraction():
    """Runs last in this file: the largest fraction of its bar any output above used (run alone: of one small case)."""
    if not WORST:
        test_equal_ends_and_a_half_turn()
    key = max(WORST, key=WORST.get)
    print(f"worst fraction of the bar over {len(WORST)} outputs: {WORST[key]:.3f} ({key})")
    assert WORST[key] <= 1.0
