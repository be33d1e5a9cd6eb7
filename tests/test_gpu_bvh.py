"""k_bvh_decode, k_quats_to_channels and k_retarget (csrc/mst_bvh.h) through mst_amd.utils.bvh and motion_process.retarget_joints: against
the reference's recorded outputs (tests/golden/bvh.npz) and against the float64 form of tests/bvh_fixture.py at the shapes where a kernel
changes path.

  decode        goldens (four files the reference wrote, two it read); own lengths in {1, 2, 63, 64, 65, 255, 256, 257, 600} (the wave edge,
                the workgroup edge, a carry across more than one round) with sign changes counted on both sides of a round's boundary;
                file joints in {2, 6, 31, the cap}; all six rotation orders in both channel layouts; End Sites; scale; B in {1, 3} with
                mixed lengths (equal to single calls, rows past a length exactly 0.0); stride in {2, 3} with every phase (equal to the
                full-rate result sliced, and to the recorded lists)
  selection     none: the recorded `Anim.quats`; one that skips intermediate joints: the fixture; the result feeds encode_joints
  channels      the recorded degrees modulo 360, 'zyx' and 'xzy', positions=True, quaternions that are not normalised, a joint order the
                writer permutes; save_bvh's file against the recorded text
  round trips   read_bvh(save_bvh(x)); fit_joints -> save_fits -> load_bvh against fit.positions
  retarget      goldens; lengths {1, 2, 64, 65}; B = 3 mixed; the J = 5 tree with a mid-tree chain; a zero-length bone; bone lengths; drop-in

Bars.  Per case the fixture is evaluated in float32 and in float64 on the same inputs; per output the kernel's distance from the float64
result may be 4 x the distance between the two, and not below 1e-6 (the rule of test_gpu_encode.py and test_gpu_joint_fit.py); positions
relative to the output's norm, degrees modulo 360 relative to 180.  Sign decisions, lengths, padded rows, hierarchy text and joint orders
are exact.  Every case prints `bvh: <case> <output> ref <dev> got <dev> bar <bar>`.  Operands sit in front of a NaN-filled guard and are
asserted unmodified.  Every input passes bvh_fixture.assert_clear.
Worst figures measured on an MI355X, fp32 fixture / kernel / bar (the table is in DESIGN.md section 5): decode of the goldens 2.3e-7 /
2.5e-7 / 1.0e-6, at the length edges 3.6e-7 / 3.8e-7 / 1.4e-6, the joint counts 2.8e-7 / 2.8e-7 / 1.1e-6, the six orders 3.6e-7 / 3.4e-7 /
1.5e-6, the selection 3.2e-7 / 3.0e-7 / 1.3e-6; degrees (over 180) 4.5e-7 / 4.1e-7 / 1.8e-6; retarget 1.5e-7 / 1.5e-7 / 1.0e-6; the fit's
files 9.7e-8 / 1.3e-7 / 1.0e-6 and 1.7e-6 m from fit.positions (bound 5e-5); read_bvh(save_bvh(x)) 7.2e-7 (bound 4e-6).  The kernel
comes no closer to a bar than 0.26 of it; the file takes 3 s."""
import os

import numpy as np
import pytest
import torch

import bvh_fixture as bf
import ik_fixture as ik
import mst_amd  # noqa: F401
from conftest import GOLDEN, SEED
from mst_amd.utils import bvh
from mst_amd.utils import joint_fit as jf
from mst_amd.utils import motion_process as mp

pytestmark = pytest.mark.gpu
GUARD = 4096
DECODED = ("rotations", "positions", "local_positions", "global_rotations")


def dev():
    return torch.device("cuda:0")


def guarded(values, dtype=torch.float32):
    """`values` on the GPU as a view of a buffer whose next GUARD elements are NaN."""
    v = torch.from_numpy(np.ascontiguousarray(values)).to(dtype)
    buf = torch.full((v.numel() + GUARD,), float("nan"), dtype=dtype, device=dev())
    buf[:v.numel()] = v.reshape(-1).to(dev())
    return buf[:v.numel()].view(v.shape)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "bvh.npz"))


def check(case, name, got, f32, f64, scale=None):
    """The suite's rule.  scale: compare absolute differences modulo 360 over it (degrees) instead of norms."""
    if scale is None:
        own, dev_ = bf.rel(f32, f64), bf.rel(got, f64)
    else:
        wrap = lambda a: np.abs((np.asarray(a, np.float64) + 180) % 360 - 180).max() / scale
        own, dev_ = wrap(f32 - f64), wrap(got - f64)
    print(f"bvh: {case} {name} ref {own:.3e} got {dev_:.3e} bar {bf.bar(own):.3e}")
    assert np.isfinite(got).all() and dev_ <= bf.bar(own), (case, name, dev_, own)
    return bf.bar(own)


def gpu_decode(ch, sk, lengths=None, **kw):
    c = guarded(ch)
    m = bvh.decode_channels(c, sk, lengths, return_local=True, return_global=True, **kw)
    assert torch.equal(c.cpu(), torch.from_numpy(ch))
    return m


def run_decode(case, ch, sk, lengths=None, scale=1.0, stride=1, phase=0, joints=None):
    """[B, T, C] host channels: one call against the fixture in both precisions.  -> (BvhMotion, the float64 fixture's batch and clips)."""
    kw = dict(scale=scale, stride=stride, phase=phase, joints=joints)
    f32, _ = bf.decode_batch(ch, sk, lengths, np.float32, **kw)
    f64, clips = bf.decode_batch(ch, sk, lengths, np.float64, **kw)
    for c in clips:
        bf.assert_clear(dots=c["dots"])
    m = gpu_decode(ch, sk, lengths, scale=scale, downsample_rate=None if stride == 1 else stride, phase=phase, joints=joints)
    assert m.lengths.dtype == torch.int32 and np.array_equal(m.lengths.cpu().numpy(), f64["lengths"]), case
    for name in DECODED:
        got = getattr(m, name).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == f64[name].shape, (case, name, got.shape, f64[name].shape)
        check(case, name, got, f32[name], f64[name])
        for b, n in enumerate(f64["lengths"]):
            assert not got[b, n:].any(), (case, name, b)                  # rows past a clip: exact zeros
    rot = m.rotations.cpu().numpy()
    assert ((rot * f64["rotations"]).sum(-1)[f64["rotations"].any(-1)] > 0).all(), case          # every sign decision
    return m, f64, clips


def golden_file(gold, name):
    if name in bf.GOLDEN_WRITE:
        return bvh.parse_bvh(gold[f"{name}|text"].tobytes().decode())
    Jf, T, layout, order = bf.GOLDEN_DECODE[name]
    sk = bf.file_skeleton(SEED, name, Jf, layout, order)
    return bvh.parse_bvh(bvh.format_bvh(sk, bf.channels(SEED, name, sk, T)[0]))


# ------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("name", list(bf.GOLDEN_WRITE) + list(bf.GOLDEN_DECODE))
def test_decode_against_the_reference_outputs(gold, name):
    sk, ch = golden_file(gold, name)
    m, f64, clips = run_decode(name, ch[None], sk)
    assert (clips[0]["signs"] < 0).any()
    for out, key in (("rotations", "read_ends|quats"), ("local_positions", "read_ends|pos"), ("positions", "fk")):
        got, ref = getattr(m, out)[0].cpu().numpy(), gold[f"{name}|{key}"]
        own = bf.rel(bf.decode(ch, sk, np.float32)[out], f64[out][0])
        d = bf.rel(got, ref)
        print(f"bvh: {name} recorded {out} got {d:.3e} bar {bf.bar(own) + bf.rel(ref, f64[out][0]):.3e}")
        assert d <= bf.bar(own) + bf.rel(ref, f64[out][0]), (name, out)
    assert ((m.rotations[0].cpu().numpy() * gold[f"{name}|read_ends|quats"]).sum(-1) > 0).all()      # the reference's sign decisions


@pytest.mark.parametrize("name", ("w6", "d31"))
def test_read_bvh_returns_the_reference_anim(gold, name, tmp_path):
    sk, ch = golden_file(gold, name)
    path = tmp_path / f"{name}.bvh"
    path.write_text(bvh.format_bvh(sk, ch))
    quats = gold[f"{name}|read_ends|quats"]
    tol = bf.bar(bf.rel(bf.decode(ch, sk, np.float32)["rotations"], bf.decode(ch, sk, np.float64)["rotations"])) + 1e-7
    for ends, key in ((False, "read"), (True, "read_ends")):
        a = bvh.read_bvh(str(path), end_sites=ends)
        keep = list(range(sk.joints)) if ends else sk.not_end_index
        assert list(a.parents) == list(gold[f"{name}|{key}|parents"]) and list(a.bones) == list(gold[f"{name}|{key}|bones"])
        assert np.array_equal(a.offsets, gold[f"{name}|{key}|offsets"]) and np.array_equal(a.end_offsets, gold[f"{name}|{key}|end_offsets"])
        assert a.quats.shape == quats[:, keep].shape and bf.rel(a.quats, quats[:, keep]) <= tol
        assert np.array_equal(a.pos, gold[f"{name}|read_ends|pos"][:, keep])
    full = bvh.read_bvh(str(path))
    anims = bvh.read_bvh(str(path), downsample_rate=3)
    assert len(anims) == 3
    for i, a in enumerate(anims):
        ref = gold[f"{name}|ds3|{i}|quats"]
        assert np.array_equal(a.quats, full.quats[i::3]) and np.array_equal(a.pos, gold[f"{name}|ds3|{i}|pos"]) and a.end_offsets is None
        assert a.quats.shape == ref.shape and bf.rel(a.quats, ref) <= tol and ((a.quats * ref).sum(-1) > 0).all()
    part = bvh.read_bvh(str(path), start=3, end=20)
    assert part.quats.shape[0] == 17


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 255, 256, 257, 600))
def test_decode_at_the_wave_and_round_edges(n):
    sk = bf.file_skeleton(SEED, "edges", 6)
    ch = bf.channels(SEED, f"edges{n}", sk, n, step=4.0)
    _, _, clips = run_decode(f"len{n}", ch, sk)
    if n >= 257:                             # sign changes on both sides of the first round's boundary, and a carry into the later rounds
        s = clips[0]["signs"]
        before, after = (s[1:256] != s[:255]).sum(), (s[256:] != s[255:-1]).sum()
        assert before > 0 and (s[255] < 0).any() and (n == 257 or after > 0), (before, after)
    if n == 600:
        assert (clips[0]["signs"][512:] < 0).any() and (clips[0]["signs"][511] < 0).any()


@pytest.mark.parametrize("Jf", (2, 6, 31, 96))
def test_decode_at_every_joint_count(Jf):
    assert bvh.max_joints() == 96
    sk = bf.file_skeleton(SEED, f"count{Jf}", Jf)
    run_decode(f"Jf{Jf}", bf.channels(SEED, f"count{Jf}", sk, 70), sk)
    with pytest.raises(ValueError, match="mst_bvh_max_joints"):
        big = bf.file_skeleton(SEED, "count100", 100)
        bvh.decode_channels(torch.zeros(1, 2, big.channels, device=dev()), big)


@pytest.mark.parametrize("layout", ("root6", "all6"))
@pytest.mark.parametrize("order", bf.ORDERS)
def test_decode_in_every_rotation_order_and_layout(order, layout):
    sk = bf.file_skeleton(SEED, f"order/{order}/{layout}", 7, layout, order)
    m, f64, _ = run_decode(f"{order}/{layout}", bf.channels(SEED, f"order/{order}/{layout}", sk, 66), sk)
    ends = [j for j in range(sk.joints) if sk.is_end[j]]
    assert ends and (m.rotations[0, :, ends].cpu() == torch.tensor([1.0, 0, 0, 0])).all()              # End Sites: the identity


def test_decode_scale_applies_to_offsets_and_position_channels():
    sk = bf.file_skeleton(SEED, "scale", 9, "all6", scale=100.0)
    ch = bf.channels(SEED, "scale", sk, 40)
    m, _, _ = run_decode("scale", ch, sk, scale=0.01)
    plain = gpu_decode(ch, sk)
    assert torch.equal(m.rotations, plain.rotations) and bf.rel(m.positions.cpu().numpy() * 100, plain.positions.cpu().numpy()) < 1e-6


@pytest.mark.parametrize("stride", (1, 2, 3))
def test_decode_batch_of_mixed_lengths_equals_single_calls(stride):
    sk = bf.file_skeleton(SEED, "mixed", 10)
    T, lengths = 300, np.array([300, 1, 130])
    ch = bf.channels(SEED, "mixed", sk, T, B=3)
    full = gpu_decode(ch, sk, lengths)
    for phase in range(stride):
        m, f64, _ = run_decode(f"mixed/s{stride}p{phase}", ch, sk, lengths, stride=stride, phase=phase)
        for name in DECODED:
            got = getattr(m, name)
            assert torch.equal(got, getattr(full, name)[:, phase::stride]), (name, stride, phase)      # signs scanned at the full rate
            for b, n in enumerate(lengths):
                one = gpu_decode(ch[b:b + 1, :n], sk, downsample_rate=None if stride == 1 else stride, phase=phase) if n > phase else None
                rows = int(f64["lengths"][b])
                assert rows == (0 if one is None else getattr(one, name).shape[1])
                assert rows == 0 or torch.equal(got[b, :rows], getattr(one, name)[0]), (name, b)
                assert not got[b, rows:].any()


# ------------------------------------------------------------------------------------------ selection
def test_selection_folds_skipped_joints_and_feeds_encode_joints():
    sk = bf.file_skeleton(SEED, "select", 31)
    keep = sk.not_end_index
    inner = [j for j in keep if j and j in sk.parents]
    skipped = inner[1::6][:3]
    sel = [j for j in keep if j not in skipped][:20]
    sel = sel[:3] + sel[3:][::-1]            # the model's order is not the file's
    assert len(sel) == 20 and sel[0] == 0 and any(sk.parents[j] in skipped for j in sel)
    ch = bf.channels(SEED, "select", sk, 76)
    m, f64, _ = run_decode("select", ch, sk, joints=sel)
    assert m.joints == sel and m.rotations.shape == (1, 76, 20, 4) and m.parents[0] == -1
    by_name = gpu_decode(ch, sk, joints=[sk.names[j] for j in sel])
    assert torch.equal(by_name.rotations, m.rotations) and torch.equal(by_name.positions, m.positions)
    everything = gpu_decode(ch, sk)
    assert torch.equal(m.positions, everything.positions[:, :, sel]) and torch.equal(m.global_rotations, everything.global_rotations[:, :, sel])
    direct = [k for k, j in enumerate(sel) if sk.parents[j] < 0 or sk.parents[j] in sel]
    assert torch.equal(m.rotations[:, :, direct], everything.rotations[:, :, [sel[k] for k in direct]])     # the file's own quaternion
    # forward kinematics over the selected joints alone reproduces their global positions
    rot, lp = f64["rotations"][0], f64["local_positions"][0]
    order = sorted(range(20), key=lambda k: sel[k])
    gr, gp = {}, {}
    for k in order:
        a = m.parents[k]
        q = rot[:, k] / np.linalg.norm(rot[:, k], axis=-1, keepdims=True)
        gr[k] = q if a < 0 else bf.qmul(gr[a], q)
        gp[k] = lp[:, k] if a < 0 else bf.qrot(gr[a], lp[:, k]) + gp[a]
    assert max(np.abs(gp[k] - f64["positions"][0][:, k]).max() for k in order) < 1e-9
    sample, lengths = mp.encode_joints(m.positions, m.rotations, chains=[], raw_offsets=None, face_joint_indx=(1, 2, 3, 4), fid_l=(5, 6),
                                       fid_r=(7, 8), lengths=m.lengths)
    assert sample.shape == (1, 9 * 20 + 1, 1, 76) and int(lengths[0]) == 75


# ------------------------------------------------------------------------------------------ quaternions -> channels
def gpu_channels(q, root, parents, order, positions=None):
    tq, tr = guarded(q), guarded(root)
    tp = None if positions is None else guarded(positions)
    out = bvh.quats_to_channels(tq, tr, parents, order, tp)
    assert torch.equal(tq.cpu(), torch.from_numpy(q)) and torch.equal(tr.cpu(), torch.from_numpy(root))
    return out.cpu().numpy()


def split(ch, J, positions):
    """-> (position columns, angle columns)."""
    if positions:
        c = ch.reshape(ch.shape[:-1] + (J, 6))
        return c[..., :3], c[..., 3:]
    return ch[..., :3], ch[..., 3:]


@pytest.mark.parametrize("name", list(bf.GOLDEN_WRITE))
def test_quats_to_channels_against_the_recorded_degrees(gold, name, tmp_path):
    names, par, off, end, order, positions, q, pos = bf.writer_case(SEED, name)
    bf.assert_clear(writer=q, order=order)
    assert np.abs(np.linalg.norm(q, axis=-1) - 1).max() > 0.05           # not normalised
    f32, f64 = (bf.channels_from_quats(q, pos[:, 0], par, order, pos if positions else None, dt) for dt in (np.float32, np.float64))
    got = gpu_channels(q[None], pos[None, :, 0], par, order, pos[None] if positions else None)[0]
    J = len(par)
    assert got.shape == f64.shape == gold[f"{name}|channels"].shape
    (gp, ga), (p32, a32), (p64, a64), (rp, ra) = (split(a, J, positions) for a in (got, f32, f64, gold[f"{name}|channels"]))
    assert np.array_equal(gp, rp) and np.array_equal(gp, p32)           # positions are copied
    b = check(name, "degrees", ga, a32, a64, scale=180.0)
    wrap = lambda a: np.abs((a.astype(np.float64) + 180) % 360 - 180).max() / 180
    assert wrap(ga - ra) <= b + wrap(ra - a64), name                     # the reference's own numbers
    # save_bvh: the file the reference wrote, up to those figures and the six decimals of the text
    path = tmp_path / f"{name}.bvh"
    anim = bvh.Anim(q.copy(), pos.copy(), off.copy(), list(par), list(names), end.copy())
    bvh.save_bvh(str(path), anim, 1 / 30, order, positions)
    assert np.array_equal(anim.quats, q)
    text, ref = path.read_text(), gold[f"{name}|text"].tobytes().decode()
    assert text.split("Frame Time")[0] == ref.split("Frame Time")[0]    # hierarchy and frame count: exact
    sk, ch = bvh.parse_bvh(text)
    sp, sa = split(ch, J, positions)
    assert np.abs(sp - rp).max() <= 1e-6 and wrap(sa - ra) <= b + wrap(ra - a64) + 1e-6 / 180


def test_quats_to_channels_in_the_writers_joint_order():
    par = [-1, 0, 0, 1, 2, 1]
    seq = bvh.writer_sequence(par)
    assert seq != list(range(6))
    *_, q, pos = bf.writer_case(SEED, "w6")
    pos = pos + np.arange(6, dtype=np.float32)[None, :, None]
    for positions in (None, pos):
        f32, f64 = (bf.channels_from_quats(q, pos[:, 0], par, "zyx", positions, dt) for dt in (np.float32, np.float64))
        got = gpu_channels(np.stack([q, q[::-1]]), np.stack([pos[:, 0], pos[::-1, 0]]), par, "zyx",
                           None if positions is None else np.stack([pos, pos[::-1]]))
        assert np.array_equal(got[1], got[0][::-1])                      # B = 2: the second clip is the first reversed
        (gp, ga), (p32, a32), (p64, a64) = (split(a, 6, positions is not None) for a in (got[0], f32, f64))
        assert np.array_equal(gp, p32)
        check(f"permuted/{positions is not None}", "degrees", ga, a32, a64, scale=180.0)
    with pytest.raises(NotImplementedError, match="q2eul"):
        bvh.quats_to_channels(torch.zeros(1, 2, 6, 4, device=dev()), torch.zeros(1, 2, 3, device=dev()), par, "zxy")


# ------------------------------------------------------------------------------------------ round trips
@pytest.mark.parametrize("name", ("w6", "w31"))
def test_read_bvh_of_save_bvh_reproduces_the_quaternions(name, tmp_path):
    """Up to sign, for 'zyx' files.  (The reference's 'yzx' formula set is not the inverse of its eul2q in 'xzy' order: an 'xzy' file does
    not give its quaternions back, there as here -- the recorded degrees and the recorded read of that file pin both halves.)  The bound: per Euler angle the float32 q2eul is within 9.1e-5 degrees of float64 up to an arcsin argument of 0.99
    (bvh_fixture, measured with the reference's functions) and the text rounds to 5e-7 degrees; three angles a joint turn the quaternion
    by at most 3 * 9.2e-5 degrees = 4.8e-6 rad, half of that in its components, 2.4e-6; float32 eul2q adds a few 6e-8: 4e-6."""
    names, par, off, end, order, positions, q, pos = bf.writer_case(SEED, name)
    bf.assert_clear(writer=q, order=order)
    path = tmp_path / "a.bvh"
    bvh.save_bvh(str(path), bvh.Anim(q, pos, off, list(par), list(names), end), 1 / 30, order)
    a = bvh.read_bvh(str(path))
    assert list(a.parents) == list(par) and a.bones == list(names) and np.abs(a.offsets - off).max() <= 5.1e-7
    assert np.abs(a.end_offsets - end).max() <= 5.1e-7
    unit = q / np.linalg.norm(q, axis=-1, keepdims=True)
    d = np.minimum(np.abs(a.quats - unit).max(-1), np.abs(a.quats + unit).max(-1)).max()
    print(f"bvh: roundtrip/{name} quats got {d:.3e} bound 4.0e-06")
    assert d <= 4e-6
    assert ((a.quats[1:] * a.quats[:-1]).sum(-1) > 0).all()             # and continuous in time


def test_fit_save_fits_load_bvh_round_trip(tmp_path):
    """fit_joints -> save_fits -> load_bvh: the files' forward kinematics against fit.positions.  The fixture goes the same way in float32
    and float64 (degrees from the fitted quaternions, six decimals of text, decode); the suite's rule on that, and against fit.positions
    itself the bound of the text: nine joints deep at most, each turned by at most 4.8e-6 rad (see the test above) over bones of at
    most 1 m, and 5e-7 per offset: 5e-5 m."""
    J, T, B = 6, 12, 2
    parents, off = ik.tiny_tree(J)
    assert bvh.writer_sequence(parents) != list(range(J))
    data, target = ik.make_clip(SEED, f"bvh/fit/J{J}", T, J, parents, off, B=B)
    lengths = np.array([T, 7])
    fit = jf.fit_joints(torch.from_numpy(data).to(dev()), J, parents, off, torch.from_numpy(target).to(dev()), 5, lengths=lengths)
    quats, r_pos = fit.joint_quats.cpu().numpy(), fit.r_pos.cpu().numpy()
    bf.assert_clear(writer=quats[0], order="zyx")
    bf.assert_clear(writer=quats[1, :7], order="zyx")
    paths = [str(tmp_path / f"{b}.bvh") for b in range(B)]
    names = [f"n{j}" for j in range(J)]
    bvh.save_fits(paths, fit, off, parents, names, lengths)
    m = bvh.load_bvh(paths)
    seq = bvh.writer_sequence(parents)
    assert m.lengths.tolist() == [T, 7] and m.skeleton.simple_names == [names[j] for j in seq]
    keep = [m.skeleton.not_end_index[seq.index(j)] for j in range(J)]       # the file's joint of every fitted joint
    got = m.positions[:, :, keep].cpu().numpy()
    zero = off.copy()
    zero[0] = 0
    wsk, _ = bvh.writer_skeleton(names, parents, zero, None, "zyx", False, bvh.FIT_FRAME_TIME)
    for b, n in enumerate(lengths):
        want = []
        for dt in (np.float32, np.float64):
            ch = bf.channels_from_quats(quats[b, :n], r_pos[b, :n], parents, "zyx", None, dt)
            sk, ch = bvh.parse_bvh(bvh.format_bvh(wsk, ch))
            want.append(bf.decode(ch, sk, dt)["positions"][:, keep])
        check(f"fit/{b}", "positions", got[b, :n], want[0], want[1])
        d = np.abs(got[b, :n] - fit.positions[b, :n].cpu().numpy()).max()
        print(f"bvh: fit/{b} against fit.positions got {d:.3e} bound 5.0e-05")
        assert d <= 5e-5 and not got[b, n:].any()
    # the callable fit_joints_bvh documents: the same file as save_fits writes for a single clip
    one = str(tmp_path / "one.bvh")
    jf.fit_joints_bvh(one, data[0], J, parents, off, target[0], names=names, iter_num=5, save=bvh.save_fit)
    assert open(one).read() == open(paths[0]).read()


# ------------------------------------------------------------------------------------------ retarget
def run_retarget(case, sk, pos, tgt, l_idx, lengths=None):
    B, T = pos.shape[:2]
    n_of = lambda b: T if lengths is None else int(lengths[b])
    want = []
    for dt in (np.float32, np.float64):
        out = np.zeros(pos.shape, dt)
        for b in range(B):
            out[b, :n_of(b)], diag = bf.retarget(pos[b, :n_of(b)], tgt, sk.raw, sk.chains, l_idx, sk.face, dt)
            if dt is np.float64:
                bf.assert_clear(retarget_diag=diag)
        want.append(out)
    p = guarded(pos)
    got = mp.retarget_joints(p, tgt, sk.raw, sk.chains, l_idx, sk.face, lengths=lengths)
    assert torch.equal(p.cpu(), torch.from_numpy(pos)) and got.shape == pos.shape and got.dtype == torch.float32
    check(case, "joints", got.cpu().numpy(), want[0], want[1])
    for b in range(B):
        assert not got[b, n_of(b):].any()
    return got, want[1]


@pytest.mark.parametrize("J,T", bf.GOLDEN_RETARGET)
def test_retarget_against_the_reference_outputs(gold, J, T):
    sk, pos, tgt, l_idx = bf.retarget_case(SEED, J, T)
    got, f64 = run_retarget(f"retarget/J{J}T{T}", sk, pos, tgt, l_idx)
    ref = gold[f"retarget|J{J}T{T}"]
    f32, _ = bf.retarget(pos[0], tgt, sk.raw, sk.chains, l_idx, sk.face, np.float32)
    assert bf.rel(got[0].cpu().numpy(), ref) <= bf.bar(bf.rel(f32, f64[0])) + bf.rel(ref, f64[0])
    par = ik.parents_of(sk.chains, J)
    bones = (got[0, :, 1:] - got[0, :, par[1:]]).norm(dim=-1).cpu().numpy()
    want = np.linalg.norm(tgt[1:], axis=-1)
    assert np.abs(bones / want - 1).max() <= 1e-5                        # the target's bone lengths: a unit quaternion to 8 float32 roundings
    one = mp.uniform_skeleton_basic(pos[0], torch.from_numpy(tgt), torch.from_numpy(sk.raw), sk.chains, l_idx, sk.face)
    assert isinstance(one, np.ndarray) and np.array_equal(one, got[0].cpu().numpy())
    dropin = mp.uniform_skeleton_basic(torch.from_numpy(pos[0]).to(dev()), tgt, sk.raw, sk.chains, l_idx, sk.face)
    assert torch.equal(dropin, got[0])
    if J == 5:
        assert sk.chains[2][0] == 1          # the mid-tree chain restarts from the root quaternion
        loose = mp.retarget_joints(torch.from_numpy(pos).to(dev()), tgt, sk.raw, sk.chains[:2], l_idx, sk.face)
        assert not loose[:, :, 4].any() and torch.equal(loose[:, :, :4], got[:, :, :4])      # a joint no chain names: zeros, as np.zeros leaves it


@pytest.mark.parametrize("n", (1, 2, 64, 65))
def test_retarget_at_the_wave_edges(n):
    sk, pos, tgt, l_idx = bf.retarget_case(SEED, 22, 65)
    run_retarget(f"retarget/len{n}", sk, pos[:, :n], tgt, l_idx)


def test_retarget_batch_of_mixed_lengths_equals_single_calls():
    lengths = np.array([65, 1, 300])
    sk, pos, tgt, l_idx = bf.retarget_case(SEED, 22, 300, B=3, lengths=lengths)
    got, _ = run_retarget("retarget/mixed", sk, pos, tgt, l_idx, lengths)
    for b, n in enumerate(lengths):
        one = mp.retarget_joints(torch.from_numpy(pos[b:b + 1, :n]).to(dev()), tgt, sk.raw, sk.chains, l_idx, sk.face)
        assert torch.equal(one[0], got[b, :n])


def test_retarget_zero_length_bone_gives_nan_where_the_reference_has_it():
    sk, pos, tgt, l_idx = bf.retarget_case(SEED, 5, 24)
    pos = pos.copy()
    pos[:, 3:7, 2] = pos[:, 3:7, 1]          # joint 2 on its parent, joint 1, in four frames
    with np.errstate(all="ignore"):
        want, _ = bf.retarget(pos[0], tgt, sk.raw, sk.chains, l_idx, sk.face, np.float64)
    got = mp.retarget_joints(torch.from_numpy(pos).to(dev()), tgt, sk.raw, sk.chains, l_idx, sk.face)[0].cpu().numpy()
    assert np.isnan(want).any() and np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.abs(got[ok] - want[ok]).max() <= 1e-5
