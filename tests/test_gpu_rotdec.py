"""The rotation-channel decoders on the GPU (utils/rot_decode.py, csrc/mst_rotdec.h) against the float64 fixture (tests/rotdec_fixture.py).

The bar: per case and output, max error over the output's largest magnitude (quaternions up to sign) at most 4 x the reference's own
float32-to-float64 distance for that case and output, read from tests/golden/rotdec.npz, floor 1e-6 (the floor of the BVH tests).  The
factor covers the scan's other summation order and device sincos / acos against libm.  Every case prints
`rotdec: <case> <output> ref <dist> got <dist> bar <bar> ratio <got / bar>`.

Exact: the theta = 0 joint, zeros past every length, a batch against single-clip calls, the samplers' layout against rows, every
optional output against the call that asks for it alone, the drop-ins against the batched call, a side stream against the default one,
the HIERARCHY text of the written files against the reference's.

Measured on an MI355X (reference fp32 / kernel / bar, worst per output): hml_rot quats 3.6e-7 / 5.4e-7 / 1.4e-6 (0.38 of the bar, the
closest approach), joints 1.9e-7 / 2.2e-7 / 1.0e-6, root 6.7e-8 / 7.7e-8 / 1.0e-6; real_rot quats 2.2e-7 / 2.2e-7 / 1.0e-6, joints 1.9e-7 /
2.2e-7 / 1.0e-6, local rows 3.7e-7 / 3.5e-7 / 1.5e-6, root 1.4e-7 / 1.1e-7 / 1.0e-6; at 4096 frames no output is above 0.25 of its bar.
Files read back within 5.2e-7 (bound 4e-6), no frame-joint left out.  Consistency: rot 2.1e-7, ric 8.5e-8, rot against ric
1.7e-7 (each against the one bar 1e-6); with one block rolled 0.79.  Fit round trip: 2.9e-7 against the fixture, 3.3e-7 against
fit.positions (bar 1e-6).  pos_ik: quats 3.8e-6 / 4.1e-6 / 1.5e-5 (0.27), at 4096 frames 8.6e-6 / 8.8e-6 / 3.5e-5; joints and root below
0.1 of the floor.  The file takes 5 s."""
import os

import numpy as np
import pytest
import torch

import bvh_fixture as bf
import encode_fixture as ef
import mst_amd  # noqa: F401
import rotdec_fixture as rf
from conftest import GOLDEN, SEED
from mst_amd.utils import bvh
from mst_amd.utils import motion_process as mp
from mst_amd.utils import rot_decode as rd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "rotdec.npz"))


def dev():
    return torch.device("cuda")


def cu(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=dev(), dtype=dtype)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def decode(route, name, data, lengths=None, **kw):
    """-> dict of numpy outputs, every one asked for."""
    J, chains, off = rf.tree(name)
    x = data if torch.is_tensor(data) else cu(data)
    want_local = route == rf.REAL
    if route == rf.POS:
        kw = dict(kw, raw_offsets=rf.raw_of(off), face_joint_indx=rf.face_of(J))
    res = rd.decode_rotations(x, J, chains, off, route=route, lengths=lengths, joints=True, local=want_local, **kw)
    out = dict(quats=host(res[0].quats), root_pos=host(res[0].root_pos), joints=host(res[1]), anim=res[0])
    if want_local:
        out["local"] = host(res[2])
    return out


def check(gold, key, got, f64, route):
    worst = 0.0
    for k in rf.OUTPUTS[route]:
        own = float(gold[f"dist|{key}|{k}"])
        e, b = rf.distance(k, got[k], f64[k]), rf.bar(own)
        print(f"rotdec: {key} {k} ref {own:.3e} got {e:.3e} bar {b:.3e} ratio {e / b:.2f}")
        assert got[k].shape == f64[k].shape and got[k].dtype == np.float32
        assert e <= b, (key, k, e, b)
        worst = max(worst, e / b)
    gap = rf.quat_gap(got["quats"], f64["quats"])
    assert gap <= rf.bar(float(gold[f"dist|{key}|quats"])), (key, gap)
    return worst


def exact_parts(route, name, got, lengths, T):
    J, chains, _ = rf.tree(name)
    for b, n in enumerate(lengths):
        for k in rf.OUTPUTS[route]:
            assert not got[k][b, n:].any(), (name, k, b)                          # exactly 0.0 past the clip
            assert np.isfinite(got[k][b, :n]).all()
        if route == rf.REAL:
            assert (got["quats"][b, :n, rf.identity_joint(chains)] == np.array([1, 0, 0, 0], np.float32)).all()
        elif route == rf.HML:
            for i in rf.identity_carriers(name):
                assert (got["quats"][b, :n, i, 1:] == 0).all()


@pytest.mark.parametrize("route", rf.ROUTES)
@pytest.mark.parametrize("T", rf.FRAMES)
def test_every_tree_at_the_scan_edges(gold, route, T):
    lengths = rf.lengths_of(T)
    for name in rf.TREES:
        J, chains, off = rf.tree(name)
        data = rf.make_rows(name, route, T)
        f64 = rf.decode_batch(route, data, J, chains, off, lengths, np.float64)
        got = decode(route, name, data, lengths)
        check(gold, f"{route}|{name}|T{T}", got, f64, route)
        exact_parts(route, name, got, lengths, T)
        # a batch equals single-clip calls bit for bit, at each clip's own frame count
        for b, n in enumerate(lengths):
            one = decode(route, name, data[b:b + 1, :n])
            for k in rf.OUTPUTS[route]:
                assert np.array_equal(one[k][0], got[k][b, :n]), (name, k, b)
        # the samplers' layout equals the row layout bit for bit; with mean / std it equals the rows the kernel denormalises to
        x = cu(data)
        sampler = x.permute(0, 2, 1)[:, :, None, :].contiguous()
        same = decode(route, name, sampler, lengths)
        F = data.shape[-1]
        mean = (0.1 * np.sin(np.arange(F))).astype(np.float32)
        std = (0.5 + 0.25 * np.cos(np.arange(F)) ** 2).astype(np.float32)
        norm = ((data - mean) / std).astype(np.float32)
        den = (norm * std + mean).astype(np.float32)              # fp32 multiply, then fp32 add: what the kernel forms
        fused = decode(route, name, cu(norm).permute(0, 2, 1)[:, :, None, :].contiguous(), lengths, mean=mean, std=std)
        rows = decode(route, name, den, lengths)
        strided = decode(route, name, cu(np.concatenate([data, data], -1))[..., :F], lengths)       # rows with a frame stride of 2 F
        for k in rf.OUTPUTS[route]:
            assert np.array_equal(same[k], got[k]), (name, k)
            assert np.array_equal(fused[k], rows[k]), (name, k)
            assert np.array_equal(strided[k], got[k]), (name, k)


@pytest.mark.parametrize("route,name", ((rf.HML, "t2m22"), (rf.REAL, "mid21"), (rf.POS, "t2m22")))
def test_a_4096_frame_clip(gold, route, name):
    """The scan's accumulated error over the longest clip the entry takes."""
    T = rf.LONG
    assert T == rd.max_frames(22)
    J, chains, off = rf.tree(name)
    lengths = rf.lengths_of(T)
    data = rf.make_rows(name, route, T)
    f64 = rf.decode_batch(route, data, J, chains, off, lengths, np.float64)
    got = decode(route, name, data, lengths)
    check(gold, f"{route}|{name}|T{T}", got, f64, route)
    exact_parts(route, name, got, lengths, T)
    with pytest.raises(RuntimeError, match=r"4097 frames > 4096.*mst_rot_decode_max_frames"):
        decode(route, name, torch.zeros(1, T + 1, data.shape[-1], device=dev()))


class Skel:
    def __init__(self, name):
        J, chains, off = rf.tree(name)
        self._kinematic_tree, self._offset, self._parents = chains, torch.from_numpy(off), rf.chain_parents(chains, J)


@pytest.mark.parametrize("route", rf.ROUTES)
def test_optional_outputs_and_drop_ins(gold, route, tmp_path):
    name, T = "t2m22" if route != rf.REAL else "mid21", 65
    J, chains, off = rf.tree(name)
    lengths = rf.lengths_of(T)
    data = rf.make_rows(name, route, T)
    x = cu(data)
    full = decode(route, name, x, lengths)
    ik = dict(raw_offsets=rf.raw_of(off), face_joint_indx=rf.face_of(J)) if route == rf.POS else {}
    dec = lambda **kw: rd.decode_rotations(x, J, chains, off, route=route, lengths=lengths, **ik, **kw)
    # lengths on the device are used as they are (no copy back); out-of-range values are clamped into 1 .. T by the kernel
    on_dev = decode(route, name, x, torch.tensor(lengths, dtype=torch.int32, device=dev()))
    clamped = decode(route, name, x, torch.tensor([T + 5, 0, lengths[2]], dtype=torch.int64, device=dev()))
    for k in rf.OUTPUTS[route]:
        assert np.array_equal(on_dev[k], full[k]) and np.array_equal(clamped[k], full[k]), k
    only_q = dec(root_pos=False)
    assert only_q.root_pos is None and np.array_equal(host(only_q.quats), full["quats"])
    only_r = dec(quats=False)
    assert only_r.quats is None and np.array_equal(host(only_r.root_pos), full["root_pos"])
    anim, jp = dec(joints=True, quats=False, root_pos=False)
    assert anim.quats is None and anim.root_pos is None and np.array_equal(host(jp), full["joints"])
    assert anim.parents == full["anim"].parents and np.array_equal(anim.offsets, full["anim"].offsets)
    if route == rf.REAL:
        _, lo = dec(local=True, quats=False, root_pos=False)
        assert np.array_equal(host(lo), full["local"])
    # the drop-ins: the reference's signatures on one clip
    sk = Skel(name)
    rows = x[0]
    if route == rf.HML:
        assert np.array_equal(host(rd.recover_from_rot(rows, J, sk)), full["joints"][0])
        assert np.array_equal(host(rd.recover_from_rot(data[0], J, sk)), full["joints"][0])           # numpy in: uploaded
        a = rd.output_bvh(str(tmp_path / "a.bvh"), rows, J, chains, torch.from_numpy(off))
    elif route == rf.POS:
        names = [f"b{i}" for i in range(J + len(chains))]
        a = rd.output_bvh_with_pos(str(tmp_path / "a.bvh"), rows, J, chains, torch.from_numpy(off), torch.from_numpy(rf.raw_of(off)),
                                   rf.face_of(J), bone_names=names)
        assert "JOINT b26\n" in open(tmp_path / "a.bvh").read()
        # the route's joints are recover_from_ric's: the older kernel sums the root serially in float32, this one in double -- the floor
        assert rf.relmax(host(mp.recover_from_ric(rows, J)), full["joints"][0]) <= rf.FLOOR
    else:
        assert np.array_equal(host(rd.recover_from_real_rot(rows, J, sk)), full["joints"][0])
        assert np.array_equal(host(rd.recover_from_real_rot(x[:1], J, sk)), full["joints"][:1])       # leading dimensions kept
        assert np.array_equal(host(rd.process_pos_from_real_rot(rows, J, sk)), full["local"][0])
        a = rd.output_bvh_from_real_rot(str(tmp_path / "a.bvh"), rows, J, chains, off, names=[f"b{i}" for i in range(J)])
        assert "JOINT b5\n" in open(tmp_path / "a.bvh").read()
    assert np.array_equal(host(a.quats)[0], full["quats"][0]) and np.array_equal(host(a.root_pos)[0], full["root_pos"][0])
    rd.save_rot_bvhs([str(tmp_path / f"{b}.bvh") for b in range(3)], full["anim"], lengths)
    if route == rf.HML:
        assert open(tmp_path / "a.bvh").read() == open(tmp_path / "0.bvh").read()
    assert open(tmp_path / "1.bvh").read().count("\n") == open(tmp_path / "0.bvh").read().count("\n") - (T - 1)
    with pytest.raises(RuntimeError, match="decode_rotations runs on the GPU only"):
        rd.decode_rotations(x.cpu(), J, chains, off, route=route, **ik)


@pytest.mark.parametrize("route", rf.ROUTES)
def test_the_written_files(gold, route, tmp_path):
    """The HIERARCHY block equals the reference's recorded text character for character; the channel values read back with parse_bvh give
    the decoder's quaternions back within DESIGN.md's bound for read_bvh(save_bvh(x)), 4e-6 per component up to sign (three angles of
    9.2e-5 degrees), on frame-joints whose middle angle is clear of +-85 degrees.  Those left out are at most 1 % (uniform random
    rotations: 1 - sin 85 deg = 0.38 %), asserted first for the reference's own recorded quaternions."""
    T = 65
    for name in rf.TREES:
        J, chains, off = rf.tree(name)
        share, _ = rf.euler_clear_share(gold[f"{route}|{name}|T{T}|quats"])
        print(f"rotdec: files {route}|{name} share of frame-joints beyond 85 degrees (reference) {share:.4f}")
        assert share <= 0.01, (name, share)
        data = rf.make_rows(name, route, T)
        lengths = rf.lengths_of(T)
        got = decode(route, name, data, lengths)
        paths = [str(tmp_path / f"{name}_{b}.bvh") for b in range(3)]
        rd.save_rot_bvhs(paths, got["anim"], lengths)
        want = gold[f"{route}|{name}|hierarchy"].tobytes().decode()
        seq = bvh.writer_sequence(got["anim"].parents)
        left, total, worst = 0, 0, 0.0
        for b, n in enumerate(lengths):
            text = open(paths[b]).read()
            assert text[:text.index("MOTION")] == want, (name, b)
            assert f"Frames: {n}\nFrame Time: 0.050000\n" in text
            sk, ch = bvh.parse_bvh(paths[b])
            assert ch.shape == (n, 3 + 3 * len(seq))
            assert np.abs(ch[:, :3] - got["root_pos"][b, :n]).max() <= 5.1e-7                 # six decimals of text
            back = bf.eul2q(ch[:, 3:].reshape(n, len(seq), 3).astype(np.float64), "zyx", np.float64)
            q = got["quats"][b, :n][:, seq].astype(np.float64)
            q /= np.linalg.norm(q, axis=-1, keepdims=True)
            _, out = rf.euler_clear_share(q)
            d = np.minimum(np.abs(back - q).max(-1), np.abs(back + q).max(-1))
            left, total = left + int(out.sum()), total + out.size
            worst = max(worst, float(d[~out].max()))
        print(f"rotdec: files {route}|{name} read back got {worst:.3e} bound 4.0e-06, left out {left} of {total}")
        assert worst <= 4e-6 and left <= 0.01 * total, (name, worst, left, total)


def test_rotation_and_position_channels_of_an_encoded_clip_agree(gold):
    """What the feature exists to offer: `recover_from_rot` against `recover_from_ric` on a HumanML row.  A clip encoded by encode_joints
    carries both.  The bar is the rule above with the reference's own distance for this clip, recorded by the golden maker
    (`dist|consistency|rot`: its float32 `recover_from_rot` against float64): each decoder is within it of the float64 fixture, the two
    agree within it, and with ONE 6D block of one frame perturbed they differ by more than 100 x it."""
    sk, pos, off, _, rows64 = rf.consistency_case()
    J, T = sk.J, pos.shape[1]
    rot64 = rf.hml_rot(rows64, J, sk.chains, off, np.float64)["joints"]
    ric64 = ef.recover_from_ric(rows64, J, np.float64)
    own, own_ric = float(gold["dist|consistency|rot"]), float(gold["dist|consistency|ric"])
    b = rf.bar(own)
    sample, lens = mp.encode_joints(cu(pos), mode=mp.HML, frames_out=T - 1, **sk.kw())
    assert int(lens[0]) == T - 1
    skel = type("S", (), dict(_offset=torch.from_numpy(off), _kinematic_tree=sk.chains, _parents=sk.parents))
    rows = sample[0, :, 0].T.contiguous()
    rot = host(rd.recover_from_rot(rows, J, skel))
    ric = host(mp.recover_from_ric(rows, J))
    e_rot, e_ric, gap = rf.relmax(rot, rot64), rf.relmax(ric, ric64), rf.relmax(rot, ric)
    print(f"rotdec: consistency rot ref {own:.3e} got {e_rot:.3e} bar {b:.3e}; ric ref {own_ric:.3e} got {e_ric:.3e} bar {rf.bar(own_ric):.3e}; "
          f"rot vs ric {gap:.3e} bar {b:.3e}")
    assert e_rot <= b and e_ric <= rf.bar(own_ric) and gap <= b
    bad = rows.clone()
    j, t = 9, 30
    blk = 4 + 3 * (J - 1) + 6 * (j - 1)
    bad[t, blk:blk + 6] = bad[t, blk:blk + 6].roll(2)               # one block of one frame
    rot_bad = host(rd.recover_from_rot(bad, J, skel))
    ric_bad = host(mp.recover_from_ric(bad, J))
    assert np.array_equal(ric_bad, ric)                              # the position channels do not see it
    gap_bad = rf.relmax(rot_bad, ric_bad)
    print(f"rotdec: consistency perturbed rot vs ric {gap_bad:.3e} ({gap_bad / b:.0f} bars)")
    assert gap_bad > 100 * b
    keep = np.ones(T - 1, bool)
    keep[t] = False
    assert np.array_equal(rot_bad[keep], rot[keep])                  # and only that frame moves


def test_a_fit_encoded_by_encode_fit_gives_its_positions_back():
    """fit_joints -> encode_fit -> recover_from_real_rot: the rotation channels of the encoded fit, decoded, are the fit's own positions
    in the encoder's frame (floor, origin and initial facing removed: the fixture's float64 `global_positions` of fit.positions).  The
    bar is the 4 x rule, for the decoder against the float64 fixture of the same rows and against the positions themselves alike.  The fit
    is computed on the GPU, so no reference distance can be recorded for it: the float32 fixture, which the golden maker holds no further
    from the reference than the reference is from float64, stands for the reference."""
    from mst_amd.utils import joint_fit as jf
    J, T = 21, 40
    sk = ef.skeleton(SEED, J, 6.0)
    off = sk.offsets.astype(np.float32)
    data, target = rf.ik.make_clip(SEED, "rotdec/fit", T, J, sk.parents, off, noise=0.03 * 6.0)
    fit = jf.fit_joints(cu(data), J, sk.parents, off, cu(target), 5)
    pos, quats = host(fit.positions), host(fit.joint_quats)
    e32, _ = ef.encode(pos, quats, sk, ef.POSROT, np.float32, frames_out=T - 1)
    e64, diags = ef.encode(pos, quats, sk, ef.POSROT, np.float64, frames_out=T - 1)
    ef.assert_clear(diags, ef.POSROT)
    j32, j64 = (rf.real_rot(e["sample"][0, :, 0].T, J, sk.chains, off, dt)["joints"] for e, dt in ((e32, np.float32), (e64, np.float64)))
    want = e64["global_positions"][0, :T - 1]
    model = rf.relmax(j64, want)
    assert model <= rf.FLOOR, model
    sample, lens = jf.encode_fit(fit.positions, fit, chains=sk.chains, face_joint_indx=sk.face, fid_l=sk.fid_l, fid_r=sk.fid_r)
    n = int(lens[0])
    assert n == T - 1
    skel = type("S", (), dict(_offset=torch.from_numpy(off), _kinematic_tree=sk.chains, _parents=sk.parents))
    got = host(rd.recover_from_real_rot(sample[0, :, 0, :n].T.contiguous(), J, skel))
    own = rf.relmax(j32, j64)
    e, back = rf.relmax(got, j64), rf.relmax(got, want)
    print(f"rotdec: fit round trip ref {own:.3e} got {e:.3e} bar {rf.bar(own):.3e}; against fit.positions {back:.3e} (float64: {model:.3e})")
    assert e <= rf.bar(own) and back <= rf.bar(own)


@pytest.mark.parametrize("route", rf.ROUTES)
def test_a_side_stream_behind_queued_work_gives_the_default_streams_bits(route):
    name, T = "t2m22", 257
    J, chains, off = rf.tree(name)
    lengths = rf.lengths_of(T)
    x = cu(rf.make_rows(name, route, T))
    want = decode(route, name, x, lengths)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=dev())
    with torch.cuda.stream(side):
        y = x.clone()                                                # produced on the side stream, behind the products
        for _ in range(8):
            a = a @ a * 1e-3
        y += 0
        got = decode(route, name, y, lengths)
    side.synchronize()
    for k in rf.OUTPUTS[route]:
        assert np.array_equal(got[k], want[k]), k
