"""Motion files without a GPU: the BVH text parser and writer against the reference's recorded files (tests/golden/bvh.npz, byte for byte),
every refusal of the parser, the numpy fixture against the recorded arrays under the suite's bar, the C ABI's host-side refusals, and
the CPU-tensor errors."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import bvh_fixture as bf
import mst_amd  # noqa: F401
from conftest import ROOT
from mst_amd.utils import bvh
from mst_amd.utils import motion_process as mp

SEED = bf.SEED
G = np.load(os.path.join(ROOT, "tests", "golden", "bvh.npz"))


def test_the_seed_is_the_golden_scripts():
    import re
    text = open(os.path.join(ROOT, "tests", "golden", "make_golden.py")).read()
    assert int(re.search(r"^SEED\s*=\s*(\d+)", text, re.M).group(1)) == SEED


def _writer(name):
    names, par, off, end, order, positions, q, pos = bf.writer_case(SEED, name)
    sk, seq = bvh.writer_skeleton(names, par, off, end, order, positions, 1 / 30)
    return sk, seq, (names, par, off, end, order, positions, q, pos)


@pytest.mark.parametrize("name", list(bf.GOLDEN_WRITE))
def test_format_bvh_equals_the_reference_text_byte_for_byte(name):
    sk, seq, _ = _writer(name)
    assert seq == bvh.writer_sequence(_[1])
    assert bvh.format_bvh(sk, G[f"{name}|channels"]).encode() == G[f"{name}|text"].tobytes()


@pytest.mark.parametrize("name", list(bf.GOLDEN_WRITE))
def test_parse_bvh_of_the_reference_text(name):
    text = G[f"{name}|text"].tobytes().decode()
    sk, ch = bvh.parse_bvh(text)
    assert sk.names == list(G[f"{name}|read_ends|bones"]) and sk.parents == list(G[f"{name}|read_ends|parents"])
    assert np.array_equal(sk.offsets, G[f"{name}|read_ends|offsets"]) and sk.offsets.dtype == np.float32
    assert np.array_equal(sk.end_offsets, G[f"{name}|read|end_offsets"])
    assert sk.simple_names == list(G[f"{name}|read|bones"]) and sk.simple_parents == list(G[f"{name}|read|parents"])
    assert np.array_equal(sk.offsets[sk.not_end_index], G[f"{name}|read|offsets"])
    assert sk.order == bf.GOLDEN_WRITE[name][3] and abs(sk.frametime - 1 / 30) < 1e-6
    rows = [ln.split() for ln in text.split("MOTION\n")[1].split("\n")[2:] if ln.strip()]
    assert ch.dtype == np.float32 and np.array_equal(ch, np.array([[np.float32(float(v)) for v in r] for r in rows]))
    root6 = bf.GOLDEN_WRITE[name][2] == "root6"
    keep = sk.not_end_index
    assert [sk.pos_col[j] for j in keep] == ([0] + [-1] * (len(keep) - 1) if root6 else [6 * k for k in range(len(keep))])
    assert [sk.rot_col[j] for j in keep] == ([3 * k + 3 for k in range(len(keep))] if root6 else [6 * k + 3 for k in range(len(keep))])
    assert all(sk.rot_col[j] == -1 and sk.pos_col[j] == -1 for j in range(sk.joints) if sk.is_end[j])
    assert np.abs(ch - G[f"{name}|channels"]).max() <= 5.1e-7 * max(1.0, np.abs(ch).max())          # six decimals of values up to 180


@pytest.mark.parametrize("name", list(bf.GOLDEN_WRITE) + list(bf.GOLDEN_DECODE))
def test_parse_of_format_keeps_structure_and_values(name):
    if name in bf.GOLDEN_WRITE:
        sk, ch = bvh.parse_bvh(G[f"{name}|text"].tobytes().decode())
    else:
        Jf, T, layout, order = bf.GOLDEN_DECODE[name]
        sk = bf.file_skeleton(SEED, name, Jf, layout, order)
        ch = bf.channels(SEED, name, sk, T)[0]
    text = bvh.format_bvh(sk, ch)
    sk2, ch2 = bvh.parse_bvh(text)
    assert sk2.same_hierarchy(sk) and abs(sk2.frametime - sk.frametime) < 1e-6
    assert np.abs(ch2 - ch).max() <= 5.1e-7 * max(1.0, np.abs(ch).max())
    assert bvh.format_bvh(sk2, ch2) == text                           # a fixed point after one pass


def test_start_and_end_follow_the_reference_arithmetic(tmp_path):
    text = G["w6|text"].tobytes().decode()
    p = tmp_path / "a.bvh"
    p.write_text(text)
    full = bvh.parse_bvh(str(p))[1]
    assert np.array_equal(bvh.parse_bvh(p, start=5, end=17)[1], full[5:17])
    assert np.array_equal(bvh.parse_bvh(p, start=7)[1], full[7:])
    assert np.array_equal(bvh.parse_bvh(p, end=9)[1], full[:9])
    assert np.array_equal(bvh.parse_bvh(p, start=0, end=9)[1], full[:9])        # 0 counts as not given, as in the reference
    with pytest.raises(ValueError, match="select"):
        bvh.parse_bvh(p, start=30, end=99)


def _edit(text, old, new):
    assert text.count(old) >= 1
    return text.replace(old, new, 1)


def test_every_refusal_names_its_line():
    text = G["w6|text"].tobytes().decode()
    lines = text.split("\n")
    chan3 = next(i for i, ln in enumerate(lines) if "CHANNELS 3" in ln)
    motion = lines.index("MOTION")
    cases = {
        "nine": (_edit(text, "CHANNELS 3 Zrotation Yrotation Xrotation", "CHANNELS 9 Xposition Yposition Zposition Zrotation Yrotation Xrotation "
                       "Xscale Yscale Zscale"), chan3 + 1, "nine-channel"),
        "order": (_edit(text, "CHANNELS 3 Zrotation Yrotation Xrotation", "CHANNELS 3 Xrotation Yrotation Zrotation"), chan3 + 1, "differs"),
        "positions": (_edit(text, "Xposition Yposition Zposition", "Yposition Xposition Zposition"), 5, "X, Y, Z order"),
        "row": ("\n".join(lines[:motion + 5] + [lines[motion + 5] + " 1.0"] + lines[motion + 6:]), motion + 6, "frame row"),
        "frames": (_edit(text, "Frames: 40", "Frames: 41"), motion + 2, "Frames: 41"),
    }
    for name, (bad, line, word) in cases.items():
        with pytest.raises(ValueError, match=f"line {line}:.*{word}"):
            bvh.parse_bvh(bad)
    with pytest.raises(NotImplementedError, match="fractional"):
        bvh.read_bvh("unused.bvh", downsample_rate=1.5)
    with pytest.raises(NotImplementedError, match="q2eul"):
        bvh.quats_to_channels(torch.zeros(1, 2, 3, 4), torch.zeros(1, 2, 3), [-1, 0, 1], order="yxz")
    with pytest.raises(ValueError, match="no tree"):
        bvh.writer_sequence([-1, 0, 3, 2])


def test_writer_sequence_is_depth_first_children_in_index_order():
    assert bvh.writer_sequence([-1, 0, 0, 1, 2, 1]) == [0, 1, 3, 5, 2, 4]
    sk, seq = bvh.writer_skeleton(None, [-1, 0, 0, 1, 2, 1], np.arange(18).reshape(6, 3), None, "zyx", False)
    assert seq == [0, 1, 3, 5, 2, 4] and sk.names == [f"joint_{j}" for j in seq] and sk.parents == [-1, 0, 1, 1, 0, 4]
    assert np.array_equal(sk.offsets, np.arange(18, dtype=np.float32).reshape(6, 3)[seq])
    text = bvh.format_bvh(sk, np.zeros((1, 21), np.float32))
    assert text.count("End Site") == 3 and "\t\t\t\tOFFSET 0.000000 0.000000 0.000000\n" in text


# ------------------------------------------------------------------------------------------ the fixture against the reference's arrays
def _check(case, name, got, f32, f64):
    own, dev = bf.rel(f32, f64), bf.rel(got, f64)
    print(f"bvh: {case} {name} ref {own:.3e} got {dev:.3e} bar {bf.bar(own):.3e}")
    assert dev <= bf.bar(own), (case, name, dev, own)


@pytest.mark.parametrize("name", list(bf.GOLDEN_WRITE) + list(bf.GOLDEN_DECODE))
def test_fixture_decode_against_the_recorded_read(name):
    if name in bf.GOLDEN_WRITE:
        sk, ch = bvh.parse_bvh(G[f"{name}|text"].tobytes().decode())
    else:
        Jf, T, layout, order = bf.GOLDEN_DECODE[name]
        sk = bf.file_skeleton(SEED, name, Jf, layout, order)
        sk, ch = bvh.parse_bvh(bvh.format_bvh(sk, bf.channels(SEED, name, sk, T)[0]))
    f32, f64 = bf.decode(ch, sk, np.float32), bf.decode(ch, sk, np.float64)
    bf.assert_clear(dots=f64["dots"])
    assert (f64["signs"] < 0).any()
    quats = G[f"{name}|read_ends|quats"]
    assert np.array_equal(np.sign((quats * f64["rotations"]).sum(-1)), np.ones(quats.shape[:2]))          # every sign decision
    assert np.array_equal(f32["signs"], f64["signs"])
    _check(name, "quats", f32["rotations"], quats, f64["rotations"])
    _check(name, "pos", f32["local_positions"], G[f"{name}|read_ends|pos"], f64["local_positions"])
    _check(name, "fk", f32["positions"], G[f"{name}|fk"], f64["positions"])


@pytest.mark.parametrize("name", list(bf.GOLDEN_WRITE))
def test_fixture_channels_against_the_recorded_degrees(name):
    names, par, off, end, order, positions, q, pos = bf.writer_case(SEED, name)
    bf.assert_clear(writer=q, order=order)
    f32, f64 = (bf.channels_from_quats(q, pos[:, 0], par, order, pos if positions else None, dt) for dt in (np.float32, np.float64))
    wrap = lambda a: (a + 180) % 360 - 180
    own, dev = np.abs(wrap(G[f"{name}|channels"] - f64)).max() / 180, np.abs(wrap(f32 - f64)).max() / 180
    print(f"bvh: {name} degrees ref {own:.3e} got {dev:.3e} bar {bf.bar(own):.3e}")
    assert dev <= bf.bar(own)


@pytest.mark.parametrize("J,T", bf.GOLDEN_RETARGET)
def test_fixture_retarget_against_the_recorded_joints(J, T):
    sk, pos, tgt, l_idx = bf.retarget_case(SEED, J, T)
    f32, _ = bf.retarget(pos[0], tgt, sk.raw, sk.chains, l_idx, sk.face, np.float32)
    f64, diag = bf.retarget(pos[0], tgt, sk.raw, sk.chains, l_idx, sk.face, np.float64)
    bf.assert_clear(retarget_diag=diag)
    _check(f"retarget J{J}T{T}", "joints", f32, G[f"retarget|J{J}T{T}"], f64)
    par = bf.ik.parents_of(sk.chains, J)
    bones = np.linalg.norm(f64[:, 1:] - f64[:, par[1:]], axis=-1)
    assert np.abs(bones - np.linalg.norm(tgt[1:].astype(np.float64), axis=-1)).max() < 1e-9


def test_sign_scan_is_a_prefix_parity():
    sk = bf.file_skeleton(SEED, "parity", 6)
    d = bf.decode(bf.channels(SEED, "parity", sk, 300, step=4.0)[0], sk, np.float64)
    bf.assert_clear(dots=d["dots"])
    parity = np.concatenate([np.zeros((1, sk.joints)), np.cumsum(d["dots"] < 0, 0)]) % 2
    assert np.array_equal(d["signs"], 1 - 2 * parity) and (d["signs"] < 0).any()
    assert np.abs(d["dots"]).min() >= 0.97


# ------------------------------------------------------------------------------------------ the ABI without a GPU
def test_abi_limits_and_bad_arguments():
    from mst_amd import _native as N
    lib = N.lib()
    assert lib.mst_bvh_max_joints() >= 80 and lib.mst_bvh_max_frames(80) >= 4096 and lib.mst_retarget_max_frames(22) >= 4096
    for fn, bad, word in ((lib.mst_bvh_max_frames, 0, b"joints 0"), (lib.mst_bvh_max_frames, lib.mst_bvh_max_joints() + 1, b"outside"),
                          (lib.mst_retarget_max_frames, 1, b"joints 1"), (lib.mst_retarget_max_frames, 25, b"joints 25")):
        assert fn(bad) == -1 and word in lib.mst_last_error()
    assert bvh.max_joints() == lib.mst_bvh_max_joints() and bvh.max_frames(31) == lib.mst_bvh_max_frames(31)
    assert mp.retarget_max_frames(22) == lib.mst_retarget_max_frames(22)
    with pytest.raises(RuntimeError, match="outside"):
        bvh.max_frames(0)
    i3 = lambda *v: (C.c_int32 * len(v))(*v)
    f3 = (C.c_float * 6)()
    one = C.c_void_p(16)                     # never dereferenced: every call below is refused before a launch
    dec = lambda **k: lib.mst_bvh_decode(one, None, k.get("B", 1), k.get("T", 4), k.get("C", 9), k.get("J", 2), k.get("par", i3(-1, 0)),
                                         k.get("rot", i3(3, 6)), k.get("pos", i3(0, -1)), f3, k.get("order", i3(2, 1, 0)), 1.0, k.get("stride", 1),
                                         k.get("phase", 0), k.get("sel", None), k.get("nsel", 0), one, one, one, None, None, None)
    for kw, word in ((dict(J=0), b"joints 0"), (dict(J=97), b"joints 97"), (dict(T=0), b"frames 0"), (dict(T=10 ** 6), b"mst_bvh_max_frames"),
                     (dict(C=13), b"13 channels"), (dict(stride=0), b"stride 0"), (dict(phase=1), b"phase 1"), (dict(stride=8, phase=5), b"no frame"),
                     (dict(par=i3(-1, 1)), b"parents[1]"), (dict(par=i3(0, 0)), b"parents[0]"), (dict(rot=i3(3, 7)), b"rotation column 7"),
                     (dict(pos=i3(0, 8)), b"position column 8"), (dict(order=i3(2, 2, 0)), b"no permutation"),
                     (dict(sel=i3(0, 0), nsel=2), b"selected twice"), (dict(sel=i3(0, 2), nsel=2), b"selected joint 2"), (dict(nsel=25, sel=i3(0)), b"25 selected")):
        assert dec(**kw) != 0 and word in lib.mst_last_error(), (kw, lib.mst_last_error())
    q2c = lambda J=2, perm=i3(0, 1), order=0: lib.mst_quats_to_channels(one, one, None, perm, 1, 4, J, order, one, None)
    for kw, word in ((dict(J=0), b"joints 0"), (dict(order=2), b"order 2"), (dict(perm=i3(0, 0)), b"not a permutation"), (dict(perm=i3(1, 0)), b"root")):
        assert q2c(**kw) != 0 and word in lib.mst_last_error(), (kw, lib.mst_last_error())
    ret = lambda J=3, T=4, face=i3(0, 1, 2, 3), chains=i3(0, 1, 2, 3), starts=i3(0, 4), legs=i3(1, 2), out=one: lib.mst_retarget_joints(
        C.c_void_p(32), None, 1, T, J, face, chains, starts, 1, (C.c_float * 72)(), (C.c_float * 72)(), legs, out, None)
    for kw, word in ((dict(J=1), b"joints 1"), (dict(T=0), b"frames 0"), (dict(T=10 ** 6), b"mst_retarget_max_frames"), (dict(J=4, face=i3(0, 1, 2, 4)), b"face joint 4"),
                     (dict(J=4, face=i3(0, 1, 1, 3)), b"duplicate"), (dict(J=4, chains=i3(1, 2, 3, 0)), b"starts at joint 1"),
                     (dict(J=4, legs=i3(0, 2)), b"leg joint 0"), (dict(J=4, out=C.c_void_p(32)), b"may not be the input")):
        assert ret(**kw) != 0 and word in lib.mst_last_error(), (kw, lib.mst_last_error())


def test_cpu_tensors_raise():
    sk = bf.file_skeleton(SEED, "cpu", 6)
    ch = torch.from_numpy(bf.channels(SEED, "cpu", sk, 8))
    with pytest.raises(RuntimeError, match="runs on the GPU only"):
        bvh.decode_channels(ch, sk)
    with pytest.raises(RuntimeError, match="runs on the GPU only"):
        bvh.quats_to_channels(torch.zeros(1, 2, 3, 4), torch.zeros(1, 2, 3), [-1, 0, 1])
    with pytest.raises(RuntimeError, match="runs on the GPU only"):
        bvh.load_bvh([G["w6|text"].tobytes().decode()], device="cpu")
    esk, pos, tgt, l_idx = bf.retarget_case(SEED, 5, 4)
    with pytest.raises(RuntimeError, match="runs on the GPU only"):
        mp.retarget_joints(torch.from_numpy(pos), tgt, esk.raw, esk.chains, l_idx, esk.face)
    with pytest.raises(ValueError, match="lengths"):
        bvh.decode_channels(ch, sk, lengths=[9])
    with pytest.raises(ValueError, match="selected twice"):
        bvh.decode_channels(ch, sk, joints=[0, 1, 1])
    with pytest.raises(ValueError, match="l_idx"):
        mp.retarget_joints(torch.from_numpy(pos), tgt, esk.raw, esk.chains, (0, 1), esk.face)
