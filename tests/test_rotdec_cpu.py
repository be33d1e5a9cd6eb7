"""The rotation-channel decoders without a GPU: tests/rotdec_fixture.py against the reference's recorded outputs
(tests/golden/rotdec.npz), `expand_chains` on the three trees and on a chain list in another order, every refusal of the Python layer
(raised before any GPU call), the drop-in signatures, and the C ABI's declarations and refusals.

The golden bar is the suite's rule: 4 x the reference's own float32-to-float64 distance for the case and output, as the golden maker
recorded it, floor 1e-6.  Every case prints `rotdec: fixture <case> <output> ref <dist> got <dist> bar <bar>`."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
import rotdec_fixture as rf
from conftest import GOLDEN, ROOT
from mst_amd.utils import rot_decode as rd


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "rotdec.npz"))


@pytest.mark.parametrize("route", rf.ROUTES)
@pytest.mark.parametrize("name", rf.TREES)
def test_the_fixture_against_the_reference_outputs(gold, route, name):
    J, chains, off = rf.tree(name)
    for T in rf.STORED:
        data = rf.make_rows(name, route, T)
        keep = data.copy()
        fn = rf.DECODE[route]
        f32, f64 = fn(data[0], J, chains, off, np.float32), fn(data[0], J, chains, off, np.float64)
        assert np.array_equal(data, keep)
        key = f"{route}|{name}|T{T}"
        for k in rf.OUTPUTS[route]:
            r = gold[f"{key}|{k}"]
            own = float(gold[f"dist|{key}|{k}"])
            e, mine = rf.distance(k, r, f64[k]), rf.distance(k, f32[k], f64[k])
            print(f"rotdec: fixture {key} {k} ref {own:.3e} got {e:.3e} fixture f32 {mine:.3e} bar {rf.bar(own):.3e}")
            assert r.shape == f64[k].shape and r.dtype == np.float32
            assert e <= rf.bar(own) and mine <= rf.bar(own), (key, k)
            if T == 7:
                assert rf.distance(k, gold[f"{key}|{k}|f64"], f64[k]) <= 1e-12, (key, k)
        assert list(gold[f"{route}|{name}|parents"]) == list(f64["parents"])
        assert np.array_equal(gold[f"{route}|{name}|offsets"], f32["offsets"])
        if route == rf.REAL:                                  # the theta = 0 branch: exactly the identity, in both precisions and recorded
            j = rf.identity_joint(chains)
            for q in (f32["quats"], f64["quats"], gold[f"{key}|quats"]):
                assert (q[:, j] == np.array([1, 0, 0, 0])).all()
        elif route == rf.HML:
            # HML: the converted quaternion is not an output; q (x) (1, 0, 0, 0) = q makes two world quaternions equal bit for bit, and
            # the local quaternion between them has a vector part of exactly 0 -- without fused multiply-adds (torch.cross fuses: the
            # recorded float32 values are 1e-9, not 0)
            for i in rf.identity_carriers(name):
                assert (f64["quats"][:, i, 1:] == 0).all() and np.abs(gold[f"{key}|quats"][:, i, 1:]).max() < 1e-7
            assert rf.identity_carriers(name)
    for fn in ("output_bvh", "recover_from_rot", "output_bvh_with_pos", "output_bvh_from_real_rot", "recover_from_real_rot", "process_pos_from_real_rot"):
        assert float(gold[f"seconds|{fn}"]) > 0


@pytest.mark.parametrize("name", rf.TREES)
def test_the_reference_local_rows_as_they_run_lose_the_subtraction(gold, name):
    """The stated deviation, pinned by the reference's own output: on a 7-frame clip `process_pos_from_real_rot` as it runs returns the
    joints rotated but NOT moved to the root (its in-place subtraction reads the root's x and z after zeroing them), which is the
    fixture's `local_as_run` and not its root-relative `local`."""
    J, chains, off = rf.tree(name)
    key = f"real_rot|{name}|T7"
    f64 = rf.real_rot(rf.make_rows(name, rf.REAL, 7)[0], J, chains, off, np.float64)
    assert rf.relmax(gold[f"{key}|local_as_run|f64"], f64["local_as_run"]) <= 1e-12
    assert rf.relmax(gold[f"{key}|local_as_run"], f64["local_as_run"]) <= rf.bar(float(gold[f"dist|{key}|local"]))
    assert rf.relmax(gold[f"{key}|local_as_run"], f64["local"]) > 1e-3          # frame 0 stands at x = z = 0; the later frames do not
    assert rf.relmax(gold[f"{key}|local"], f64["local"]) <= rf.bar(float(gold[f"dist|{key}|local"]))


def test_every_case_of_the_gpu_test_has_a_recorded_distance(gold):
    for k in ("rot", "ric"):
        assert 0 < float(gold[f"dist|consistency|{k}"]) < 2e-6

    for route in rf.ROUTES:
        for name in rf.TREES:
            for T in rf.FRAMES + (rf.LONG,):
                for k in rf.OUTPUTS[route]:
                    d = float(gold[f"dist|{route}|{name}|T{T}|{k}"])
                    # fp32 rounding of a few operations, nothing else; POS_IK's bones are differences of positions up to a metre or two
                    # apart from the origin, which costs the reference's float32 a digit
                    assert 0 <= d < (2e-5 if route == rf.POS and k == "quats" else 2e-6), (route, name, T, k, d)


@pytest.mark.parametrize("name", rf.TREES)
def test_expand_chains(gold, name):
    J, chains, off = rf.tree(name)
    parents, xoff, source = rd.expand_chains(chains, off)
    fp, fo, fs = rf.expand_chains(chains, off)
    assert parents == fp == list(gold[f"hml_rot|{name}|parents"]) and source == fs
    assert np.array_equal(xoff, fo) and np.array_equal(xoff, gold[f"hml_rot|{name}|offsets"]) and xoff.dtype == np.float32
    Jx = J + len(chains)
    assert len(parents) == len(source) == Jx and xoff.shape == (Jx, 3)
    assert parents[0] == -1 and all(0 <= parents[i] < Jx for i in range(1, Jx))
    assert set(source) <= set(range(J)) and source[0] == 0     # (a joint's rotation may be dropped: a later chain's first write wins)
    assert int((np.abs(xoff).sum(1) == 0).sum()) == len(chains)                      # one zero-offset duplicate per chain
    assert rd.chain_parents(chains, J) == rf.chain_parents(chains, J) == list(gold[f"real_rot|{name}|parents"])
    text = gold[f"hml_rot|{name}|hierarchy"].tobytes().decode()
    assert text.count("JOINT ") + 1 == Jx and text.startswith("HIERARCHY\nROOT joint_0\n")


def test_expand_chains_later_write_wins():
    """Two chains off joint 2 in either order: the joint that begins a later chain is written twice, first as a member of its own chain
    (carrying its successor's rotation), then as the later chain's first joint (carrying its own)."""
    off = np.arange(18, dtype=np.float32).reshape(6, 3)
    a = [[0, 1, 2, 3], [2, 4], [2, 5]]
    pa, oa, sa = rd.expand_chains(a, off)
    assert pa == [-1, 0, 1, 2, 3, 3, 5, 3, 7]
    assert sa == [0, 1, 2, 2, 3, 4, 4, 5, 5]                 # new joint 3 is old joint 2: rewritten from 3 (its successor) to 2 (its own)
    assert np.array_equal(oa, rf.expand_chains(a, off)[1]) and (pa, sa) == tuple(rf.expand_chains(a, off)[k] for k in (0, 2))
    # the branches listed first: joint 2 is written as their first joint BEFORE its own chain writes it, and keeps its successor's rotation
    b = [[0, 1, 2], [2, 4], [2, 5], [2, 3]]
    pb, ob, sb = rd.expand_chains(b, off)
    assert (pb, sb) == tuple(rf.expand_chains(b, off)[k] for k in (0, 2))
    new2 = [i for i in range(len(pb)) if np.array_equal(ob[i], off[2])]
    assert len(new2) == 1 and sb[new2[0]] == 2                # [0, 1, 2] ends at joint 2: it repeats its own rotation, and the later chains agree
    c = [[0, 1, 2, 3], [2, 4]]
    d = [[0, 1, 2], [2, 4], [2, 3]]                           # the same tree; joint 3 hangs off joint 2 in a chain of its own
    (pc, oc, sc), (pd, od, sd) = rd.expand_chains(c, off[:5]), rd.expand_chains(d, off[:5])
    at = lambda o, j: [i for i in range(len(o)) if np.array_equal(o[i], off[j])][0]
    assert sc[at(oc, 1)] == 2 and sd[at(od, 1)] == 2          # joint 1 carries its successor's rotation either way
    assert len(pc) == 7 and len(pd) == 8                      # one duplicate per chain
    # a single chain: nothing is overwritten; the last joint has no successor and repeats the rotation of the one before it
    p1, o1, s1 = rd.expand_chains([[0, 1, 2]], off[:3])
    assert p1 == [-1, 0, 1, 2] and s1 == [0, 1, 2, 2] and np.array_equal(o1, np.array([off[0], [0, 0, 0], off[1], off[2]]))


def test_host_refusals():
    J, chains, off = rf.tree("tree3")
    hml, real = torch.zeros(1, 4, 35), torch.zeros(1, 4, 28)
    dec = lambda x=hml, J=J, chains=chains, off=off, route="hml_rot", **kw: rd.decode_rotations(x, J, chains, off, route=route, **kw)
    with pytest.raises(ValueError, match="route 'pos_ik' needs raw_offsets and face_joint_indx"):
        dec(route="pos_ik")
    with pytest.raises(ValueError, match="route 'pos_ik' needs raw_offsets and face_joint_indx"):
        dec(route="pos_ik", raw_offsets=rf.raw_of(off))
    with pytest.raises(ValueError, match=r"raw_offsets of shape \(2, 3\), expected \(3, 3\)"):
        dec(route="pos_ik", raw_offsets=rf.raw_of(off)[:2], face_joint_indx=(1, 2, 1, 2))
    with pytest.raises(ValueError, match=r"face_joint_indx \[1, 2, 3, 2\]: four joints of 0\.\.2"):
        dec(route="pos_ik", raw_offsets=rf.raw_of(off), face_joint_indx=(1, 2, 3, 2))
    with pytest.raises(ValueError, match=r"face_joint_indx \[1, 2, 1\]: four joints"):
        dec(route="pos_ik", raw_offsets=rf.raw_of(off), face_joint_indx=(1, 2, 1))
    with pytest.raises(ValueError, match="raw_offsets and face_joint_indx belong to route 'pos_ik', not 'hml_rot'"):
        dec(raw_offsets=rf.raw_of(off))
    with pytest.raises(ValueError, match="belong to route 'pos_ik', not 'real_rot'"):
        dec(real, route="real_rot", face_joint_indx=(1, 2, 1, 2))
    with pytest.raises(ValueError, match="route 'euler' is none of"):
        dec(route="euler")
    with pytest.raises(TypeError, match="sample is a tensor"):
        dec(hml.numpy())
    with pytest.raises(ValueError, match=r"1 joints outside 2\.\.24 \(mst_rot_decode_max_joints\)"):
        dec(J=1)
    with pytest.raises(ValueError, match=r"25 joints outside 2\.\.24"):
        dec(J=25)
    with pytest.raises(ValueError, match=r"28 features, expected 12 \* J - 1 = 35, the row of route 'hml_rot' at 3 joints"):
        dec(real)
    with pytest.raises(ValueError, match=r"35 features, expected 9 \* J \+ 1 = 28"):
        dec(hml, route="real_rot")
    with pytest.raises(ValueError, match=r"sample of shape \(4, 35\), expected \[B, T, 35\] or the samplers' \[B, 35, 1, T\]"):
        dec(hml[0])
    with pytest.raises(ValueError, match=r"offsets of shape \(2, 3\), expected \(3, 3\)"):
        dec(off=off[:2])
    with pytest.raises(ValueError, match="chain 1 starts at joint 2, which no earlier chain has placed"):
        dec(chains=[[0, 1], [2, 1]])
    with pytest.raises(ValueError, match="joint 1 is named twice as a child"):
        dec(chains=[[0, 1], [0, 1, 2]])
    with pytest.raises(ValueError, match="joint 2 is named by no chain"):
        dec(chains=[[0, 1]])
    with pytest.raises(ValueError, match=r"joint 3 of chain 0 outside 0\.\.2"):
        dec(chains=[[0, 3], [0, 2]])
    with pytest.raises(ValueError, match="chain 1 has fewer than two joints"):
        dec(chains=[[0, 1, 2], [0]])
    with pytest.raises(ValueError, match="no kinematic chains"):
        dec(chains=[])
    with pytest.raises(ValueError, match="mean and std come together"):
        dec(mean=np.zeros(35))
    with pytest.raises(ValueError, match=r"std of shape \(34,\), expected \(35,\)"):
        dec(mean=np.zeros(35), std=np.ones(34))
    with pytest.raises(ValueError, match=r"lengths 0\.\.0 outside 1\.\.4"):
        dec(lengths=[0])
    with pytest.raises(ValueError, match=r"lengths 5\.\.5 outside 1\.\.4"):
        dec(lengths=torch.tensor([5]))
    with pytest.raises(ValueError, match="2 lengths for 1 clips"):
        dec(lengths=[1, 2])
    with pytest.raises(ValueError, match="the local rows .* belong to route 'real_rot'"):
        dec(local=True)
    with pytest.raises(ValueError, match="no output asked for"):
        dec(quats=False, root_pos=False)
    limit = rd.max_frames(3)
    assert limit == 4096 and rd.max_joints() == 24
    with pytest.raises(RuntimeError, match=rf"{limit + 1} frames > {limit}.*mst_rot_decode_max_frames\(3\)"):
        dec(torch.zeros(1, limit + 1, 35))
    # everything in order, but on the CPU
    for call in (lambda: dec(), lambda: dec(real, route="real_rot", joints=True, local=True), lambda: dec(hml.permute(0, 2, 1)[:, :, None]),
                 lambda: dec(lengths=[3]), lambda: dec(route="pos_ik", raw_offsets=rf.raw_of(off), face_joint_indx=(1, 2, 1, 2))):
        with pytest.raises(RuntimeError, match="decode_rotations runs on the GPU only"):
            call()

    class Sk:
        _offset, _kinematic_tree, _parents = torch.from_numpy(off), chains, [-1, 0, 0]

    for fn, x in ((rd.recover_from_rot, hml[0]), (rd.recover_from_real_rot, real[0]), (rd.process_pos_from_real_rot, real[0])):
        with pytest.raises(RuntimeError, match=f"{fn.__name__} runs on the GPU only"):
            fn(x, J, Sk)
        with pytest.raises(TypeError, match="skeleton has no `_offset`"):
            fn(x, J, object())
    for fn, x in ((rd.output_bvh, hml[0]), (rd.output_bvh_from_real_rot, real[0])):
        with pytest.raises(RuntimeError, match=f"{fn.__name__} runs on the GPU only"):
            fn("never_written.bvh", x, J, chains, off)
    assert not os.path.exists("never_written.bvh")
    with pytest.raises(RuntimeError, match="output_bvh_with_pos runs on the GPU only"):
        rd.output_bvh_with_pos("never_written.bvh", hml[0], J, chains, off, rf.raw_of(off), (1, 2, 1, 2))
    with pytest.raises(NotImplementedError, match="output_bvh_with_22rot is not covered"):
        rd.output_bvh_with_22rot("x.bvh", None, None, J, chains, off)
    with pytest.raises(NotImplementedError, match="fit_joints_bvh_quats is not covered"):
        rd.fit_joints_bvh_quats()
    with pytest.raises(TypeError, match="anim is a RotAnim"):
        rd.save_rot_bvhs(["x.bvh"], object())
    anim = rd.RotAnim(torch.zeros(2, 4, 3, 4), torch.zeros(2, 4, 3), [-1, 0, 0], off)
    with pytest.raises(ValueError, match="1 paths for 2 clips"):
        rd.save_rot_bvhs(["x.bvh"], anim)
    with pytest.raises(ValueError, match=r"lengths \[4, 5\] for 2 clips of 4 frames"):
        rd.save_rot_bvhs(["x.bvh", "y.bvh"], anim, lengths=[4, 5])


def test_the_drop_in_signatures():
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(rd.recover_from_rot) == ["data", "joints_num", "skeleton"]
    assert names(rd.recover_from_real_rot) == ["data", "joints_num", "skeleton"]
    assert names(rd.process_pos_from_real_rot) == ["data", "joints_num", "skel"]
    assert names(rd.output_bvh) == ["path", "data", "joints_num", "kinematic_chain", "tgt_offsets"]
    assert names(rd.output_bvh_from_real_rot) == ["path", "data", "joints_num", "kinematic_chain", "tgt_offsets", "names"]
    assert names(rd.output_bvh_with_pos) == ["path", "data", "joints_num", "kinematic_chain", "tgt_offsets", "n_raw_offsets", "face_joint_indx",
                                             "bone_names"]
    sig = inspect.signature(rd.decode_rotations)
    assert names(rd.decode_rotations)[:4] == ["sample", "joints_num", "chains", "offsets"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names(rd.decode_rotations)[4:])
    assert names(rd.decode_rotations)[4:] == ["route", "mean", "std", "lengths", "raw_offsets", "face_joint_indx", "joints", "local", "quats",
                                              "root_pos"]
    assert sig.parameters["joints"].default is False and sig.parameters["local"].default is False
    assert names(rd.save_rot_bvhs) == ["paths", "anim", "lengths", "frametime"] and inspect.signature(rd.save_rot_bvhs).parameters["frametime"].default == 1 / 20


def test_the_c_abi_declares_exports_and_refuses():
    from mst_amd import _native as N
    text = open(os.path.join(ROOT, "include", "mst_engine.h")).read()
    lib = N.lib()
    for name in ("mst_rot_decode", "mst_rot_decode_max_joints", "mst_rot_decode_max_frames"):
        assert name in N.SIGNATURES and re.search(rf"\bint {name}\(", text) and hasattr(lib, name)
    decl = re.search(r"\bint mst_rot_decode\((.*?)\);", text, flags=re.S).group(1)
    assert len(decl.split(",")) == len(N.SIGNATURES["mst_rot_decode"][1]) == 26
    assert lib.mst_rot_decode_max_joints() == 24
    for J in (2, 22, 24):
        assert lib.mst_rot_decode_max_frames(J) == 4096
    assert lib.mst_rot_decode_max_frames(1) == -1 and b"joints 1 outside 2..24" in lib.mst_last_error()
    assert lib.mst_rot_decode_max_frames(25) == -1

    one = C.c_void_p(8)                                    # never dereferenced: every case is refused before a launch
    ints = lambda v: (C.c_int32 * max(len(v), 1))(*v)

    def call(route=0, joints=3, frames=4, feats=None, batch=1, data=one, mean=None, std=None, chains=((0, 1), (0, 2)), off=True,
             source=(0, 1, 1, 2, 2), parents=(-1, 0, 1, 0, 3), out_joints=None, quats=one, root=one, jpos=None, local=None,
             face=(1, 2, 1, 2), raw=True):
        flat = [j for c in chains or () for j in c]
        starts = [0]
        for c in chains or ():
            starts.append(starts[-1] + len(c))
        feats = (12 * joints - 1 if route != 1 else 9 * joints + 1) if feats is None else feats
        if out_joints is None:
            out_joints = 5 if route != 1 else joints
        raws = (C.c_float * (3 * 24))() if raw and route == 2 else None
        offs = (C.c_float * (3 * 24))() if off else None
        return lib.mst_rot_decode(data, frames * feats, feats, 1, mean, std, None, batch, frames, feats, joints, route,
                                  ints(flat) if chains is not None else None, ints(starts), len(chains) if chains is not None else 0, offs,
                                  ints(face) if face is not None and route == 2 else None, raws,
                                  ints(source) if source is not None else None, ints(parents) if parents is not None else None, out_joints,
                                  quats, root, jpos, local, None)

    for kw, msg in ((dict(route=3), b"route 3 is none of 0 (HML_ROT), 1 (REAL_ROT), 2 (POS_IK)"), (dict(route=-1), b"route -1 is none of"),
                    (dict(route=2, face=None), b"route 2 (POS_IK) needs the face joints and the raw offsets"),
                    (dict(route=2, raw=False), b"route 2 (POS_IK) needs the face joints and the raw offsets"),
                    (dict(route=2, face=(1, 2, 3, 2)), b"face joint 3 outside 0..2"), (dict(route=2, face=(1, -1, 1, 2)), b"face joint -1 outside"),
                    (dict(route=2, feats=28), b"feats 28 != 12 * joints - 1 = 35"), (dict(route=2, local=one), b"belong to route 1"),
                    (dict(route=2, source=None), b"null gather map or parents"), (dict(joints=1, feats=11), b"joints 1 outside 2..24"),
                    (dict(joints=25, feats=299), b"joints 25 outside"), (dict(feats=28), b"feats 28 != 12 * joints - 1 = 35"),
                    (dict(route=1, feats=35), b"feats 35 != 9 * joints + 1 = 28"), (dict(frames=0), b"frames 0 < 1"),
                    (dict(frames=4097), b"frames 4097 > 4096 (mst_rot_decode_max_frames)"), (dict(batch=0), b"batch 0 outside 1..65535"),
                    (dict(batch=65536), b"batch 65536 outside"), (dict(data=None), b"null data"),
                    (dict(mean=one), b"mean and std come together"), (dict(std=one), b"mean and std come together"),
                    (dict(chains=None), b"null skeleton"), (dict(off=False), b"null skeleton"),
                    (dict(quats=None, root=None), b"no output asked for"), (dict(local=one), b"local rows (process_pos_from_real_rot) belong to route 1"),
                    (dict(chains=((0, 1), (0,))), b"chain 1 has fewer than two joints"),
                    (dict(chains=((0, 1), (0, 3))), b"joint 3 of chain 1 outside 0..2"),
                    (dict(chains=((0, 1), (2, 1))), b"chain 1 starts at joint 2, which no earlier chain has placed"),
                    (dict(chains=((0, 1), (0, 1, 2))), b"joint 1 is named twice as a child"),
                    (dict(chains=((0, 1),)), b"joint 2 is named by no chain"),
                    (dict(source=None), b"null gather map or parents"), (dict(parents=None), b"null gather map or parents"),
                    (dict(out_joints=2), b"out_joints 2 outside 3..48"), (dict(out_joints=49), b"out_joints 49 outside 3..48"),
                    (dict(source=(0, 1, 3, 2, 2)), b"out_source[2] = 3 names no joint of 0..2"),
                    (dict(source=(0, 1, -2, 2, 2)), b"out_source[2] = -2 names no joint"),
                    (dict(parents=(-1, 0, 5, 0, 3)), b"out_parents[2] = 5 outside 0..4"),
                    (dict(parents=(-1, 0, -1, 0, 3)), b"out_parents[2] = -1 outside 0..4"),
                    (dict(route=1, out_joints=5), b"route 1 writes the J local quaternions: out_joints 5 != joints 3")):
        assert call(**kw) != 0 and msg in lib.mst_last_error(), (kw, lib.mst_last_error())
