"""The motion encoder without a GPU: tests/encode_fixture.py against the reference's recorded outputs (tests/golden/encode.npz), its
161-tap filter against a direct clamped-index sum, every refusal of the Python layer (raised before any GPU call), the drop-in signatures,
and the C ABI's declarations and refusals.

The golden bar is the suite's rule: the float32 fixture's distance from the float64 fixture, times 4, floor 1e-6.  Every case prints
`encode: <case> <output> ref <dev> got <dev> bar <bar>`, where `got` is the recorded reference output against the float64 fixture."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import encode_fixture as ef
import mst_amd  # noqa: F401
from conftest import GOLDEN, ROOT, SEED
from mst_amd.utils import joint_fit as jf
from mst_amd.utils import motion_process as mp

NAMES = ("data", "global_positions", "positions", "l_velocity")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "encode.npz"))


def four(m):
    return m["sample"][0, :, 0].T, m["global_positions"][0], m["positions"][0], m["l_velocity"][0]


@pytest.mark.parametrize("mode,J,T", ef.GOLDEN_CASES)
def test_the_fixture_against_the_reference_outputs(gold, mode, J, T):
    sk, pos, rot = ef.golden_inputs(SEED, mode, J, T)
    keep = pos.copy(), rot.copy()
    m32, _ = ef.encode(pos[None], rot[None], sk, mode, np.float32, frames_out=T - 1)
    m64, diags = ef.encode(pos[None], rot[None], sk, mode, np.float64, frames_out=T - 1)
    ef.assert_clear(diags, mode)
    assert np.array_equal(pos, keep[0]) and np.array_equal(rot, keep[1])                     # the fixture leaves its inputs alone
    key = f"{mode}|J{J}T{T}"
    assert m64["sample"].shape == (1, ef.feats(J, mode), 1, T - 1) and m64["lengths"][0] == T - 1
    for name, a32, a64 in zip(NAMES, four(m32), four(m64)):
        fr = ef.golden_frames(name, len(a64))
        r = gold[f"{key}|{name}"]
        own, e = ef.rel(a32[fr], a64[fr]), ef.rel(r, a64[fr])
        print(f"encode: fixture {key} {name} ref {own:.3e} got {e:.3e} bar {ef.bar(own):.3e}")
        assert r.shape == a64[fr].shape and e <= ef.bar(own), (key, name)
    if mode == ef.HML:
        assert np.array_equal(gold[f"{key}|data"][:, -4:], four(m32)[0][:, -4:])             # contacts: exact
        assert np.array_equal(gold[f"{key}|data"][:, -4:], four(m64)[0][:, -4:])
    r32, r64 = ef.recover_from_ric(four(m32)[0], J, np.float32), ef.recover_from_ric(four(m64)[0], J, np.float64)
    fr = ef.golden_frames("recover", T - 1)
    own, e = ef.rel(r32[fr], r64[fr]), ef.rel(gold[f"{key}|recover"], r64[fr])
    print(f"encode: fixture {key} recover ref {own:.3e} got {e:.3e} bar {ef.bar(own):.3e}")
    assert e <= ef.bar(own)
    assert np.abs(r64 - four(m64)[1][:-1]).max() <= 1e-12                                   # the round trip is exact in exact arithmetic
    assert float(gold[f"{key}|seconds"]) > 0


@pytest.mark.parametrize("n", (2, 80, 81, 161, 162))
def test_the_filter_against_a_direct_sum(n):
    x = ef.syn.normal(SEED, f"enc/cpu/filter{n}", (n, 3)).astype(np.float64)
    w = ef.taps()
    assert w.shape == (161,) and abs(w.sum() - 1) < 1e-15 and np.array_equal(w, w[::-1]) and w.argmax() == 80
    want = np.zeros((n, 3))
    for t in range(n):
        for k in range(-80, 81):
            want[t] += w[k + 80] * x[min(max(t + k, 0), n - 1)]
    got = ef.smooth(x, np.float64)
    assert np.abs(got - want).max() <= 1e-14
    got32 = ef.smooth(x, np.float32)
    assert got32.dtype == np.float32 and np.abs(got32 - want).max() <= 2e-5
    try:
        from scipy.ndimage import gaussian_filter1d
    except ImportError:
        return
    assert np.abs(gaussian_filter1d(x, 20, axis=0, mode="nearest") - want).max() <= 1e-14


def test_lengths_mean_std_and_cut_in_the_fixture():
    sk = ef.skeleton(SEED, 5)
    pos, rot = ef.make_clip(SEED, "enc/cpu/lengths", 9, sk, ef.HML, B=3, lengths=[2, 9, 6])
    F = ef.feats(5, ef.HML)
    mean, std = 0.1 * ef.syn.normal(SEED, "enc/cpu/mean", (F,)), 0.5 + ef.syn.uniform01(SEED, "enc/cpu/std", F)
    m, diags = ef.encode(pos, rot, sk, ef.HML, np.float64, lengths=[2, 9, 6], mean=mean, std=std, frames_out=6)
    ef.assert_clear(diags, ef.HML)
    assert list(m["lengths"]) == [1, 6, 5] and m["sample"].shape == (3, F, 1, 6)
    assert not m["sample"][0, :, 0, 1:].any() and not m["sample"][2, :, 0, 5:].any() and m["sample"][1, :, 0, 5].any()
    single, _ = ef.encode(pos[2:, :6], rot[2:, :6], sk, ef.HML, np.float64, frames_out=6)
    assert np.allclose(m["sample"][2, :, 0, :5], ((single["sample"][0, :, 0, :5].T - mean) / std).T, rtol=0, atol=1e-12)
    # the mid-tree chain: restarting from the root quaternion is not accumulating down the tree
    other, _ = ef.encode(pos, rot, sk, ef.HML, np.float64, lengths=[2, 9, 6], restart=False)
    plain, _ = ef.encode(pos, rot, sk, ef.HML, np.float64, lengths=[2, 9, 6])
    R0 = 4 + 3 * 4
    col = slice(R0 + 6 * 3, R0 + 6 * 4)                                                     # joint 4, the child of the chain [1, 4]
    assert ef.rel(other["sample"][:, col], plain["sample"][:, col]) > 1e-2
    assert np.array_equal(np.delete(other["sample"], np.r_[col], 1), np.delete(plain["sample"], np.r_[col], 1))


# ------------------------------------------------------------------------------------------ refusals
def cpu_args(J=5, T=4, B=1, mode=ef.HML):
    sk = ef.skeleton(SEED, J)
    pos, rot = ef.make_clip(SEED, f"enc/cpu/args{J}", T, sk, mode, B=B)
    return sk, torch.from_numpy(pos), torch.from_numpy(rot)


def test_everything_is_refused_before_any_gpu_is_touched():
    sk, pos, rot = cpu_args()
    kw = sk.kw()
    enc = mp.encode_joints
    with pytest.raises(TypeError, match="positions and rotations are tensors"):
        enc(pos.numpy(), **kw)
    with pytest.raises(ValueError, match=r"expected \[B, T, J, 3\]"):
        enc(pos[0], **kw)
    with pytest.raises(IndexError, match="a clip of 1 frame has no velocity row"):
        enc(pos[:, :1], **kw)
    with pytest.raises(ValueError, match="25 joints outside 2..24"):
        enc(torch.zeros(1, 3, 25, 3), **kw)
    with pytest.raises(ValueError, match="1 joints outside 2..24"):
        enc(torch.zeros(1, 3, 1, 3), **kw)
    with pytest.raises(ValueError, match="mode 'posrot' needs the rotations"):
        enc(pos, mode="posrot", **kw)
    with pytest.raises(ValueError, match="mode 'xyz' is none of"):
        enc(pos, mode="xyz", **kw)
    with pytest.raises(ValueError, match="rotations of shape"):
        enc(pos, rot[:, :2], **kw)
    for face, msg in (((1, 3, 4), "four face joints"), ((1, 3, 4, 5), r"outside 0\.\.4"), ((1, -1, 4, 2), r"outside 0\.\.4"),
                      ((1, 3, 1, 2), "duplicate face joints")):
        with pytest.raises(ValueError, match=msg):
            enc(pos, **dict(kw, face_joint_indx=face))
    with pytest.raises(ValueError, match=r"foot joints \[3, 2, 1, 5\] outside"):
        enc(pos, **dict(kw, fid_r=(1, 5)))
    with pytest.raises(ValueError, match="two foot joints a side"):
        enc(pos, **dict(kw, fid_l=(1,)))
    for chains, msg in (([[0, 1, 2], [3, 4]], "chain 1 starts at joint 3, which no earlier chain has placed"),
                        ([[0, 1, 2], [0, 3], [1, 2]], r"joint 2 is named twice as a child \(chain 2\)"),
                        ([[0, 1, 0]], "joint 0 is named twice as a child"), ([[0, 1, 7]], "chain 0 names a joint outside"),
                        ([[0, 1], []], "chain 1 is empty"), ([], "needs the kinematic chains")):
        with pytest.raises(ValueError, match=msg):
            enc(pos, **dict(kw, chains=chains))
    with pytest.raises(ValueError, match="raw offsets of shape"):
        enc(pos, **dict(kw, raw_offsets=sk.raw[:4]))
    with pytest.raises(ValueError, match="needs the raw offsets"):
        enc(pos, **dict(kw, raw_offsets=None))
    F = ef.feats(5, ef.HML)
    with pytest.raises(ValueError, match="mean and std come together"):
        enc(pos, mean=np.zeros(F), **kw)
    with pytest.raises(ValueError, match=rf"std of shape \({F - 1},\), expected \({F},\)"):
        enc(pos, mean=np.zeros(F), std=np.ones(F - 1), **kw)
    with pytest.raises(ValueError, match=r"mean of shape \(59,\), expected \(46,\)"):          # POSROT has its own width
        enc(pos, rot, mean=np.zeros(F), std=np.ones(F), **kw)
    with pytest.raises(ValueError, match="frames_out 0 < 1"):
        enc(pos, frames_out=0, **kw)
    with pytest.raises(ValueError, match=r"lengths 1\.\.1 outside 2\.\.4"):
        enc(pos, lengths=[1], **kw)
    with pytest.raises(ValueError, match=r"lengths 5\.\.5 outside 2\.\.4"):
        enc(pos, lengths=torch.tensor([5]), **kw)
    with pytest.raises(ValueError, match="2 lengths for 1 clips"):
        enc(pos, lengths=[2, 3], **kw)
    limit = mp.encode_max_frames(5, "hml")
    assert limit >= 197 and mp.encode_max_frames(24, "posrot") >= 197
    with pytest.raises(RuntimeError, match=rf"{limit + 1} frames > {limit}.*mst_encode_max_frames\(5, 'hml'\)"):
        enc(torch.zeros(1, limit + 1, 5, 3), **kw)
    # everything in order, but on the CPU
    for call in (lambda: enc(pos, **kw), lambda: enc(pos, rot, lengths=[3], **kw)):
        with pytest.raises(RuntimeError, match="encode_joints runs on the GPU only"):
            call()
    fit = jf.JointFit(*(torch.zeros(1) for _ in range(4)), rot)
    with pytest.raises(RuntimeError, match="encode_joints runs on the GPU only"):
        jf.encode_fit(pos, fit, chains=sk.chains, face_joint_indx=sk.face, fid_l=sk.fid_l, fid_r=sk.fid_r)
    with pytest.raises(TypeError, match="fit is the JointFit"):
        jf.encode_fit(pos, rot, chains=sk.chains, face_joint_indx=sk.face, fid_l=sk.fid_l, fid_r=sk.fid_r)
    with pytest.raises(ValueError, match=r"process_file: positions of shape \(1, 4, 5, 3\), expected one clip"):
        mp.process_file(pos.numpy(), sk.face, sk.fid_l, sk.fid_r, 0.002, sk.raw, sk.chains)
    with pytest.raises(ValueError, match="process_file_with_rotation: rotations of shape"):
        mp.process_file_with_rotation(pos[0].numpy(), rot[0, :2].numpy(), sk.face, sk.fid_l, sk.fid_r, 0.002, sk.raw, sk.chains)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="process_file runs on the GPU only"):
            mp.process_file(pos[0].numpy(), sk.face, sk.fid_l, sk.fid_r, 0.002, sk.raw, sk.chains)


def test_the_drop_in_signatures():
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(mp.process_file_with_rotation) == ["positions", "rotations", "face_joint_indx", "fid_l", "fid_r", "feet_thre",
                                                    "n_raw_offsets", "kinematic_chain"]
    assert names(mp.process_file) == ["positions", "face_joint_indx", "fid_l", "fid_r", "feet_thre", "n_raw_offsets", "kinematic_chain"]
    sig = inspect.signature(mp.encode_joints)
    assert names(mp.encode_joints)[:2] == ["positions", "rotations"] and sig.parameters["rotations"].default is None
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names(mp.encode_joints)[2:])
    assert sig.parameters["feet_thre"].default == 0.002 and sig.parameters["return_aux"].default is False
    assert names(jf.encode_fit)[:2] == ["joints", "fit"]
    assert mp.encode_feats(22, "hml") == 263 and mp.encode_feats(20, "posrot") == 181 and mp.encode_feats(21, "posrot") == 190


def test_the_c_abi_declares_exports_and_refuses():
    from mst_amd import _native as N
    text = open(os.path.join(ROOT, "include", "mst_engine.h")).read()
    lib = N.lib()
    for name in ("mst_encode_motion", "mst_encode_max_frames"):
        assert name in N.SIGNATURES and re.search(rf"\bint {name}\(", text) and hasattr(lib, name)
    decl = re.search(r"\bint mst_encode_motion\((.*?)\);", text, flags=re.S).group(1)
    assert len(decl.split(",")) == len(N.SIGNATURES["mst_encode_motion"][1]) == 23
    for J in (2, 20, 24):
        for mode in (0, 1):
            assert lib.mst_encode_max_frames(J, mode) >= 197
    assert lib.mst_encode_max_frames(1, 0) == -1 and b"joints 1 outside 2..24" in lib.mst_last_error()
    assert lib.mst_encode_max_frames(25, 1) == -1 and lib.mst_encode_max_frames(5, 2) == -1

    one = C.c_void_p(8)                                    # never dereferenced: every case is refused before a launch

    def call(joints=5, frames=4, mode=1, rot=None, mean=None, std=None, face=(1, 3, 4, 2), feet=(3, 2, 1, 4),
             chains=((0, 1, 2), (0, 3), (1, 4)), frames_out=4, raw=True):
        flat = [j for c in chains for j in c]
        starts = [0]
        for c in chains:
            starts.append(starts[-1] + len(c))
        ints = lambda v: (C.c_int32 * max(len(v), 1))(*v)
        off = (C.c_float * (3 * 24))() if raw else None
        return lib.mst_encode_motion(one, rot, None, mean, std, 1, frames, joints, mode, ints(face), ints(feet), ints(flat), ints(starts),
                                     len(chains), off, 0.002, frames_out, one, one, None, None, None, None)

    for kw, msg in ((dict(frames=1), b"frames 1 < 2"), (dict(joints=1), b"joints 1 outside 2..24"), (dict(joints=25), b"joints 25 outside"),
                    (dict(mode=2), b"mode 2 is neither"), (dict(frames_out=0), b"frames_out 0 < 1"),
                    (dict(frames=lib.mst_encode_max_frames(5, 1) + 1), b"(mst_encode_max_frames)"),
                    (dict(mode=0), b"POSROT needs the rotations"), (dict(mean=one), b"mean and std come together"),
                    (dict(std=one), b"mean and std come together"), (dict(face=(1, 3, 4, 5)), b"face joint 5 outside 0..4"),
                    (dict(face=(1, 3, 3, 2)), b"duplicate face joint 3"), (dict(feet=(3, 2, 1, -1)), b"foot joint -1 outside"),
                    (dict(chains=((0, 1, 2), (3, 4))), b"chain 1 starts at joint 3, which no earlier chain has placed"),
                    (dict(chains=((0, 1, 2), (0, 3), (1, 2))), b"joint 2 is named twice as a child"),
                    (dict(chains=((0, 1, 9),)), b"joint 9 of chain 0 outside"), (dict(chains=()), b"HML needs"),
                    (dict(raw=False), b"HML needs")):
        assert call(**kw) != 0 and msg in lib.mst_last_error(), (kw, lib.mst_last_error())
