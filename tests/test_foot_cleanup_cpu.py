"""The foot-skate cleanup without a GPU: tests/foot_fixture.py against the reference's recorded outputs (tests/golden/fs.npz, written by
tests/golden/make_golden_fs.py), and everything mst_amd.utils.foot_cleanup refuses before it launches.

In the reference's precision (fp32 arrays, float64 filter) the fixture is BIT-EQUAL to every golden motion, contact array and velocity; its
all-float64 form stays within 1e-6 relative L2 of them.  Every clip the tests use keeps each compared value 10 % of its threshold away from
it (foot_fixture.margins), so no contact bit depends on the precision it is evaluated in."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import foot_fixture as ff
import mst_amd  # noqa: F401
from conftest import GOLDEN, SEED
from mst_amd.utils import foot_cleanup as fc


@pytest.fixture(scope="module")
def fs():
    return np.load(os.path.join(GOLDEN, "fs.npz"))


def stored(fs, T, case, clip):
    """The parts of a cleaned clip fs.npz keeps, next to the golden ones."""
    key = f"T{T}|{case['tag']}"
    mine = [clip[:, list(ff.FID22)], clip[::ff.GOLDEN_EVERY[T]], clip[-1]]
    gold = [fs[f"{key}|feet"], fs[f"{key}|some"], fs[f"{key}|last"]]
    return mine, gold


@pytest.mark.parametrize("T", ff.GOLDEN_T)
def test_fixture_equals_the_reference_outputs(fs, T):
    glb, other = ff.golden_inputs(SEED, T)
    cases = ff.golden_cases(T)
    assert len(cases) == {2: 12, 196: 8}.get(T, 24)
    for case in cases:
        ref = glb if case["ref"] == "self" else other
        got, vels, contacts = ff.remove_fs(glb, ref, ff.FID22, **case["kw"])
        mine, gold = stored(fs, T, case, got)
        for m, g in zip(mine, gold):
            assert m.dtype == np.float32 and np.array_equal(m, g), (T, case["tag"])
        dkey = f"T{T}|{case['det']}|{case['ref']}"
        assert np.array_equal(contacts, fs[f"{dkey}|contacts"]) and np.array_equal(vels, fs[f"{dkey}|vels"]), (T, case["tag"])
        if not case["kw"].get("use_window"):                                   # the last frame is in contact only where the window reaches it
            assert contacts[-1].sum() == 0
        got64, vels64, contacts64 = ff.remove_fs(glb, ref, ff.FID22, dtype=np.float64, **case["kw"])
        assert np.array_equal(contacts64, contacts), (T, case["tag"])
        mine64, _ = stored(fs, T, case, got64)
        dev = ff.rel(np.concatenate([g.reshape(-1) for g in gold]), np.concatenate([m.reshape(-1) for m in mine64]))
        assert dev < 1e-6, (T, case["tag"], dev)
        # both filters leave the last frame as they find it: a joint that is no foot keeps its x and z there
        assert np.array_equal(got[-1, 0, [0, 2]], glb[-1, 0, [0, 2]])


def test_goldens_cover_every_switch(fs):
    tags = [k for k in fs.files if k.endswith("|feet")]
    for word in ("vel3_0.02", "vel3_0.05", "acc|", "acc_win", "floor", "free", "|off|", "|after|", "|both|", "|self|", "|other|"):
        for T in (3, 7, 65, 196):
            assert any(t.startswith(f"T{T}|") and word in t for t in tags), (T, word)
    assert not any(t.startswith("T2|acc") for t in tags)                       # the reference raises there


def test_two_frames_in_vel_acc_mode_have_no_contact():
    glb, _ = ff.golden_inputs(SEED, 2)
    got, vels, contacts = ff.remove_fs(glb, None, ff.FID22)
    assert contacts.shape == (2, 4) and contacts.sum() == 0 and vels.shape == (1, 4)
    want = glb.copy()
    want[:, :, 1] -= glb[..., 1].min()
    assert np.array_equal(got, want)


def test_every_test_clip_keeps_its_margins(fs):
    clips = [c for T in ff.GOLDEN_T for c in ff.golden_inputs(SEED, T)]
    clips.append(ff.make_clip(SEED, "margin/J5", 257, 5, (1, 2, 3, 4)))
    for c in clips:
        fid = ff.FID22 if c.shape[1] == 22 else (1, 2, 3, 4)
        for k, v in ff.margins(c, fid).items():
            assert v >= ff.MARGIN, (c.shape, k, v)
    assert min(json.loads(str(fs["margins"])).values()) >= ff.MARGIN and fs["demo|margins"].min() >= ff.MARGIN


def test_planted_patterns_are_the_vel3_contacts():
    T, L = 257, 5
    for pattern in ("none", "all", "from0", "to_end", "single", "gaps"):
        bits = ff.planted_stance(pattern, T, L)
        stance = np.repeat(bits[:, None], 4, axis=1)
        clip = ff.make_clip(SEED, f"planted/{pattern}", T, 22, ff.FID22, stance)
        for thr in ff.THR3:
            contacts, _ = ff.contacts_vel3(clip, ff.FID22, thr)
            assert np.array_equal(contacts[:-1].astype(bool), stance) and contacts[-1].sum() == 0, (pattern, thr)
    gaps = ff.planted_stance("gaps", T, L).astype(int)
    runs = np.flatnonzero(np.diff(np.concatenate([[0], gaps, [0]])))
    lens = set((runs[2::2] - runs[1:-1:2]).tolist())                            # gap lengths between runs
    assert {L, L + 1, 2 * L, 2 * L + 1} <= lens and runs[0] == L - 1


def test_window_refinement_is_the_last_contact_in_reach():
    """What the kernel relies on: the reference's sequential overwrite gives frame k the verdict of the LAST raw contact frame within three
    frames of it, and leaves k alone when there is none."""
    for T in (3, 7, 65, 196):
        clip, _ = ff.golden_inputs(SEED, T)
        raw, _ = ff.contacts_vel_acc(clip, ff.FID22, use_window=False)
        new, _ = ff.contacts_vel_acc(clip, ff.FID22, use_window=True)
        y = clip[:, list(ff.FID22), 1]
        want = np.zeros_like(raw)
        for i in range(4):
            for k in range(T):
                for g in range(min(k + ff.WINDOW, T - 1), max(k - ff.WINDOW, 0) - 1, -1):
                    if raw[g, i]:
                        want[k, i] = abs(y[k, i] - y[g, i]) < np.float32(ff.HTHR)
                        break
        assert np.array_equal(new, want), T


def test_signature_is_the_reference_signature(fs):
    recorded = json.loads(str(fs["signature"]))
    params = inspect.signature(fc.remove_fs).parameters
    mine = [[n, None if p.default is inspect.Parameter.empty else p.default] for n, p in params.items()
            if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert mine == recorded
    assert [n for n, p in params.items() if p.kind is inspect.Parameter.KEYWORD_ONLY] == ["lengths", "out"]


def test_names_are_resolved_on_a_copy():
    names = list(ff.NAMES22)
    assert fc.ee_ids_by_names(names, ff.EE_NAMES) == list(ff.FID22)
    assert names == ff.NAMES22 and any(":" in n for n in names)                  # the prefixed names are still prefixed
    assert fc.ee_ids_by_names(names) == list(ff.FID22)                           # the reference's default end effectors
    with pytest.raises(ValueError, match="end effector 'Tail' is not among the bone names"):
        fc.ee_ids_by_names(names, ["RightToeBase", "Tail", "LeftFoot", "RightFoot"])


def test_refusals_before_any_launch():
    names = list(ff.NAMES22)
    clip = torch.zeros(1, 8, 22, 3)
    with pytest.raises(IndexError, match="a clip of 1 frame has no velocity"):
        fc.remove_fs("", torch.zeros(1, 1, 22, 3), None, names, ff.EE_NAMES)
    with pytest.raises(IndexError, match="a clip of 1 frame has no velocity"):
        fc.remove_fs("", np.zeros((1, 22, 3), np.float32), np.zeros((1, 22, 3), np.float32), names, ff.EE_NAMES)
    with pytest.raises(ValueError, match="end effector 'Nose' is not among the bone names"):
        fc.remove_fs("", clip, None, names, ["Nose", "LeftToeBase", "LeftFoot", "RightFoot"])
    with pytest.raises(ValueError, match=r"duplicate end-effector ids \[11, 11, 7, 8\]"):
        fc.remove_fs("", clip, None, names, ["RightToeBase", "RightToeBase", "LeftFoot", "RightFoot"])
    with pytest.raises(ValueError, match=r"duplicate end-effector ids"):
        fc.foot_contacts(clip, (1, 2, 2, 3))
    with pytest.raises(ValueError, match=r"end-effector ids \[1, 2, 3, 22\] outside 0\.\.21"):
        fc.foot_contacts(clip, (1, 2, 3, 22))
    for bad in ([1], [9], [0]):
        with pytest.raises(ValueError, match=r"lengths -?\d+\.\.\d+ outside 2\.\.8"):
            fc.remove_fs("", clip, None, names, ff.EE_NAMES, lengths=bad)
    with pytest.raises(ValueError, match="2 lengths for 1 clips"):
        fc.remove_fs("", clip, None, names, ff.EE_NAMES, lengths=[4, 4])
    with pytest.raises(ValueError, match=r"reference motion of shape \(1, 7, 22, 3\)"):
        fc.remove_fs("", clip, torch.zeros(1, 7, 22, 3), names, ff.EE_NAMES)
    with pytest.raises(ValueError, match="mode 'speed' is none of"):
        fc.foot_contacts(clip, ff.FID22, mode="speed")
    # no CPU fallback: a valid call on CPU tensors ends where recover_joints's does
    for call in (lambda: fc.remove_fs("", clip, None, names, ff.EE_NAMES, lengths=[8]),
                 lambda: fc.foot_contacts(clip, ff.FID22, "vel3", 0.05),
                 lambda: fc.clean_joints(torch.zeros(1, 263, 1, 8), np.zeros(263), np.ones(263), 22, ff.FID22)):
        with pytest.raises(RuntimeError, match=r"runs on the GPU only \(no CPU fallback\)"):
            call()


def test_clip_above_the_limit_is_refused_by_name():
    from mst_amd import _native as N
    from mst_amd.utils.motion_process import recover_joints  # noqa: F401
    try:
        lib = N.lib()
    except (RuntimeError, OSError) as e:
        pytest.skip(f"the library does not load here: {e}")
    limit = int(lib.mst_remove_fs_max_frames(22))
    assert limit == fc.max_frames(22) and limit >= 1024
    assert lib.mst_remove_fs_max_frames(0) == -1 and b"joints 0 < 1" in lib.mst_last_error()
    with pytest.raises(RuntimeError, match=rf"{limit + 1} frames > {limit}.*mst_remove_fs_max_frames\(22\)"):
        fc.remove_fs("", torch.zeros(1, limit + 1, 22, 3), None, list(ff.NAMES22), ff.EE_NAMES)
    # the C entry refuses on its own, by name too, before it touches a device
    import ctypes as C
    fid = (C.c_int32 * 4)(*ff.FID22)
    one = C.c_void_p(16)
    args = lambda T, ids: (one, None, 0, None, 1, T, 22, ids, 1, 0.05, 0, 1, 5, 0, 0, one, None, None, None, 0, None)
    assert lib.mst_remove_fs(*args(limit + 1, fid)) != 0
    assert f"mst_remove_fs: frames {limit + 1} > {limit}".encode() in lib.mst_last_error()
    assert lib.mst_remove_fs(*args(1, fid)) != 0 and b"frames 1 < 2" in lib.mst_last_error()
    assert lib.mst_remove_fs(*args(8, (C.c_int32 * 4)(1, 2, 2, 3))) != 0 and b"duplicate foot id 2" in lib.mst_last_error()
    assert lib.mst_remove_fs(*args(8, (C.c_int32 * 4)(1, 2, 3, 22))) != 0 and b"foot id 22 outside 0..21" in lib.mst_last_error()


def test_demo_composition_on_the_oracle_joints(fs):
    """recover_from_ric (the fp32 oracle) and two passes in the fixture, against the reference's recorded result: the same contacts (the
    margins hold for both passes' inputs), so a deviation of fp32 rounding size."""
    from oracle import postprocess
    sample, mean, std, content = ff.demo_inputs(SEED, int(fs["demo|variant"]))
    joints = np.asarray(postprocess.recover_joints(sample, mean, std, 22))[:, 0, :ff.DEMO_LEN]
    got = ff.demo_passes(joints, content[None, :ff.DEMO_LEN], ff.FID22)[0]
    assert got.shape == fs["demo|out"].shape == (ff.DEMO_LEN, 22, 3)
    assert ff.rel(got, fs["demo|out"]) < 1e-6
    assert float(fs["ref_seconds_per_clip"]) > 0
