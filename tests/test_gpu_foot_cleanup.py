"""k_remove_fs (csrc/mst_feet.h) through mst_amd.utils.foot_cleanup: against the reference's recorded outputs (tests/golden/fs.npz) and
against the float64 form of tests/foot_fixture.py at the shapes where the kernel's loops change path.

  goldens       J = 22, T in {2, 3, 7, 65, 196}: both detectors, use_window, force_on_floor, the filter off / after / before and after,
                vel3_thr 0.02 and 0.05, contacts detected on the clip itself and on a second clip
  shapes        T in {2, 3, 255, 256, 257, 1024} (the 256-thread strides, the 8-step chunks of the filter) x J in {5, 21, 22}, interp_length
                in {1, 5, 9}; a planted clip and a random one per call
  patterns      no contact, all, a run from frame 0, a run ending at len-2, one-frame runs, gaps of L, L+1, 2L, 2L+1 frames between runs,
                gaps shorter than L at both ends -- contacts asserted equal to the planted bits
  batch         mixed lengths including 2 and T, frames from len on untouched, B = 5 equal to five single calls
  equivalences  ref=None / ref=clone, in place / out of place, clean_joints / recover_joints + two calls, numpy / tensor: torch.equal
  demo          clean_joints on the seeded (263, 1, 196) sample against the reference's composition

Bars.  Per case the fixture is evaluated in the reference's precision (fp32, float64 filter) and in float64 on the same inputs; the
kernel's distance from the float64 result may be 4 x the distance between the two, and not below 1e-6 (the rule of
tests/test_gpu_glue_shapes.py).  Contacts, pass-through frames, the last frame (which neither filter touches) and the equivalences are
exact.  Every clip keeps each compared value 10 % of its threshold away from it (foot_fixture.margins; asserted here for the clips built
here), so a contact bit cannot flip with the precision.  Every case prints `feet: <case> ref <dev> got <dev> bar <bar>`.
Operands sit in front of a NaN-filled guard: a loop that runs past a clip reads NaN.

Worst figures measured on an MI355X, fp32 fixture / kernel / bar (the table is in DESIGN.md section 5): goldens 4.6e-8 / 4.6e-8 / 1e-6
(6.0e-8 with the recorded values as the fp32 side); T = 2: 2.2e-8, T = 3: 3.7e-8, T = 255 / 256 / 257: 5.5e-8 / 5.3e-8 / 5.6e-8,
T = 1024: 5.9e-8, planted patterns 6.4e-8, mixed lengths 2.9e-8 -- the kernel's figure equal to the fixture's in each; the demo's
composition 6.1e-8 / 5.9e-8 / 1e-6.  mst_remove_fs_max_frames(22) = 4096."""
import os

import numpy as np
import pytest
import torch

import foot_fixture as ff
import glue_fixture as gf
import mst_amd  # noqa: F401
from conftest import GOLDEN, SEED
from mst_amd.utils import foot_cleanup as fc
from mst_amd.utils.motion_process import recover_joints

pytestmark = pytest.mark.gpu
GUARD = 4096
NAMES = list(ff.NAMES22)
PATTERNS = ("none", "all", "from0", "to_end", "single", "gaps")


def dev():
    return torch.device("cuda:0")


def guarded(values, dtype=torch.float32):
    """`values` on the GPU as a view of a buffer whose next GUARD elements are NaN (or, for integers, huge)."""
    v = torch.from_numpy(np.ascontiguousarray(values)).to(dtype)
    fill = float("nan") if dtype.is_floating_point else 2 ** 30
    buf = torch.full((v.numel() + GUARD,), fill, dtype=dtype, device=dev())
    buf[:v.numel()] = v.reshape(-1).to(dev())
    return buf[:v.numel()].view(v.shape)


def report(case, ref, got, bar):
    print(f"feet: {case} ref {ref:.3e} got {got:.3e} bar {bar:.3e}")


@pytest.fixture(scope="module")
def fs():
    return np.load(os.path.join(GOLDEN, "fs.npz"))


def names_for(J, fid):
    names = [f"bone{j}" for j in range(J)]
    for n, j in zip(ff.EE_NAMES, fid):
        names[j] = "rig:" + n
    return names


def run_case(tag, glb, ref, fid, lengths=None, **kw):
    """One launch on [B, T, J, 3] host arrays against the fixture in both precisions.  -> (cleaned clip on the host, contacts)."""
    B, T, J, _ = glb.shape
    want, wvels, wcontacts = ff.remove_fs_batch(glb, ref, fid, lengths, dtype=np.float64, **kw)
    mine, mvels, mcontacts = ff.remove_fs_batch(glb, ref, fid, lengths, dtype=np.float32, **kw)
    assert np.array_equal(wcontacts, mcontacts), tag
    g = guarded(glb)
    got, vels, contacts, butter = fc.remove_fs("", g, None if ref is None else guarded(ref), names_for(J, fid), ff.EE_NAMES,
                                               lengths=lengths, **kw)
    assert torch.equal(g.cpu(), torch.from_numpy(glb))                                         # the input is left alone
    assert torch.equal(butter.cpu(), torch.from_numpy(glb if ref is None else ref))
    got, vels, contacts = got.cpu().numpy(), vels.cpu().numpy(), contacts.cpu().numpy()
    assert contacts.dtype == np.int32 and np.array_equal(contacts, wcontacts), tag
    assert np.isfinite(got).all() and np.isfinite(vels).all(), tag
    assert ff.rel(vels, wvels) <= 1e-6, tag
    ref_dev, e = ff.rel(mine, want), ff.rel(got, want)
    report(tag, ref_dev, e, ff.bar(ref_dev))
    assert e <= ff.bar(ref_dev), tag
    for b in range(B):
        n = T if lengths is None else int(lengths[b])
        assert np.array_equal(got[b, n:], glb[b, n:]), tag                                     # frames from len on: bit for bit
        if not kw.get("use_butterworth"):
            assert np.array_equal(got[b, n - 1], mine[b, n - 1]), tag                          # no filter touches the last valid frame
        else:                                  # the filter in front moves the floor by its own rounding; x and z of the frame stay exact
            assert np.array_equal(got[b, n - 1][:, [0, 2]], mine[b, n - 1][:, [0, 2]]), tag
    return got, contacts


# ------------------------------------------------------------------------------------------ the reference's recorded outputs
@pytest.mark.parametrize("T", ff.GOLDEN_T)
def test_against_the_reference_outputs(fs, T):
    glb, other = ff.golden_inputs(SEED, T)
    every = ff.GOLDEN_EVERY[T]
    for case in ff.golden_cases(T):
        ref = glb if case["ref"] == "self" else other
        tag = f"golden T{T} {case['tag']}"
        got, contacts = run_case(tag, glb[None], ref[None], ff.FID22, **case["kw"])
        key, dkey = f"T{T}|{case['tag']}", f"T{T}|{case['det']}|{case['ref']}"
        assert np.array_equal(contacts[0], fs[f"{dkey}|contacts"]), tag
        want64 = ff.remove_fs(glb, ref, ff.FID22, dtype=np.float64, **case["kw"])[0]
        parts = lambda c: np.concatenate([c[:, list(ff.FID22)].reshape(-1), c[::every].reshape(-1), c[-1].reshape(-1)])
        gold = np.concatenate([fs[f"{key}|{p}"].reshape(-1) for p in ("feet", "some", "last")])
        ref_dev = ff.rel(gold, parts(want64))
        e, e_gold = ff.rel(parts(got[0]), parts(want64)), ff.rel(parts(got[0]), gold)
        report(tag + " (recorded)", ref_dev, e, ff.bar(ref_dev))
        print(f"feet: {tag} rows differing from the recorded ones: {int((parts(got[0]) != gold).sum())} of {gold.size} values")
        assert e <= ff.bar(ref_dev) and e_gold <= ff.bar(ref_dev), tag
        if not case["kw"].get("use_butterworth"):
            assert np.array_equal(got[0, -1], fs[f"{key}|last"]), tag


# ------------------------------------------------------------------------------------------ shapes
SHAPE_T = (2, 3, 255, 256, 257, 1024)
SHAPE_J = {5: (1, 2, 3, 4), 21: (10, 9, 6, 7), 22: ff.FID22}


@pytest.mark.parametrize("J", sorted(SHAPE_J))
@pytest.mark.parametrize("T", SHAPE_T)
def test_frame_and_joint_counts(T, J):
    fid = SHAPE_J[J]
    L = (1, 5, 9)[(SHAPE_T.index(T) + sorted(SHAPE_J).index(J)) % 3]
    pattern = "gaps" if T > 100 else ("all" if J == 21 else "from0")
    planted = np.repeat(ff.planted_stance(pattern, T, L)[:, None], 4, axis=1)
    glb = np.stack([ff.make_clip(SEED, f"shape/T{T}_J{J}/planted", T, J, fid, planted),
                    ff.make_clip(SEED, f"shape/T{T}_J{J}/random", T, J, fid)])
    other = ff.make_clip(SEED, f"shape/T{T}_J{J}/other", T, J, fid)[None]
    for c in (*glb, other[0]):
        assert min(ff.margins(c, fid).values()) >= ff.MARGIN
    tag = f"shape T{T} J{J} L{L}"
    _, contacts = run_case(tag + " vel3 self floor after", glb, None, fid, interp_length=L, use_vel3=True, vel3_thr=0.05,
                           force_on_floor=True, after_butterworth=True)
    assert np.array_equal(contacts[0, :-1].astype(bool), planted)
    run_case(tag + " vel3 other free off", glb, other, fid, interp_length=L, use_vel3=True, vel3_thr=0.02)
    run_case(tag + " acc_win other free both", glb, other, fid, interp_length=L, use_window=True, use_butterworth=True,
             after_butterworth=True)
    run_case(tag + " acc self floor off", glb, None, fid, interp_length=L, force_on_floor=True)


@pytest.mark.parametrize("L", (1, 5, 9))
def test_planted_contact_patterns(L):
    T, J, fid = 257, 22, ff.FID22
    bits = [np.repeat(ff.planted_stance(p, T, L)[:, None], 4, axis=1) for p in PATTERNS]
    glb = np.stack([ff.make_clip(SEED, f"pattern/{p}", T, J, fid, b) for p, b in zip(PATTERNS, bits)])
    for force in (False, True):
        got, contacts = run_case(f"patterns L{L} {'floor' if force else 'free'}", glb, None, fid, interp_length=L, use_vel3=True,
                                 vel3_thr=0.05, force_on_floor=force)
        for k, p in enumerate(PATTERNS):
            assert np.array_equal(contacts[k, :-1].astype(bool), bits[k]) and contacts[k, -1].sum() == 0, p
        floor = glb[0, :, :, 1].min()
        want = glb[0].copy()
        want[:, :, 1] -= floor
        assert np.array_equal(got[0], want)                                    # no contact: the floor shift and nothing else
        feet = got[1][:-1, list(fid)]
        assert np.array_equal(feet, np.broadcast_to(feet[:1], feet.shape))     # all frames one run: every frame holds the mean
        if force:
            assert float(np.abs(feet[..., 1]).max()) == 0.0


# ------------------------------------------------------------------------------------------ batch
def test_mixed_lengths_and_independence_of_the_neighbours():
    T, J, fid = 65, 22, ff.FID22
    lengths = [2, 65, 33, 3, 64]
    glb = np.stack([ff.make_clip(SEED, f"batch/{b}", T, J, fid) for b in range(5)])
    other = np.stack([ff.make_clip(SEED, f"batch/other{b}", T, J, fid) for b in range(5)])
    kws = [dict(use_vel3=True, vel3_thr=0.05, force_on_floor=True, after_butterworth=True),
           dict(use_window=True, use_butterworth=True, after_butterworth=True)]
    for i, kw in enumerate(kws):
        run_case(f"batch mixed lengths cfg{i} self", glb, None, fid, lengths, **kw)
        run_case(f"batch mixed lengths cfg{i} other", glb, other, fid, lengths, **kw)
        run_case(f"batch mixed lengths cfg{i} one reference", glb, other[:1], fid, lengths, **kw)
        g, o = guarded(glb), guarded(other)
        ld = guarded(np.array(lengths, np.int32), torch.int32)
        whole = fc.remove_fs("", g, o, NAMES, ff.EE_NAMES, lengths=ld, **kw)
        for b in range(5):
            single = fc.remove_fs("", g[b:b + 1], o[b:b + 1], NAMES, ff.EE_NAMES, lengths=[lengths[b]], **kw)
            for w, s in zip(whole, single):
                assert torch.equal(w[b:b + 1], s), (i, b)
            assert torch.equal(whole[0][b, lengths[b]:], g[b, lengths[b]:])
            assert int(whole[2][b, lengths[b] - 1:].sum()) == 0 or kw.get("use_window")
            assert float(whole[1][b, lengths[b] - 1:].abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------ equivalences
def test_equivalent_calls_are_bit_equal(fs):
    T, J, fid = 196, 22, ff.FID22
    glb = np.stack([ff.make_clip(SEED, f"equiv/{b}", T, J, fid) for b in range(2)])
    kw = dict(use_vel3=True, vel3_thr=0.05, force_on_floor=True, after_butterworth=True)
    g = guarded(glb)
    base = fc.remove_fs("", g, None, NAMES, ff.EE_NAMES, lengths=[196, 120], **kw)
    # the clip itself, spelled three ways
    for ref in (g, g.clone()):
        for a, b in zip(base, fc.remove_fs("", g, ref, NAMES, ff.EE_NAMES, lengths=[196, 120], **kw)):
            assert torch.equal(a, b)
    # in place
    h = guarded(glb)
    res = fc.remove_fs("", h, None, NAMES, ff.EE_NAMES, lengths=[196, 120], out=h, **kw)
    assert res[0].data_ptr() == h.data_ptr()
    for a, b in zip(base, res):
        assert torch.equal(a, b)
    assert torch.equal(res[3].cpu(), torch.from_numpy(glb))                    # butter_motion: the clip as it was on entry
    h = guarded(glb)
    for a, b in zip(fc.remove_fs("", g, g.clone(), NAMES, ff.EE_NAMES, use_window=True, use_butterworth=True),
                    fc.remove_fs("", h, None, NAMES, ff.EE_NAMES, use_window=True, use_butterworth=True, out=h)):
        assert torch.equal(a, b)
    # numpy in, numpy out
    outs = fc.remove_fs("", glb[1][:120], glb[1][:120], NAMES, ff.EE_NAMES, **kw)
    assert all(isinstance(o, np.ndarray) for o in outs) and outs[0].shape == (120, J, 3) and outs[2].dtype == np.int32
    assert np.array_equal(outs[0], base[0][1, :120].cpu().numpy()) and np.array_equal(outs[1], base[1][1, :119].cpu().numpy())
    assert np.array_equal(outs[2], base[2][1, :120].cpu().numpy()) and np.array_equal(outs[3], glb[1][:120])
    # foot_contacts: the detector alone
    for mode, thr, win in (("vel3", 0.05, False), ("vel_acc", 0.003, False), ("vel_acc", 0.003, True)):
        c, v = fc.foot_contacts(g, fid, mode, thr, use_window=win, lengths=[196, 120])
        full = fc.remove_fs("", g, None, NAMES, ff.EE_NAMES, use_vel3=mode == "vel3", vel3_thr=thr, use_window=win, lengths=[196, 120])
        assert torch.equal(c, full[2]) and torch.equal(v, full[1])
    # clean_joints = recover_joints + the demo's two calls
    sample, mean, std, content = ff.demo_inputs(SEED, int(fs["demo|variant"]))
    s, c = guarded(np.concatenate([sample, sample[:, :, :, ::-1]])), guarded(content[None])
    lengths = [ff.DEMO_LEN, 196]
    joints = recover_joints(s, mean, std, J)[:, 0]
    p1 = fc.remove_fs("", joints, c, NAMES, ff.EE_NAMES, lengths=lengths, **kw)[0]
    p2 = fc.remove_fs("", p1, p1, NAMES, ff.EE_NAMES, lengths=lengths, **kw)[0]
    assert torch.equal(fc.clean_joints(s, mean, std, J, fid, ref_joints=c, lengths=lengths), p2)
    assert torch.equal(fc.clean_joints(s, mean, std, J, fid, lengths=lengths, passes=1),
                       fc.remove_fs("", joints, None, NAMES, ff.EE_NAMES, lengths=lengths, **kw)[0])


# ------------------------------------------------------------------------------------------ the demo's composition
def test_clean_joints_against_the_reference_composition(fs):
    sample, mean, std, content = ff.demo_inputs(SEED, int(fs["demo|variant"]))
    n = ff.DEMO_LEN
    got = fc.clean_joints(guarded(sample), mean, std, 22, ff.FID22, ref_joints=guarded(content[None]), lengths=[n])
    assert tuple(got.shape) == (1, 196, 22, 3)
    joints64 = gf.recover_joints(sample, mean, std, 22)[:, 0]
    want = ff.demo_passes(joints64[:, :n], content[None, :n], ff.FID22, dtype=np.float64)[0]
    gold = fs["demo|out"]
    ref_dev, e = ff.rel(gold, want), ff.rel(got[0, :n], want)
    report("demo clean_joints 263x1x196 len 180", ref_dev, e, ff.bar(ref_dev))
    assert e <= ff.bar(ref_dev) and ff.rel(got[0, :n], gold) <= ff.bar(ref_dev)
    assert torch.equal(got[0, n:], recover_joints(guarded(sample), mean, std, 22)[0, 0, n:])


# ------------------------------------------------------------------------------------------ the limit
def test_a_clip_above_the_limit_is_refused_before_any_launch():
    limit = fc.max_frames(22)
    from mst_amd import _native as N
    print(f"feet: mst_remove_fs_max_frames(22) = {limit}, mst_recover_max_frames() = {int(N.lib().mst_recover_max_frames())}")
    assert limit >= int(N.lib().mst_recover_max_frames())
    x = torch.zeros(1, limit + 1, 22, 3, device=dev())
    with pytest.raises(RuntimeError, match=rf"{limit + 1} frames > {limit}.*mst_remove_fs_max_frames\(22\)"):
        fc.remove_fs("", x, None, NAMES, ff.EE_NAMES)
    with pytest.raises(RuntimeError, match=rf"{limit + 1} frames > {limit}.*mst_remove_fs_max_frames\(22\)"):
        fc.foot_contacts(x, ff.FID22, "vel3", 0.05)
