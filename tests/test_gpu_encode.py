"""k_encode (csrc/mst_encode.h) through mst_amd.utils.motion_process.encode_joints, its drop-ins and joint_fit.encode_fit: against the
reference's recorded outputs (tests/golden/encode.npz) and against the float64 form of tests/encode_fixture.py at the shapes where the
kernel changes path.

  goldens       process_file_with_rotation at (J 20, T 76) and (J 21, T 197), process_file at (J 22, T 197) and (J 22, T 5)
  shapes        both modes; len in {2, 3, 63, 64, 65, 80, 81, 161, 162, 197} (one output row, the 64-lane edge, clips shorter than, equal
                to and just past the filter's radius and width); J in {5, 20, 21, 22, 24}; B in {1, 3}
  lengths       mixed, including 2 and T; B = 3 equals three single calls; rows from len - 1 on exactly 0.0 with mean / std;
                frames_out above T - 1, equal to it, and below len - 1 (cut)
  equivalences  mean / std against (plain - mean) / std; the same call twice, encode_fit, the drop-ins: torch.equal
  round trip    recover_joints(encode_joints(x)) against the global_positions output; the recorded recover_from_ric against the kernel's
  chains        on the J = 5 tree the mid-tree chain restarts from the root quaternion, as in the reference; a joint no chain names; a
                zero raw offset gives NaN in the columns where the reference has it

Bars.  Per case the fixture is evaluated in float32 and in float64 on the same inputs; per output the kernel's distance from the float64
result may be 4 x the distance between the two, and not below 1e-6 (the rule of tests/test_gpu_glue_shapes.py and test_gpu_joint_fit.py).
Contacts, padded rows and output lengths are exact.  Every case prints `encode: <case> <output> ref <dev> got <dev> bar <bar>`.  Operands
sit in front of a NaN-filled guard: a loop that runs past a clip reads NaN.  Every input passes encode_fixture.assert_clear.
Worst figures measured on an MI355X, fp32 fixture / kernel / bar (the table is in DESIGN.md section 5): goldens 4.9e-7 / 4.6e-7 / 2.0e-6
(l_velocity, a difference of positions near 1 m, 8.0e-6 / 7.3e-6 / 3.2e-5), the recorded reference outputs 4.9e-7 / 4.1e-7 / 2.0e-6, shapes
1.6e-6 / 1.6e-6 / 6.5e-6 (l_velocity 5.6e-6 / 6.2e-6 / 2.2e-5), mixed lengths 6.3e-7 / 6.1e-7 / 2.5e-6, round trip 8.3e-8 / 4.7e-8 / 1e-6;
the kernel comes no closer to a bar than 0.28 of it."""
import os

import numpy as np
import pytest
import torch

import encode_fixture as ef
import mst_amd  # noqa: F401
from conftest import GOLDEN, SEED
from mst_amd.utils import joint_fit as jf
from mst_amd.utils import motion_process as mp

pytestmark = pytest.mark.gpu
CLIP = dict(pace=0.4, gated=True)                            # clips whose feet are clearly planted or clearly moving (encode_fixture.make_clip)
GUARD = 4096
OUTPUTS = ("sample", "global_positions", "positions", "l_velocity")


def dev():
    return torch.device("cuda:0")


def guarded(values, dtype=torch.float32):
    """`values` on the GPU as a view of a buffer whose next GUARD elements are NaN (or, for integers, huge)."""
    v = torch.from_numpy(np.ascontiguousarray(values)).to(dtype)
    fill = float("nan") if dtype.is_floating_point else 2 ** 30
    buf = torch.full((v.numel() + GUARD,), fill, dtype=dtype, device=dev())
    buf[:v.numel()] = v.reshape(-1).to(dev())
    return buf[:v.numel()].view(v.shape)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "encode.npz"))


_WANT = {}


def expected(tag, pos, rot, sk, mode, **kw):
    """The fixture in both precisions, once per case; the float64 inputs are asserted clear of every discontinuity."""
    if tag not in _WANT:
        m32 = ef.encode(pos, rot, sk, mode, np.float32, **kw)[0]
        m64, diags = ef.encode(pos, rot, sk, mode, np.float64, **kw)
        ef.assert_clear(diags, mode)
        _WANT[tag] = (m32, m64)
    return _WANT[tag]


def gpu_call(pos, rot, sk, mode, lengths=None, mean=None, std=None, frames_out=None):
    p, r = guarded(pos), guarded(rot)
    ld = None if lengths is None else guarded(np.asarray(lengths, np.int32), torch.int32)
    m, s = (None, None) if mean is None else (guarded(mean), guarded(std))
    out = mp.encode_joints(p, r if mode == ef.POSROT else None, mode=mode, lengths=ld, mean=m, std=s, frames_out=frames_out,
                           return_aux=True, **sk.kw())
    assert torch.equal(p.cpu(), torch.from_numpy(pos)) and torch.equal(r.cpu(), torch.from_numpy(rot))      # the inputs are left alone
    return dict(zip(OUTPUTS[:1] + ("lengths",) + OUTPUTS[1:], out))


def run_case(tag, pos, rot, sk, mode, lengths=None, mean=None, std=None, frames_out=None):
    """One call on host arrays against the fixture in both precisions.  -> (the outputs as tensors, the float64 fixture)."""
    m32, m64 = expected(tag, pos, rot, sk, mode, lengths=lengths, mean=mean, std=std, frames_out=frames_out)
    got = gpu_call(pos, rot, sk, mode, lengths, mean, std, frames_out)
    B, T, J = pos.shape[:3]
    fo = T if frames_out is None else frames_out
    assert got["lengths"].dtype == torch.int32 and np.array_equal(got["lengths"].cpu().numpy(), m64["lengths"]), tag
    for k in OUTPUTS:
        v = got[k].cpu().numpy()
        assert v.dtype == np.float32 and v.shape == m64[k].shape and np.isfinite(v).all(), (tag, k)
        ref_dev, e = ef.rel(m32[k], m64[k]), ef.rel(v, m64[k])
        print(f"encode: {tag} {k} ref {ref_dev:.3e} got {e:.3e} bar {ef.bar(ref_dev):.3e}")
        assert e <= ef.bar(ref_dev), (tag, k)
    sample = got["sample"].cpu().numpy()
    for b in range(B):
        rows = int(m64["lengths"][b])
        assert not sample[b, :, :, rows:].any() and sample[b, :, :, :rows].any(), (tag, b)          # padded rows: exact zeros
        n = T if lengths is None else int(lengths[b])
        assert not got["global_positions"][b, n:].any() and not got["positions"][b, n:].any() and not got["l_velocity"][b, n - 1:].any()
    if mode == ef.HML and mean is None:
        assert np.array_equal(sample[:, -4:], m64["sample"][:, -4:]), tag                          # contacts: exact
    assert sample.shape == (B, ef.feats(J, mode), 1, fo)
    return got, m64


# ------------------------------------------------------------------------------------------ the reference's recorded outputs
@pytest.mark.parametrize("mode,J,T", ef.GOLDEN_CASES)
def test_against_the_reference_outputs(gold, mode, J, T):
    sk, pos, rot = ef.golden_inputs(SEED, mode, J, T)
    key = f"{mode}|J{J}T{T}"
    got, _ = run_case(f"golden {key}", pos[None], rot[None], sk, mode, frames_out=T - 1)
    m32, m64 = expected(f"golden {key}", pos[None], rot[None], sk, mode, frames_out=T - 1)
    four = lambda m: (np.asarray(m["sample"][0, :, 0].T), m["global_positions"][0], m["positions"][0], m["l_velocity"][0])
    mine = four({k: got[k].cpu().numpy() for k in OUTPUTS})
    for name, v, a32, a64 in zip(("data", "global_positions", "positions", "l_velocity"), mine, four(m32), four(m64)):
        fr = ef.golden_frames(name, len(a64))
        r = gold[f"{key}|{name}"]
        own, e = ef.rel(a32[fr], a64[fr]), ef.rel(v[fr], r)
        print(f"encode: golden {key} {name} (recorded) ref {own:.3e} got {e:.3e} bar {ef.bar(own):.3e}")
        assert e <= ef.bar(own), name
    if mode == ef.HML:
        assert np.array_equal(mine[0][:, -4:], gold[f"{key}|data"][:, -4:])
    # the recorded recover_from_ric(data) against the kernel's rows through recover_joints
    F = ef.feats(J, mode)
    rec = mp.recover_joints(got["sample"], torch.zeros(F), torch.ones(F), J)[0, 0].cpu().numpy()
    r32, r64 = ef.recover_from_ric(four(m32)[0], J, np.float32), ef.recover_from_ric(four(m64)[0], J, np.float64)
    fr = ef.golden_frames("recover", T - 1)
    own, e = ef.rel(r32[fr], r64[fr]), ef.rel(rec[fr], gold[f"{key}|recover"])
    print(f"encode: golden {key} recover (recorded) ref {own:.3e} got {e:.3e} bar {ef.bar(own):.3e}")
    assert e <= ef.bar(own)


# ------------------------------------------------------------------------------------------ shapes
SHAPES = ((2, 5, 3), (2, 24, 1), (3, 20, 1), (63, 21, 1), (64, 22, 3), (65, 24, 1), (80, 5, 1), (81, 20, 3), (161, 21, 1), (162, 22, 1),
          (197, 24, 3), (197, 5, 1), (65, 22, 1))


@pytest.mark.parametrize("mode", (ef.POSROT, ef.HML))
@pytest.mark.parametrize("T,J,B", SHAPES)
def test_frame_counts_joint_counts_and_batches(T, J, B, mode):
    sk = ef.skeleton(SEED, J)
    pos, rot = ef.make_clip(SEED, f"enc/gpu/shape/{mode}/T{T}J{J}B{B}", T, sk, mode, B=B, **CLIP)
    run_case(f"shape {mode} T{T} J{J} B{B}", pos, rot, sk, mode)


# ------------------------------------------------------------------------------------------ lengths
@pytest.mark.parametrize("mode", (ef.POSROT, ef.HML))
def test_mixed_lengths_padding_and_cut(mode):
    J, T, lengths = 20, 90, [2, 90, 47]
    sk = ef.skeleton(SEED, J)
    F = ef.feats(J, mode)
    pos, rot = ef.make_clip(SEED, f"enc/gpu/lengths/{mode}", T, sk, mode, B=3, lengths=lengths, **CLIP)
    mean = (0.2 * ef.syn.normal(SEED, "enc/gpu/mean", (F,))).astype(np.float32)
    std = (0.5 + ef.syn.uniform01(SEED, "enc/gpu/std", F)).astype(np.float32)
    for fo in (T + 6, T - 1, 30):                           # above T - 1, equal to it, below len - 1 of two clips (cut)
        got, m64 = run_case(f"lengths {mode} fo{fo}", pos, rot, sk, mode, lengths=lengths, mean=mean, std=std, frames_out=fo)
        want = [min(n - 1, fo) for n in lengths]
        assert got["lengths"].tolist() == want
        for b, rows in enumerate(want):
            assert (got["sample"][b, :, 0, rows:] == 0.0).all()
    whole = gpu_call(pos, rot, sk, mode, lengths, mean, std, None)
    for b, n in enumerate(lengths):
        single = gpu_call(pos[b:b + 1], rot[b:b + 1], sk, mode, [n], mean, std, None)
        for k in OUTPUTS + ("lengths",):
            assert torch.equal(whole[k][b:b + 1], single[k]), (k, b)
        short = gpu_call(pos[b:b + 1, :n], rot[b:b + 1, :n], sk, mode, None, mean, std, T)       # the clip cut on the host: the same rows
        assert torch.equal(short["sample"], single["sample"]) and torch.equal(short["global_positions"][0], single["global_positions"][0, :n])
    p = guarded(pos)
    with pytest.raises(ValueError, match=r"lengths 1\.\.90 outside 2\.\.90"):
        mp.encode_joints(p, None, mode=ef.HML, lengths=[1, 90, 3], **sk.kw())


# ------------------------------------------------------------------------------------------ equivalences
def test_equivalent_calls():
    J, T, B = 21, 76, 2
    sk = ef.skeleton(SEED, J)
    lengths = [76, 40]
    for mode in (ef.POSROT, ef.HML):
        F = ef.feats(J, mode)
        pos, rot = ef.make_clip(SEED, f"enc/gpu/equiv/{mode}", T, sk, mode, B=B, lengths=lengths, **CLIP)
        mean = (0.2 * ef.syn.normal(SEED, "enc/gpu/emean", (F,))).astype(np.float32)
        std = (0.5 + ef.syn.uniform01(SEED, "enc/gpu/estd", F)).astype(np.float32)
        normed, m64 = run_case(f"equiv {mode} normalised", pos, rot, sk, mode, lengths=lengths, mean=mean, std=std)
        plain = gpu_call(pos, rot, sk, mode, lengths)
        m32 = expected(f"equiv {mode} normalised", pos, rot, sk, mode, lengths=lengths, mean=mean, std=std)[0]
        byhand = (plain["sample"] - torch.from_numpy(mean).to(dev())[None, :, None, None]) / torch.from_numpy(std).to(dev())[None, :, None, None]
        for b, n in enumerate(lengths):
            byhand[b, :, :, n - 1:] = 0
        ref_dev, e = ef.rel(m32["sample"], m64["sample"]), ef.rel(byhand, m64["sample"])
        print(f"encode: equiv {mode} (plain - mean) / std ref {ref_dev:.3e} got {e:.3e} bar {ef.bar(ref_dev):.3e}")
        assert e <= ef.bar(ref_dev) and ef.rel(byhand, normed["sample"]) <= ef.bar(ref_dev)
        again = gpu_call(pos, rot, sk, mode, lengths, mean, std)
        for k in OUTPUTS + ("lengths",):
            assert torch.equal(again[k], normed[k]), k                                            # the same call twice
        p, r = guarded(pos), guarded(rot)
        on_dev = mp.encode_joints(p, r if mode == ef.POSROT else None, mode=mode, lengths=torch.tensor(lengths, dtype=torch.int32, device=dev()),
                                  mean=torch.from_numpy(mean).to(dev()), std=torch.from_numpy(std).to(dev()), **sk.kw())
        assert len(on_dev) == 2 and torch.equal(on_dev[0], normed["sample"]) and torch.equal(on_dev[1], normed["lengths"])
        if mode == ef.POSROT:
            fit = jf.JointFit(*(torch.zeros(1, device=dev()) for _ in range(4)), r)
            s, n = jf.encode_fit(p, fit, chains=sk.chains, face_joint_indx=sk.face, fid_l=sk.fid_l, fid_r=sk.fid_r, lengths=lengths, mean=mean,
                                 std=std)
            assert torch.equal(s, normed["sample"]) and torch.equal(n, normed["lengths"])
            default = mp.encode_joints(p, r, lengths=lengths, mean=mean, std=std, **sk.kw())       # rotations given: POSROT by default
            assert torch.equal(default[0], normed["sample"])
        # the drop-in single-clip functions against the batched call
        one = gpu_call(pos[:1], rot[:1], sk, mode)
        args = (sk.face, sk.fid_l, sk.fid_r, ef.FEET_THRE, sk.raw, sk.chains)
        keep = pos[0].copy(), rot[0].copy()
        res = mp.process_file_with_rotation(pos[0], rot[0], *args) if mode == ef.POSROT else mp.process_file(pos[0], *args)
        assert np.array_equal(pos[0], keep[0]) and np.array_equal(rot[0], keep[1])
        assert all(isinstance(a, np.ndarray) and a.dtype == np.float32 for a in res) and res[0].shape == (T - 1, F)
        assert np.array_equal(res[0], one["sample"][0, :, 0, :T - 1].t().cpu().numpy())
        for a, k in zip(res[1:], OUTPUTS[1:]):
            assert np.array_equal(a, one[k][0].cpu().numpy()), k
        tens = mp.process_file_with_rotation(guarded(pos[0]), guarded(rot[0]), *args) if mode == ef.POSROT else mp.process_file(guarded(pos[0]), *args)
        assert all(torch.is_tensor(a) and a.is_cuda for a in tens) and np.array_equal(tens[0].cpu().numpy(), res[0])


# ------------------------------------------------------------------------------------------ the round trip
@pytest.mark.parametrize("mode,J,T", ((ef.POSROT, 20, 76), (ef.HML, 22, 197)))
def test_the_round_trip_on_the_device(mode, J, T):
    sk = ef.skeleton(SEED, J)
    lengths = [T, T // 2, 2]
    pos, rot = ef.make_clip(SEED, f"enc/gpu/trip/{mode}", T, sk, mode, B=3, lengths=lengths, **CLIP)
    got, _ = run_case(f"round trip {mode} J{J} T{T}", pos, rot, sk, mode, lengths=lengths)
    F = ef.feats(J, mode)
    back = mp.recover_joints(got["sample"], torch.zeros(F), torch.ones(F), J)[:, 0]
    for b, n in enumerate(lengths):
        devs = []
        for dt in (np.float32, np.float64):
            data, glob = ef.encode_clip(pos[b, :n], rot[b, :n], sk, mode, dt)[:2]
            devs.append(ef.rel(ef.recover_from_ric(data, J, dt), glob[:-1]))
        e = ef.rel(back[b, :n - 1], got["global_positions"][b, :n - 1])
        print(f"encode: round trip {mode} clip {b} len {n} ref {devs[0]:.3e} (float64 {devs[1]:.3e}) got {e:.3e} bar {ef.bar(devs[0]):.3e}")
        assert devs[1] <= 1e-12 and e <= ef.bar(devs[0])


# ------------------------------------------------------------------------------------------ the chains
def test_a_mid_tree_chain_restarts_from_the_root_quaternion():
    sk = ef.skeleton(SEED, 5)
    T = 40
    pos, rot = ef.make_clip(SEED, "enc/gpu/chain", T, sk, ef.HML, **CLIP)
    got, m64 = run_case("chain J5 T40", pos, rot, sk, ef.HML)
    other = ef.encode(pos, rot, sk, ef.HML, np.float64, restart=False)[0]["sample"]
    col = slice(4 + 3 * 4 + 6 * 3, 4 + 3 * 4 + 6 * 4)                                             # joint 4, the child of the chain [1, 4]
    mine = got["sample"].cpu().numpy()
    e_ref, e_other = ef.rel(mine[:, col], m64["sample"][:, col]), ef.rel(mine[:, col], other[:, col])
    print(f"encode: chain J5 joint 4 from the reference's form {e_ref:.3e}, from accumulating down the tree {e_other:.3e}")
    assert e_ref <= 1e-5 and e_other > 1e-2
    # a joint no chain names keeps the all-zero quaternion's matrix: (1, 0, 0, 0, 1, 0)
    kw = dict(sk.kw(), chains=[[0, 1, 2], [0, 3]])
    s = mp.encode_joints(guarded(pos), None, mode=ef.HML, **kw)[0].cpu().numpy()
    assert np.array_equal(s[0, col, 0, :T - 1], np.tile(np.array([1, 0, 0, 0, 1, 0], np.float32)[:, None], (1, T - 1)))
    assert np.array_equal(np.delete(s, np.r_[col], 1), np.delete(mine, np.r_[col], 1))


def test_a_zero_length_raw_offset_gives_nan_as_in_the_reference():
    """HML's chain IK divides by the norm of (w, u x v), which is zero for a zero raw offset: the reference returns NaN in that joint's
    rotation columns and in those of the joints after it in its chain -- stated in INTEGRATION.md, neither imitated specially nor hidden."""
    sk = ef.skeleton(SEED, 5)
    T = 6
    pos, rot = ef.make_clip(SEED, "enc/gpu/zero", T, sk, ef.HML, **CLIP)
    sk.raw[1] = 0                                           # the head of the chain [0, 1, 2]; joint 4 hangs off joint 1 in a chain of its own
    with np.errstate(invalid="ignore", divide="ignore"):
        want = ef.encode(pos, rot, sk, ef.HML, np.float64)[0]["sample"]
    got = mp.encode_joints(guarded(pos), None, mode=ef.HML, **sk.kw())[0].cpu().numpy()
    R0 = 4 + 3 * 4
    bad = np.zeros(ef.feats(5, ef.HML), bool)
    bad[R0:R0 + 12] = True                                  # joints 1 and 2
    assert np.isnan(want[0, bad, 0, :T - 1]).all() and np.isfinite(want[0, ~bad]).all()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert ef.rel(got[:, ~bad], want[:, ~bad]) <= 1e-5


def test_the_limit_is_refused_before_any_launch():
    sk = ef.skeleton(SEED, 5)
    limit = mp.encode_max_frames(5, ef.HML)
    print(f"encode: mst_encode_max_frames(5, hml) = {limit}, (24, posrot) = {mp.encode_max_frames(24, ef.POSROT)}")
    with pytest.raises(RuntimeError, match=rf"{limit + 1} frames > {limit}"):
        mp.encode_joints(torch.zeros(1, limit + 1, 5, 3, device=dev()), None, mode=ef.HML, **sk.kw())
    with pytest.raises(RuntimeError, match="encode_joints runs on the GPU only"):
        mp.encode_joints(torch.zeros(1, 4, 5, 3), None, mode=ef.HML, **sk.kw())
