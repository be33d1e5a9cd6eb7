"""k_ik_init / k_ik_solve (csrc/mst_ik.h) through mst_amd.utils.joint_fit: against the reference's recorded outputs (tests/golden/ik.npz)
and against the float64 form of tests/ik_fixture.py at the shapes where the kernels change path.

  goldens       (J 20, T 76, 100 iterations), (J 21, T 65, 100), (J 22, T 7, 1 and 2): parameters, positions, quaternions, losses
  gradient      iter_num = 1, both gradient forms, J in {2, 5, 20, 21, 22}: the `grad` output against the fixture; leaves exactly zero
  shapes        T in {1, 2, 63, 64, 65, 76, 129} (the 64-lane workgroup, clips that end inside one) with B in {1, 3}, iterations in {1, 2, 100}
  lengths       mixed, including 1 and T: frames beyond a length take no step (their parameters are the starting point's, bit for bit,
                whatever the iteration count); B = 3 equals three single calls
  equivalences  the samplers' layout with mean / std against the denormalised one, fit_clean_joints against clean_joints + fit_joints,
                the same call twice: torch.equal
  fit_joints_bvh with a recording `save`

Bars.  Per case the fixture is evaluated in float32 and in float64 on the same inputs; the kernel's distance from the float64 result may
be 4 x the distance between the two, and not below 1e-6 (the rule of tests/test_gpu_glue_shapes.py).  Every case prints
`ik: <case> <output> ref <dev> got <dev> bar <bar>`.  Operands sit in front of a NaN-filled guard: a loop that runs past a clip reads NaN.
Worst figures measured on an MI355X, fp32 fixture / kernel / bar (the table is in DESIGN.md section 5): goldens 2.9e-7 / 4.6e-7 / 1.1e-6
(losses 1.1e-6 / 2.9e-6 / 4.3e-6), first-iteration gradients 2.2e-6 / 2.9e-6 / 8.7e-6, shapes 2.8e-7 / 3.5e-7 / 1.1e-6, mixed lengths
7.9e-8 / 7.5e-8 / 1e-6, 24 joints 2.5e-7 / 3.3e-7 / 1e-6."""
import os

import numpy as np
import pytest
import torch

import ik_fixture as ik
import mst_amd  # noqa: F401
from conftest import GOLDEN, SEED
from mst_amd.utils import foot_cleanup as fc
from mst_amd.utils import joint_fit as jf

pytestmark = pytest.mark.gpu
GUARD = 4096
KEYS = ("cont6d", "r_pos", "r_rot_quat", "positions", "joint_quats")


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
    return np.load(os.path.join(GOLDEN, "ik.npz"))


def skeleton(J):
    return ik.tiny_tree(J) if J < 17 else ik.humanoid(SEED, J)[1:]


_WANT = {}


def expected(tag, data, parents, off, target, iters, true_gradient=False, lengths=None):
    """The fixture in both precisions, once per case."""
    if tag not in _WANT:
        _WANT[tag] = tuple(ik.solve(data, parents, off, target, iters, dt, true_gradient, lengths) for dt in (np.float32, np.float64))
    return _WANT[tag]


def as_numpy(fit):
    return {k: getattr(fit, k).cpu().numpy() for k in KEYS + ("frame_loss", "grad")}


def run_case(tag, data, parents, off, target, iters, true_gradient=False, lengths=None):
    """One call on host arrays data [B, T, F], target [B, T, J, 3] against the fixture in both precisions.  -> the outputs on the host."""
    m32, m64 = expected(tag, data, parents, off, target, iters, true_gradient, lengths)
    ik.assert_angles_clear(m64["cont6d"])
    d, g = guarded(data), guarded(target)
    ld = None if lengths is None else guarded(np.asarray(lengths, np.int32), torch.int32)
    fit = jf.fit_joints(d, len(parents), parents, off, g, iters, lengths=ld, true_gradient=true_gradient,
                        return_loss=True, return_grad=True)
    assert torch.equal(d.cpu(), torch.from_numpy(data)) and torch.equal(g.cpu(), torch.from_numpy(target))     # the inputs are left alone
    got = as_numpy(fit)
    for k, v in got.items():
        assert v.dtype == np.float32 and v.shape == m32[k].shape and np.isfinite(v).all(), (tag, k)
        ref_dev, e = ik.rel(m32[k], m64[k]), ik.rel(v, m64[k])
        print(f"ik: {tag} {k} ref {ref_dev:.3e} got {e:.3e} bar {ik.bar(ref_dev):.3e}")
        assert e <= ik.bar(ref_dev), (tag, k)
    J, lv = len(parents), ik.leaves(parents)
    B, T = data.shape[:2]
    assert not got["grad"][..., :6 * J].reshape(B, T, J, 6)[:, :, lv].any(), tag                  # a leaf's gradient: exact zeros
    start = data[..., 4 + 3 * (J - 1):].reshape(B, T, J, 6)
    assert np.array_equal(got["cont6d"][:, :, lv], start[:, :, lv]), tag                          # and Adam never moves it
    return got


# ------------------------------------------------------------------------------------------ the reference's recorded outputs
@pytest.mark.parametrize("J,T,iters", ik.GOLDEN_CASES)
def test_against_the_reference_outputs(gold, J, T, iters):
    _, parents, off, data, target = ik.golden_inputs(SEED, J, T)
    key = f"J{J}T{T}I{iters}"
    got = run_case(f"golden {key}", data[None], parents, off, target[None], iters)
    m64 = expected(f"golden {key}", data[None], parents, off, target[None], iters)[1]
    for k in KEYS:
        r32 = gold[f"{key}|{k}|f32"]
        r64 = gold[f"{key}|{k}|f64"] if f"{key}|{k}|f64" in gold else m64[k][0]
        own, e, e_gold = ik.rel(r32, r64), ik.rel(got[k][0], r64), ik.rel(got[k][0], r32)
        print(f"ik: golden {key} {k} (recorded) ref {own:.3e} got {e:.3e} from the recorded fp32 {e_gold:.3e} bar {ik.bar(own):.3e}")
        assert e <= ik.bar(own) and e_gold <= ik.bar(own), k
    for dt in ("f32", "f64"):
        r = gold[f"{key}|loss|{dt}"]
        loss = got["frame_loss"][0].astype(np.float64).sum(0)
        own = ik.rel(gold[f"{key}|loss|f32"], gold[f"{key}|loss|f64"])
        print(f"ik: golden {key} loss first / last {loss[0]:.6f} / {loss[1]:.6f} recorded {dt} {r[0]:.6f} / {r[1]:.6f} bar {ik.bar(own):.3e}")
        assert ik.rel(loss, r) <= ik.bar(own)
    if iters == 1:
        r32, g64 = gold[f"{key}|grad|f32"], gold[f"{key}|grad|f64"]
        assert ik.rel(got["grad"][0], g64) <= ik.bar(ik.rel(r32, g64))


# ------------------------------------------------------------------------------------------ the gradient
@pytest.mark.parametrize("true_gradient", (False, True), ids=("reference", "true"))
@pytest.mark.parametrize("J", (2, 5, 20, 21, 22))
def test_the_gradient_of_the_first_iteration(J, true_gradient):
    parents, off = skeleton(J)
    data, target = ik.make_clip(SEED, f"ik/gpu/grad/J{J}", 7, J, parents, off)
    got = run_case(f"grad J{J} {'true' if true_gradient else 'reference'}", data, parents, off, target, 1, true_gradient)
    other = expected(f"grad J{J} {'reference' if true_gradient else 'true'}", data, parents, off, target, 1, not true_gradient)[1]["grad"]
    inner = [j for j in range(J) if j not in ik.leaves(parents)]
    mine = got["grad"][..., :6 * J].reshape(1, 7, J, 6)[:, :, inner, :3]
    assert ik.rel(mine, other[..., :6 * J].reshape(1, 7, J, 6)[:, :, inner, :3]) > 1e-2          # it is this form, not the other one


# ------------------------------------------------------------------------------------------ shapes
SHAPES = ((1, 1, 1), (1, 3, 100), (2, 3, 2), (63, 1, 2), (64, 1, 1), (64, 3, 2), (65, 3, 100), (76, 1, 2), (129, 1, 1), (129, 3, 2))


@pytest.mark.parametrize("T,B,iters", SHAPES)
def test_frame_counts_batches_and_iteration_counts(T, B, iters):
    J = 20 if iters < 100 and T * B <= 130 else 5
    parents, off = skeleton(J)
    data, target = ik.make_clip(SEED, f"ik/gpu/shape/T{T}B{B}", T, J, parents, off, B=B)
    run_case(f"shape T{T} B{B} it{iters} J{J}", data, parents, off, target, iters)


# ------------------------------------------------------------------------------------------ lengths
def test_mixed_lengths_and_independence_of_the_neighbours():
    J, T, lengths = 20, 65, [1, 65, 33]
    parents, off = skeleton(J)
    data, target = ik.make_clip(SEED, "ik/gpu/lengths", T, J, parents, off, B=3)
    got = run_case("mixed lengths it2", data, parents, off, target, 2, lengths=lengths)
    d, g = guarded(data), guarded(target)
    kw = dict(return_loss=True, return_grad=True)
    whole = jf.fit_joints(d, J, parents, off, g, 2, lengths=lengths, **kw)
    longer = jf.fit_joints(d, J, parents, off, g, 5, lengths=guarded(np.array(lengths, np.int32), torch.int32), **kw)
    start = data[..., 4 + 3 * (J - 1):].reshape(3, T, J, 6)
    zero = ik.solve(data, parents, off, target, 0, np.float32)
    for b, n in enumerate(lengths):
        single = jf.fit_joints(d[b:b + 1], J, parents, off, g[b:b + 1], 2, lengths=[n], **kw)
        for k in KEYS + ("frame_loss", "grad"):
            assert torch.equal(getattr(whole, k)[b:b + 1], getattr(single, k)), (k, b)
            # beyond the length: no step was taken, whatever the iteration count
            assert torch.equal(getattr(whole, k)[b, n:], getattr(longer, k)[b, n:]), (k, b)
        assert np.array_equal(got["cont6d"][b, n:], start[b, n:])
        assert not got["grad"][b, n:].any() and not got["frame_loss"][b, n:].any()
        assert np.array_equal(got["r_pos"][b, n:, 1], data[b, n:, 3])
        for k in ("r_pos", "r_rot_quat", "positions", "joint_quats"):
            assert n == T or ik.rel(got[k][b, n:], zero[k][b, n:]) <= 1e-6, (k, b)
        assert not torch.equal(whole.cont6d[b, :n], longer.cont6d[b, :n])
    with pytest.raises(ValueError, match=r"lengths 0\.\.65 outside 1\.\.65"):
        jf.fit_joints(d, J, parents, off, g, 2, lengths=[0, 65, 3])


# ------------------------------------------------------------------------------------------ equivalences
def test_equivalent_calls_are_bit_equal():
    J, T, B = 20, 76, 2
    F = 9 * J + 1
    chains, parents, off = ik.humanoid(SEED, J)
    data, target = ik.make_clip(SEED, "ik/gpu/equiv", T, J, parents, off, B=B)
    mean = (0.2 * ik.syn.normal(SEED, "ik/gpu/mean", (F,))).astype(np.float32)
    std = (0.5 + ik.syn.uniform01(SEED, "ik/gpu/std", F)).astype(np.float32)
    sample = guarded(np.ascontiguousarray(((data - mean) / std).transpose(0, 2, 1)[:, :, None, :]))        # [B, F, 1, T]
    g = guarded(target)
    kw = dict(return_loss=True, return_grad=True, lengths=[76, 40])
    m, s = torch.from_numpy(mean).to(dev()), torch.from_numpy(std).to(dev())
    den = sample[:, :, 0, :].permute(0, 2, 1) * s + m                         # what the kernel forms as it reads
    a = jf.fit_joints(sample, J, parents, off, g, 3, mean=mean, std=std, **kw)
    for other in (jf.fit_joints(den.contiguous(), J, parents, off, g, 3, **kw),             # the denormalised layout
                  jf.fit_joints(den, J, chains, off, g, 3, **kw),                          # any strides; parents from chains
                  jf.fit_joints(sample, J, parents, off, g, 3, mean=m, std=s, **kw),       # statistics already on the device
                  jf.fit_joints(sample, J, parents, off, g, 3, mean=mean, std=std, **kw)):  # the same call twice
        for k in KEYS + ("frame_loss", "grad"):
            assert torch.equal(getattr(a, k), getattr(other, k)), k
    plain = jf.fit_joints(sample, J, parents, off, g, 3, mean=mean, std=std, lengths=[76, 40])
    assert plain.frame_loss is None and plain.grad is None and torch.equal(plain.cont6d, a.cont6d)
    # fit_clean_joints = clean_joints, then fit_joints on the same sample
    ee, lengths = (4, 8, 3, 7), [76, 40]
    joints = fc.clean_joints(sample, mean, std, J, ee, lengths=lengths)
    want = jf.fit_joints(sample, J, parents, off, joints, 3, mean=mean, std=std, **kw)
    cleaned, fit = jf.fit_clean_joints(sample, mean, std, J, parents, off, ee, lengths=lengths, iter_num=3, return_loss=True, return_grad=True)
    assert torch.equal(cleaned, joints)
    for k in KEYS + ("frame_loss", "grad"):
        assert torch.equal(getattr(fit, k), getattr(want, k)), k
    ref = guarded(target[:1])
    joints = fc.clean_joints(sample, mean, std, J, ee, ref_joints=ref, passes=1)
    cleaned, fit = jf.fit_clean_joints(sample, mean, std, J, parents, off, ee, ref_joints=ref, iter_num=2, passes=1)
    assert torch.equal(cleaned, joints) and torch.equal(fit.joint_quats, jf.fit_joints(sample, J, parents, off, joints, 2, mean=mean, std=std).joint_quats)


def test_fit_joints_bvh_hands_the_animation_to_save():
    J, T = 21, 9
    chains, parents, off = ik.humanoid(SEED, J, scale=6.0)
    data, target = ik.make_clip(SEED, "ik/gpu/bvh", T, J, parents, off, noise=0.1)
    names = [f"bone{j}" for j in range(J)]
    calls = []

    class Skeleton:
        _parents = parents

    keep = off.copy()
    fit = jf.fit_joints_bvh("out.bvh", torch.from_numpy(data[0]), J, Skeleton(), off, target[0], names, iter_num=4, save=lambda *a: calls.append(a))
    assert np.array_equal(off, keep) and len(calls) == 1
    path, quats, positions, real_offset, par, nm, frametime = calls[0]
    assert path == "out.bvh" and par == parents and nm is names and frametime == 1 / 20
    assert quats.shape == (T, J, 4) and quats.dtype == np.float32 and np.array_equal(quats, fit.joint_quats[0].cpu().numpy())
    assert np.array_equal(real_offset[1:], off[1:]) and not real_offset[0].any()
    assert np.array_equal(positions[:, 0], fit.r_pos[0].cpu().numpy()) and np.array_equal(positions[:, 1:], np.broadcast_to(off[1:], (T, J - 1, 3)))
    want = jf.fit_joints(guarded(data), J, parents, off, guarded(target), 4)
    assert torch.equal(want.joint_quats, fit.joint_quats) and torch.equal(want.r_pos, fit.r_pos)
    fit2 = jf.fit_joints_bvh("again.bvh", data[0], J, chains, off, target[0], save=lambda *a: calls.append(a), iter_num=4)     # numpy rows
    assert torch.equal(fit2.cont6d, fit.cont6d) and calls[1][0] == "again.bvh"
    unit = np.abs(np.linalg.norm(quats.astype(np.float64), axis=-1) - 1).max()
    print(f"ik: fit_joints_bvh quaternion norms off one by at most {unit:.3e}")
    assert unit <= 1e-5


def test_the_limits_are_refused_before_any_launch():
    J = 5
    parents, off = skeleton(J)
    frames, joints = jf.max_frames(J), jf.max_joints()
    print(f"ik: mst_fit_joints_max_joints() = {joints}, mst_fit_joints_max_frames({J}) = {frames}")
    with pytest.raises(RuntimeError, match=rf"{frames + 1} frames > {frames}.*mst_fit_joints_max_frames\(5\)"):
        jf.fit_joints(torch.zeros(1, frames + 1, 46, device=dev()), J, parents, off, torch.zeros(1, frames + 1, J, 3, device=dev()))
    with pytest.raises(RuntimeError, match="fit_joints runs on the GPU only"):
        jf.fit_joints(torch.zeros(1, 3, 46), J, parents, off, torch.zeros(1, 3, J, 3, device=dev()))
    # the most joints the kernel takes: a chain
    par = list(range(-1, joints - 1))
    o = (0.1 + 0.05 * ik.syn.normal(SEED, "ik/gpu/maxj", (joints, 3))).astype(np.float32)
    data, target = ik.make_clip(SEED, "ik/gpu/maxj", 3, joints, par, o)
    run_case(f"most joints J{joints} T3 it2", data, par, o, target, 2)
