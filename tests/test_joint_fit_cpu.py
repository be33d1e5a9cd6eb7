"""The joint-rotation fit without a GPU: tests/ik_fixture.py (the numpy restatement the GPU tests measure the kernel against) against the
reference's recorded outputs in tests/golden/ik.npz, the fixture's own consistency, and everything mst_amd.utils.joint_fit and
mst_fit_joints refuse on the host.

Bars.  Against the recorded fp32 outputs the fixture's fp32 evaluation may be 4 x as far as those are from float64 (the recorded float64
outputs for the short cases, the fixture's own float64 for the long ones -- the generator asserted the two equal to 1e-14), and never has
to be below 1e-6: the rule of tests/test_gpu_glue_shapes.py.  The generator itself asserted the stricter "no further than the reference's
fp32 is from its float64" where it ran; numpy's fp32 sin / cos may differ by an ulp between machines, so that is not repeated here.
float64 against recorded float64: 1e-12.  The finite difference: a central difference with step h has a truncation error of h^2 / 6 times
a third derivative of order one and a rounding error of about 1e-16 |L| / h; at h = 1e-5 and |L| around 0.1 both are below 1e-10, far
below the bar of 1e-6 of the largest gradient entry."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ik_fixture as ik
import mst_amd  # noqa: F401
from conftest import GOLDEN, ROOT, SEED
from mst_amd.utils import joint_fit as jf

KEYS = ("cont6d", "r_pos", "r_rot_quat", "positions", "joint_quats")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "ik.npz"))


_SOLVED = {}


def solved(J, T, iters, dtype):
    key = (J, T, iters, np.dtype(dtype).name)
    if key not in _SOLVED:
        _, parents, off, data, target = ik.golden_inputs(SEED, J, T)
        _SOLVED[key] = ik.solve(data[None], parents, off, target[None], iters, dtype)
    return _SOLVED[key]


@pytest.mark.parametrize("J,T,iters", ik.GOLDEN_CASES)
def test_the_fixture_reproduces_the_reference_outputs(gold, J, T, iters):
    key = f"J{J}T{T}I{iters}"
    m32, m64 = solved(J, T, iters, np.float32), solved(J, T, iters, np.float64)
    ik.assert_angles_clear(m64["cont6d"])
    for k in KEYS:
        r32 = gold[f"{key}|{k}|f32"]
        if f"{key}|{k}|f64" in gold:
            r64 = gold[f"{key}|{k}|f64"]
            assert ik.rel(m64[k][0], r64) <= 1e-12, k
        else:
            r64 = m64[k][0]
        own, fix = ik.rel(r32, r64), ik.rel(m32[k][0], r32)
        print(f"ik: fixture {key} {k}: reference fp32 vs float64 {own:.3e}, fixture fp32 vs reference fp32 {fix:.3e}, bar {ik.bar(own):.3e}")
        assert fix <= ik.bar(own), k
    assert ik.rel(m64["loss"][[0, -1]], gold[f"{key}|loss|f64"]) <= 1e-12
    assert ik.rel(m32["loss"][[0, -1]], gold[f"{key}|loss|f32"]) <= ik.bar(ik.rel(gold[f"{key}|loss|f32"], gold[f"{key}|loss|f64"]))
    g32, g64 = solved(J, T, 1, np.float32)["grad"][0], solved(J, T, 1, np.float64)["grad"][0]
    r32 = gold[f"{key}|grad|f32"]
    if f"{key}|grad|f64" in gold:
        assert np.abs(g64 - gold[f"{key}|grad|f64"]).max() <= 1e-12 * np.abs(g64).max()
    assert ik.rel(g32, r32) <= ik.bar(ik.rel(r32, g64))
    assert float(gold[f"{key}|seconds"]) > 0


def small_case(J, T=3, B=2):
    parents, off = ik.tiny_tree(J) if J < 17 else ik.humanoid(SEED, J)[1:]
    data, target = ik.make_clip(SEED, f"ik/cpu/J{J}T{T}", T, J, parents, off, B=B)
    return parents, off, data, target


def test_the_true_gradient_is_the_finite_difference_of_the_loss():
    J = 5
    parents, off, data, target = small_case(J)
    c, rp, q = ik.init(data, J, np.float64)
    q = q + 0.05 * np.arange(1, 5)                         # off the unit sphere: the normalisation inside has a gradient to get right
    loss, _, g = ik.loss_and_grad(c, rp, q, parents, off, target, true_gradient=True)
    flat = ik.flat_grad(g)
    h, worst = 1e-5, 0.0
    for group, arr in enumerate((c, rp, q)):
        view = arr.reshape(arr.shape[0], arr.shape[1], -1)
        base = 0 if group == 0 else (6 * J if group == 1 else 6 * J + 3)
        for k in range(view.shape[-1]):
            keep = view[..., k].copy()
            view[..., k] = keep + h
            up = ik.loss_and_grad(c, rp, q, parents, off, target)[0]
            view[..., k] = keep - h
            down = ik.loss_and_grad(c, rp, q, parents, off, target)[0]
            view[..., k] = keep
            worst = max(worst, float(np.abs((up - down) / (2 * h) - flat[..., base + k]).max()))
    print(f"ik: true gradient vs central difference: worst {worst:.3e}, largest entry {np.abs(flat).max():.3e}")
    assert worst <= 1e-6 * np.abs(flat).max()


@pytest.mark.parametrize("J", (2, 5, 20, 22))
def test_the_quirk_touches_x_raw_alone_and_leaves_get_exact_zeros(J):
    parents, off, data, target = small_case(J)
    for dtype in (np.float32, np.float64):
        c, rp, q = ik.init(data, J, dtype)
        (gc_q, grp_q, gq_q), (gc_t, grp_t, gq_t) = (ik.loss_and_grad(c, rp, q, parents, off, target.astype(dtype), tg)[2] for tg in (False, True))
        assert np.array_equal(gc_q[..., 3:], gc_t[..., 3:]) and np.array_equal(grp_q, grp_t) and np.array_equal(gq_q, gq_t)
        inner = [j for j in range(J) if j not in ik.leaves(parents)]
        diff = np.abs(gc_q[..., inner, :3] - gc_t[..., inner, :3]).max()
        assert diff > 1e-3 * np.abs(gc_t).max(), diff      # not a rounding difference
        lv = ik.leaves(parents)
        assert lv and not gc_q[..., lv, :].any() and not gc_t[..., lv, :].any()
    out = ik.solve(data, parents, off, target, 3, np.float32)
    assert np.array_equal(out["cont6d"][..., lv, :], ik.init(data, J, np.float32)[0][..., lv, :])     # Adam never moves a leaf


def test_the_starting_point_and_the_identity_conversion():
    J = 5
    parents, off, data, target = small_case(J, T=4, B=1)
    c, rp, q = ik.init(data, J, np.float64)
    assert not rp[:, 0, [0, 2]].any() and np.array_equal(rp[..., 1], data[..., 3].astype(np.float64))
    ang = np.concatenate([[0.0], np.cumsum(data[0, :-1, 0].astype(np.float64))])
    assert np.allclose(q[0, :, 0], np.cos(ang)) and np.allclose(q[0, :, 2], np.sin(ang)) and not q[..., [1, 3]].any()
    eye = np.tile(np.array([1, 0, 0, 0, 1, 0], np.float32), (1, 1, J, 1))
    unit = np.tile(np.array([1, 0, 0, 0], np.float32), (1, 1, 1))
    assert np.array_equal(ik.to_quats(eye, unit), np.tile(np.array([1, 0, 0, 0], np.float32), (1, 1, J, 1)))     # the 0.1 substitution
    zero = ik.solve(data, parents, off, target, 0, np.float32, lengths=[4])
    some = ik.solve(data, parents, off, target, 2, np.float32, lengths=[1])
    for k in KEYS:
        assert np.array_equal(zero[k][:, 1:], some[k][:, 1:]) and not np.array_equal(zero[k][:, :1], some[k][:, :1])
    assert not some["grad"][:, 1:].any() and not some["frame_loss"][:, 1:].any() and some["grad"][:, 0].any()


# ------------------------------------------------------------------------------------------ refusals
def cpu_args(J=5, T=3, B=1):
    parents, off, data, target = small_case(J, T, B)
    return torch.from_numpy(data), J, parents, off, torch.from_numpy(target)


def test_parents_come_as_a_list_as_chains_or_as_a_skeleton():
    chains, parents, _ = ik.humanoid(SEED, 21)
    assert jf.parents_from_chains(chains, 21) == parents == ik.parents_of(chains, 21)
    assert jf._resolve_parents(chains, 21) == parents and jf._resolve_parents(np.array(parents), 21) == parents

    class Skeleton:
        _parents = parents

    assert jf._resolve_parents(Skeleton(), 21) == parents
    assert jf.parents_from_chains([[0, 1, 2]], 4) == [-1, 0, 1, 0]          # joint 3 is in no chain: it hangs off the root


@pytest.mark.parametrize("bad,msg", [([-1, 0, 2, 1, 1], r"parents\[2\] = 2"), ([-1, 0, 0, 4, 1], r"parents\[3\] = 4"),
                                     ([-1, -1, 0, 1, 1], r"parents\[1\] = -1"), ([-1, 0, 0, 1], "4 parents for 5 joints"),
                                     ([[0, 1, 2], [0, 3, 7]], "joint 7 of a kinematic chain")])
def test_a_bad_tree_is_refused(bad, msg):
    data, J, _, off, target = cpu_args()
    with pytest.raises(ValueError, match=msg):
        jf.fit_joints(data, J, bad, off, target)


def test_shapes_and_options_are_refused_before_any_gpu_is_touched():
    data, J, parents, off, target = cpu_args()
    with pytest.raises(ValueError, match=r"263 features, expected 9 \* 22 \+ 1 = 199"):
        jf.fit_joints(torch.zeros(1, 3, 263), 22, ik.humanoid(SEED, 22)[1], np.zeros((22, 3)), torch.zeros(1, 3, 22, 3))
    with pytest.raises(ValueError, match="45 features"):
        jf.fit_joints(data[..., :-1], J, parents, off, target)
    with pytest.raises(ValueError, match="target of shape"):
        jf.fit_joints(data, J, parents, off, target[:, :2])
    with pytest.raises(ValueError, match="offsets of shape"):
        jf.fit_joints(data, J, parents, off[:4], target)
    with pytest.raises(ValueError, match="iter_num=None.*never ends"):
        jf.fit_joints(data, J, parents, off, target, iter_num=None)
    with pytest.raises(ValueError, match="iter_num 0 < 1"):
        jf.fit_joints(data, J, parents, off, target, iter_num=0)
    with pytest.raises(ValueError, match="mean and std come together"):
        jf.fit_joints(data, J, parents, off, target, mean=np.zeros(46))
    with pytest.raises(ValueError, match=r"std of shape \(45,\)"):
        jf.fit_joints(data, J, parents, off, target, mean=np.zeros(46), std=np.ones(45))
    with pytest.raises(ValueError, match="1 joints outside 2.."):
        jf.fit_joints(torch.zeros(1, 3, 10), 1, [-1], np.zeros((1, 3)), torch.zeros(1, 3, 1, 3))
    limit = jf.max_joints()
    with pytest.raises(ValueError, match=rf"{limit + 1} joints outside 2\.\.{limit}"):
        jf.fit_joints(torch.zeros(1, 3, 9 * limit + 10), limit + 1, list(range(-1, limit)), np.zeros((limit + 1, 3)),
                      torch.zeros(1, 3, limit + 1, 3))
    with pytest.raises(ValueError, match=r"lengths 0\.\.0 outside 1\.\.3"):
        jf.fit_joints(data, J, parents, off, target, lengths=[0])
    with pytest.raises(ValueError, match="2 lengths for 1 clips"):
        jf.fit_joints(data, J, parents, off, target, lengths=[1, 2])
    frames = jf.max_frames(J)
    with pytest.raises(RuntimeError, match=rf"{frames + 1} frames > {frames}.*mst_fit_joints_max_frames\(5\)"):
        jf.fit_joints(torch.zeros(1, frames + 1, 46), J, parents, off, torch.zeros(1, frames + 1, J, 3))
    # everything in order, but on the CPU
    for call in (lambda: jf.fit_joints(data, J, parents, off, target),
                 lambda: jf.fit_joints(data.permute(0, 2, 1)[:, :, None], J, parents, off, target, mean=np.zeros(46), std=np.ones(46))):
        with pytest.raises(RuntimeError, match="fit_joints runs on the GPU only"):
            call()
    with pytest.raises(RuntimeError, match="fit_clean_joints runs on the GPU only"):
        jf.fit_clean_joints(data.permute(0, 2, 1)[:, :, None], np.zeros(46), np.ones(46), J, parents, off, (1, 2, 3, 4))


def test_fit_joints_bvh_refuses_what_the_reference_cannot_finish():
    data, J, parents, off, target = cpu_args()
    rows, glb = data[0], target[0].numpy()
    with pytest.raises(NotImplementedError, match="use_lbfgs"):
        jf.fit_joints_bvh("x.bvh", rows, J, parents, off, glb, use_lbfgs=True)
    with pytest.raises(ValueError, match="iter_num=None"):
        jf.fit_joints_bvh("x.bvh", rows, J, parents, off, glb, iter_num=None)
    with pytest.raises(ValueError, match=r"expected \[T, F\] and \[T, J, 3\]"):
        jf.fit_joints_bvh("x.bvh", data, J, parents, off, glb)
    try:
        import data_loaders.humanml.common.bvh_utils  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="save=callable"):
            jf.fit_joints_bvh("x.bvh", rows, J, parents, off, glb)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="fit_joints_bvh runs on the GPU only"):
            jf.fit_joints_bvh("x.bvh", rows, J, parents, off, glb, save=lambda *a: None)


def test_the_c_abi_declares_exports_and_refuses():
    from mst_amd import _native as N
    text = open(os.path.join(ROOT, "include", "mst_engine.h")).read()
    lib = N.lib()
    for name in ("mst_fit_joints", "mst_fit_joints_max_joints", "mst_fit_joints_max_frames"):
        assert name in N.SIGNATURES and re.search(rf"\bint {name}\(", text) and hasattr(lib, name)
    decl = re.search(r"\bint mst_fit_joints\((.*?)\);", text, flags=re.S).group(1)
    assert len(decl.split(",")) == len(N.SIGNATURES["mst_fit_joints"][1]) == 24
    J = int(lib.mst_fit_joints_max_joints())
    assert J >= 22 and lib.mst_fit_joints_max_frames(22) >= 196
    assert lib.mst_fit_joints_max_frames(1) == -1 and b"joints 1 outside 2.." in lib.mst_last_error()
    assert lib.mst_fit_joints_max_frames(J + 1) == -1

    def call(joints=5, parents=(-1, 0, 0, 1, 1), iters=1, feats=46, frames=3):
        par = (C.c_int32 * len(parents))(*parents)
        off = (C.c_float * (3 * len(parents)))()
        one = C.c_void_p(8)                                # never dereferenced: every case is refused before a launch
        return lib.mst_fit_joints(one, frames * feats, feats, 1, None, None, one, None, 1, frames, feats, joints, par, off, iters, 0,
                                  one, one, one, one, one, None, None, None)

    for kw, msg in ((dict(joints=1, parents=(-1,), feats=10), b"joints 1 outside 2.."), (dict(joints=J + 1, feats=9 * J + 10), b"outside 2.."),
                    (dict(parents=(-1, 0, 2, 1, 1)), b"parents[2] = 2: not a tree"), (dict(parents=(-1, 0, -1, 1, 1)), b"parents[2] = -1"),
                    (dict(iters=0), b"iters 0 < 1"), (dict(feats=45), b"feats 45 != 9 * 5 + 1"), (dict(frames=0), b"frames 0 < 1"),
                    (dict(frames=lib.mst_fit_joints_max_frames(5) + 1), b"(mst_fit_joints_max_frames)")):
        assert call(**kw) != 0 and msg in lib.mst_last_error(), (kw, lib.mst_last_error())
