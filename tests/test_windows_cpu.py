"""Window plans without a GPU: the plan rule, the NumPy statement of the stitch in float32 against float64, every refusal of
mst_window_plan_create (it validates on the host, in front of any device call), and the new symbols declared, exported and bound."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mst_amd  # noqa: F401
from conftest import ROOT, SEED
import window_fixture as wf

NEW_SYMBOLS = ("mst_window_max_frames", "mst_window_plan_create", "mst_window_plan_destroy", "mst_window_plan_set_fold",
               "mst_window_unfold", "mst_window_stitch", "mst_sample_loop_windows")


def overlaps(W):
    return [0] if W == 1 else list(range(1, W))


@pytest.mark.parametrize("W", [1, 5, 16])
def test_plan_rule(W):
    """len 1 .. 3W, every overlap: full windows, coverage, strictly ascending starts, the window count; the package's planner and the
    fixture's agree."""
    from mst_amd.diffusion.windows import plan_windows, window_count
    for O in overlaps(W):
        S = W - O
        lens = list(range(1, 3 * W + 1))
        win0, starts, clips = plan_windows(lens, W, O)
        f0, fs, fc = wf.plan(lens, W, O)
        assert np.array_equal(win0, f0) and np.array_equal(starts, fs) and np.array_equal(clips, fc)
        assert win0[0] == 0 and win0[-1] == len(starts) == len(clips)
        for c, n in enumerate(lens):
            own = starts[win0[c]:win0[c + 1]]
            assert np.all(clips[win0[c]:win0[c + 1]] == c)
            assert len(own) == window_count(n, W, O) == (1 if n <= W else -(-(n - W) // S) + 1), (W, O, n)
            assert own[0] == 0 and np.all(np.diff(own) > 0), (W, O, n)
            if n <= W:
                assert list(own) == [0]
                continue
            assert np.all(own + W <= n) and own[-1] == n - W, (W, O, n)          # every window is full, the last one ends the clip
            assert np.all(np.diff(own) <= W), (W, O, n)                          # no gap between neighbours: every frame is covered
            assert np.all(own[:-1] == np.arange(len(own) - 1) * S), (W, O, n)
            covered = np.zeros(n, bool)
            for s in own:
                covered[s:s + W] = True
            assert covered.all()


def test_plan_refuses_bad_overlap():
    from mst_amd.diffusion.windows import plan_windows
    for W, O in ((5, 0), (5, 5), (5, -1), (1, 1), (0, 0)):
        with pytest.raises(ValueError, match="overlap|window"):
            plan_windows([7], W, O)
    with pytest.raises(ValueError, match="length"):
        plan_windows([7, 0], 5, 2)


@pytest.mark.parametrize("W,O", [(1, 0), (5, 1), (5, 4), (16, 3), (16, 15)])
def test_fixture_float32_against_float64(W, O):
    """The float32 statement stays within a few roundings of the float64 one (values of order 1, at most W terms of weight <= W / 2 + 1),
    keeps singly covered elements and agreeing windows bit for bit, and folds to exact zeros from a clip's length on."""
    rng = np.random.default_rng(SEED + 7 * W + O)
    lens = [max(1, W - 2), W, W + 1, 2 * W + 3]
    L, F = max(lens) + 2, 3
    win0, starts, clips = wf.plan(lens, W, O)
    long = rng.standard_normal((len(lens), F, 1, L)).astype(np.float32)
    win = wf.unfold(long, lens, win0, starts, clips, W)
    for c, n in enumerate(lens):                                  # unfold pads with exact zeros
        for k in range(win0[c], win0[c + 1]):
            assert np.all(win[k, :, 0, max(0, n - starts[k]):] == 0.0)
    # unfolded windows agree on shared frames: the stitch keeps every bit, and the fold is the long clip again
    s32, l32 = wf.stitch(win, lens, win0, starts, clips, W, L, np.float32)
    assert np.array_equal(s32.view(np.uint32), win.view(np.uint32))
    for c, n in enumerate(lens):
        assert np.array_equal(l32[c, :, 0, :n], long[c, :, 0, :n]) and np.all(l32[c, :, 0, n:] == 0.0)
    # independent windows: the weighted mean
    noisy = (win + rng.standard_normal(win.shape)).astype(np.float32)
    s32, l32 = wf.stitch(noisy, lens, win0, starts, clips, W, L, np.float32)
    s64, l64 = wf.stitch(noisy, lens, win0, starts, clips, W, L, np.float64)
    assert s32.dtype == np.float32 and s64.dtype == np.float64
    bound = (W + 2) * 2.0 ** -24 * max(1.0, float(np.abs(noisy).max()))          # one rounding a term, one for the quotient
    assert np.abs(s32 - s64).max() <= bound and np.abs(l32 - l64).max() <= bound
    for c, n in enumerate(lens):
        assert np.all(l32[c, :, 0, n:] == 0.0)
        for f in range(n):
            K = wf.covering(lens, win0, starts, W, c, f)
            vals = [s32[k, :, 0, f - starts[k]] for k in K]
            assert all(np.array_equal(v, vals[0]) for v in vals) and np.array_equal(l32[c, :, 0, f], vals[0])
            if len(K) == 1:
                assert np.array_equal(vals[0], noisy[K[0], :, 0, f - starts[K[0]]])
            else:                                                 # a convex combination of what the windows held
                given = np.stack([noisy[k, :, 0, f - starts[k]] for k in K]).astype(np.float64)
                assert np.all(s64[K[0], :, 0, f - starts[K[0]]] <= given.max(0) + 1e-12)
                assert np.all(s64[K[0], :, 0, f - starts[K[0]]] >= given.min(0) - 1e-12)


def _lib():
    import __graft_entry__ as g
    g.build()
    from mst_amd import _native
    return _native.lib()


def _create(lib, lens, win0, starts, W, L, clips=None, windows=None):
    arr = lambda a: np.ascontiguousarray(np.asarray(a, np.int32))
    l, w0, st = arr(lens), arr(win0), arr(starts)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    h = C.c_void_p()
    rc = lib.mst_window_plan_create(p(l), p(w0), p(st), len(l) if clips is None else clips, len(st) if windows is None else windows,
                                    W, L, 0, C.byref(h))
    return rc, lib.mst_last_error().decode()


REFUSALS = [
    # lens, clip_win0, win_start, W, L -> what the message names
    ("ascending", [12], [0, 3], [0, 4, 4], 5, 12, "strictly ascending"),
    ("descending", [12], [0, 3], [0, 4, 2], 5, 12, "strictly ascending"),
    ("gap", [12], [0, 3], [0, 6, 7], 5, 12, "uncovered frame 5"),
    ("first-not-zero", [12], [0, 2], [1, 6], 5, 12, "uncovered frame 0"),
    ("tail-uncovered", [12], [0, 2], [0, 5], 5, 12, "uncovered frame 10"),
    ("past-the-clip", [12], [0, 3], [0, 4, 8], 5, 12, r"start \+ W <= max\(len, W\)"),
    ("short-clip-second-window", [3], [0, 2], [0, 1], 5, 8, r"start \+ W <= max\(len, W\)"),
    ("negative-start", [12], [0, 3], [-1, 4, 7], 5, 12, "negative"),
    ("long-frames-above-the-cap", [12], [0, 3], [0, 4, 7], 5, 4097, r"long_frames 4097 outside 1\.\.4096"),
    ("long-frames-zero", [12], [0, 3], [0, 4, 7], 5, 0, "long_frames 0 outside"),
    ("length-above-long-frames", [13], [0, 3], [0, 4, 8], 5, 12, r"length 13 outside 1\.\.long_frames 12"),
    ("length-zero", [0], [0, 1], [0], 5, 12, "length 0 outside"),
    ("clip-without-window", [7, 5], [0, 2, 2], [0, 2], 5, 7, "names no window"),
    ("win0-not-from-zero", [12], [1, 3], [0, 4, 7], 5, 12, "clip_win0 must run from 0"),
    ("win0-not-to-the-count", [12], [0, 2], [0, 4, 7], 5, 12, "clip_win0 must run from 0"),
    ("window-zero", [12], [0, 3], [0, 4, 7], 0, 12, "window 0 must be at least 1"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_plan_create_refusals(case):
    _, lens, win0, starts, W, L, what = case
    rc, msg = _create(_lib(), lens, win0, starts, W, L)
    assert rc != 0
    assert msg.startswith("mst_window_plan_create:") and re.search(what, msg), msg


def test_plan_create_refuses_null_and_counts():
    lib = _lib()
    h = C.c_void_p()
    assert lib.mst_window_plan_create(None, None, None, 1, 1, 5, 5, 0, C.byref(h)) != 0
    assert b"null argument" in lib.mst_last_error()
    rc, msg = _create(lib, [5, 5], [0, 1, 2], [0], 5, 5, windows=1)
    assert rc != 0 and "every clip has at least one window" in msg
    assert lib.mst_window_max_frames() == 4096


def test_window_symbols_declared_exported_bound():
    from mst_amd import _native
    lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mst_engine.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mst_[a-z_0-9]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _native.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "typedef struct mst_window_plan mst_window_plan;" in text
    # the loop-argument block is the one the other loops take: its layout did not move
    assert C.sizeof(_native.MstLoopArgs) == 9 * 4 + 4 + 8 + 6 * 8
    assert _native.SIGNATURES["mst_sample_loop_windows"][1][2] == C.POINTER(_native.MstLoopArgs)
