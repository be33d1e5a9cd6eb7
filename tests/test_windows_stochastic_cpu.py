"""The stochastic and guided windowed loops without a GPU: mst_window_noise and mst_window_sample_loop report bad arguments in front of
any device call, both are declared, exported and bound, and the NumPy statement of the noise (tests/window_noise_fixture.py: window noise
= unfold of the long draw) against a case written out by hand."""
import ctypes as C
import os
import re

import numpy as np

import mst_amd  # noqa: F401
from conftest import ROOT
from oracle import philox
import window_fixture as wf
import window_noise_fixture as nf

NEW_SYMBOLS = ("mst_window_noise", "mst_window_sample_loop")


def _lib():
    import __graft_entry__ as g
    g.build()
    from mst_amd import _native
    return _native.lib()


def test_window_noise_reports_bad_arguments_without_a_gpu():
    lib = _lib()
    out = (C.c_float * 4)()                                   # never written: every call below returns in front of any launch

    def call(plan, feats, nsteps, dst):
        rc = lib.mst_window_noise(plan, feats, 1, 0, nsteps, dst, None)
        return rc, lib.mst_last_error().decode()
    for args, what in (((None, 0, 1, out), "feats 0 must be at least 1"), ((None, -3, 1, out), "feats -3 must be at least 1"),
                       ((None, 3, 0, out), "nsteps 0 must be at least 1"), ((None, 3, -1, out), "nsteps -1 must be at least 1"),
                       ((None, 3, 1, out), "null plan"), ((None, 3, 1, None), "null plan")):
        rc, msg = call(*args)
        assert rc != 0 and msg.startswith("mst_window_noise:") and what in msg, msg
    assert not any(out)


def test_window_sample_loop_reports_null_arguments_without_a_gpu():
    from mst_amd import _native
    lib = _lib()
    a = _native.MstLoopArgs()
    for args in ((None, None, None, None, None, None), (None, None, C.byref(a), None, None, None)):
        assert lib.mst_window_sample_loop(*args) != 0
        msg = lib.mst_last_error().decode()
        assert msg.startswith("mst_window_sample_loop:") and "null argument" in msg, msg


def test_new_symbols_declared_exported_bound():
    from mst_amd import _native
    lib = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mst_engine.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mst_[a-z_0-9]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _native.SIGNATURES and hasattr(lib, name), name
    assert sorted(_native.SIGNATURES) == sorted(declared)     # binding and header still agree (tests/test_abi.py)
    sig = _native.SIGNATURES["mst_window_sample_loop"][1]
    assert sig[2] == C.POINTER(_native.MstLoopArgs) and sig[4] == C.POINTER(_native.MstGuideArgs)
    assert C.sizeof(_native.MstLoopArgs) == 9 * 4 + 4 + 8 + 6 * 8          # the loop-argument block did not move
    assert _native.SIGNATURES["mst_window_noise"][1][2:4] == [C.c_uint64, C.c_uint32]


def test_noise_statement_against_a_hand_built_case():
    """One clip of 7 frames, W = 4, O = 2 (stride 2): windows at 0, 2 and the shifted last one at 3.  L = 9: two long frames past the
    clip.  Every window row is a slice of the ONE long row; a long frame's number is the same in every window that covers it."""
    lens, W, O, F, L, seed, step0, n = [7], 4, 2, 3, 9, 1234 + (5 << 32), 2, 3
    win0, starts, clips = wf.plan(lens, W, O)
    assert list(starts) == [0, 2, 3] and list(win0) == [0, 3]
    got = nf.window_noise(lens, W, O, F, L, seed, step0, n)
    assert got.shape == (n, 3, F, 1, W) and got.dtype == np.float64
    for j in range(n):
        z = philox.normal(1, F, L, seed, step0 + j)[0]        # [F, L]
        assert np.array_equal(got[j, 0, :, 0], z[:, 0:4]) and np.array_equal(got[j, 1, :, 0], z[:, 2:6])
        assert np.array_equal(got[j, 2, :, 0], z[:, 3:7])
        assert np.array_equal(got[j, 0, :, 0, 2:], got[j, 1, :, 0, :2]) and np.array_equal(got[j, 1, :, 0, 1:], got[j, 2, :, 0, :3])
    # one element from the generator itself: (c 0, f 2, l 5) of step 3 is component 5 & 3 = 1 of counter (5 >> 2, 2, 0, 3)
    u = philox.uniforms(*philox.philox4x32_10(1, 2, 0, 3, *philox.key(seed)))
    want = philox.box_muller(*u)[1]
    assert got[1, 1, 2, 0, 3] == want and got[1, 2, 2, 0, 2] == want          # long frame 5 = local frame 3 of window 1, 2 of window 2
    assert np.all(np.abs(got) < 6.0) and got.std() > 0.5


def test_noise_statement_pads_short_clips_with_zeros():
    """A clip shorter than the window has one window at 0; its frames from the length on are exactly 0.0 -- also where W exceeds L."""
    lens, W, O, F, L = [3, 5], 8, 2, 2, 5
    got = nf.window_noise(lens, W, O, F, L, 7, 0, 2)
    assert got.shape == (2, 2, F, 1, W)
    for c, n in enumerate(lens):
        assert not got[:, c, :, 0, n:].any() and np.all(got[:, c, :, 0, :n] != 0.0)
        for j in range(2):
            assert np.array_equal(got[j, c, :, 0, :n], philox.normal(2, F, L, 7, j)[c, :, :n])
