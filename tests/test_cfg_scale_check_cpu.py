"""The guidance-scale check of DenoiserEngine (engine.CFG_SCALE_MAX) without a GPU: it is host logic over the engine's
attributes, so it runs here on a stand-in object."""
import types
import warnings

import numpy as np
import torch

import mst_amd  # noqa: F401
from mst_amd.engine import CFG_SCALE_MAX, DenoiserEngine


def _stub(precise=False):
    return types.SimpleNamespace(_precise_on=precise)


def _warned(eng, scale):
    with warnings.catch_warnings(record=True) as got:
        warnings.simplefilter("always")
        DenoiserEngine.check_guidance_scale(eng, scale)
    return [w for w in got if "CFG_SCALE_MAX" in str(w.message)]


def test_limit_is_a_guidance_factor_the_suite_measures():
    assert 2.5 <= CFG_SCALE_MAX < 4.0          # the reference's scripts use 2.5; 4.0 measured above the bar


def test_warns_above_the_limit_once_and_names_precise_mode():
    eng = _stub()
    assert not _warned(eng, torch.tensor([1.0, 2.5, CFG_SCALE_MAX]))
    assert not _warned(eng, None)
    got = _warned(eng, torch.tensor([1.5, CFG_SCALE_MAX + 0.25]))
    assert len(got) == 1
    msg = str(got[0].message)
    assert "DenoiserEngine.set_precise(True)" in msg and "MST_PRECISE=1" in msg
    assert not _warned(eng, torch.tensor([10.0]))                  # once per engine


def test_negative_scales_and_host_arrays():
    assert len(_warned(_stub(), np.array([1.0, 1.0 - CFG_SCALE_MAX - 0.5]))) == 1     # 1 - s is the factor on c - u's other side
    assert not _warned(_stub(), [0.0, 1.0 - CFG_SCALE_MAX])
    assert len(_warned(_stub(), [CFG_SCALE_MAX + 1.0])) == 1


def test_precise_mode_is_silent():
    assert not _warned(_stub(precise=True), torch.tensor([100.0]))


def test_a_tensor_is_read_once_per_version():
    eng = _stub()
    s = torch.tensor([2.0, 2.0])
    assert not _warned(eng, s)
    assert eng._cfg_seen[0] is s
    assert not _warned(eng, s)                                      # same object, same version: not read again
    s[1] = CFG_SCALE_MAX + 1.0                                      # changed in place: read again
    assert len(_warned(eng, s)) == 1
