"""What the four sampling methods of DenoiserEngine hand the library, pinned field by field without a GPU.

sample_loop, sample_loop_windows, window_sample_loop and sample_loop_plms share one builder of the loop request (engine._loop_request)
and one bracket around the windowed entries (engine._windowed_call).  Over a table of calls, with the library replaced by the recording
stub of tests/lib_stub.py, every library call a method makes is recorded in order, at the moment it is made: the entry's name, which of
its arguments are NULL, every non-pointer field of the MstLoopArgs / MstPlmsArgs / MstGuideArgs it points to and, for every pointer
field, whether it is NULL; for mst_window_plan_set_fold, whether the fold is set or cleared.  What the method returns is recorded
beside it (the x0-hat dump's shape, or null).

tests/golden/loop_request.json holds the records as this same script (`python tests/test_loop_request_cpu.py`) printed them at the
commit in front of the one that introduced the shared builder: the methods still fill every field as their four separate bodies did.
A row is compared whole, so one changed field of one row fails it."""
import ctypes as C
import json
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                                 # (under pytest tests/conftest.py and rootdir do this)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import mst_amd  # noqa: E402,F401
from mst_amd import _native as N  # noqa: E402
from mst_amd import engine as E  # noqa: E402
from lib_stub import install, stub_engine, stub_schedule  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "loop_request.json")
B, F, T = 3, 5, 8
SHAPE = (B, F, 1, T)
CLIPS, LONG = 2, 13                                        # the long clips behind the B windows of the stub plan


class _OnGpu(torch.Tensor):
    """A CPU tensor that answers `is_cuda` as a GPU tensor does: fold_out and the PLMS ring are asserted to be on the GPU."""
    is_cuda = True


def _t(*shape, gpu=False):
    t = torch.arange(int(torch.Size(shape).numel()), dtype=torch.float32).reshape(shape) / 7.0
    return t.as_subclass(_OnGpu) if gpu else t


def _x():
    return _t(*SHAPE)


def _plan():
    return types.SimpleNamespace(handle=C.c_void_p(1), n_clips=CLIPS, long_frames=LONG)


def _fold():
    return _t(CLIPS, F, 1, LONG, gpu=True)


def _ring():
    return _t(3, *SHAPE, gpu=True)


MASK_B11T = lambda: (_t(B, 1, 1, T) > 1.0).float()        # noqa: E731  a noise mask: broadcasts
MASK_FULL = lambda: _t(*SHAPE) > 2.0                       # noqa: E731  half of the inpainting pair, as bool
grad_guide = lambda: E.guide_args(_x(), grad=_t(*SHAPE))   # noqa: E731
target_guide = lambda follow=False: E.guide_args(_x(), target=_t(1, F, 1, T), mask=MASK_B11T(), weight=[1.0, 2.0, 3.0],  # noqa: E731
                                                 follow_schedule=follow)

# name -> (method, positional arguments after (schedule, x), keyword arguments as a thunk: tensors are made per run)
CASES = {
    # ---- sample_loop(schedule, x, t_start, t_end, sampler, eta, ...)
    "loop/ddpm_philox_seed": ("sample_loop", (4, 2), lambda: dict(seed=7)),
    "loop/ddpm_philox_no_seed": ("sample_loop", (4, 2), lambda: dict()),
    "loop/ddim_eta_buffer_cfg_scalar": ("sample_loop", (4, 2, E.SAMPLER_DDIM, 0.5),
                                        lambda: dict(cfg=True, scale=2.5, noise=_t(3, *SHAPE), seed=7)),
    "loop/cfg_per_clip_scale": ("sample_loop", (9, 0, E.SAMPLER_DDIM), lambda: dict(cfg=True, scale=torch.tensor([[1.0], [2.0], [2.5]]), seed=3)),
    "loop/cfg_off_scale_given": ("sample_loop", (9, 0), lambda: dict(cfg=False, scale=torch.tensor([2.0]), seed=3)),
    "loop/single_step_noise_x_shape": ("sample_loop", (3, 3), lambda: dict(noise=_t(*SHAPE))),
    "loop/single_step_noise_stacked": ("sample_loop", (3, 3), lambda: dict(noise=_t(1, *SHAPE))),
    "loop/mask_alone": ("sample_loop", (4, 2), lambda: dict(mask=MASK_B11T(), seed=1)),
    "loop/mask_alone_mask_noise_off": ("sample_loop", (4, 2), lambda: dict(mask=MASK_B11T(), mask_noise=False, seed=1)),
    "loop/pair": ("sample_loop", (4, 2), lambda: dict(mask=MASK_FULL(), motion=_t(*SHAPE).double(), seed=1)),
    "loop/pair_mask_noise_off_clip": ("sample_loop", (4, 2), lambda: dict(mask=MASK_FULL(), motion=_t(*SHAPE), mask_noise=False,
                                                                          clip_denoised=True, seed=1)),
    "loop/motion_alone": ("sample_loop", (4, 2), lambda: dict(motion=_t(*SHAPE), seed=1)),
    "loop/dump": ("sample_loop", (4, 2), lambda: dict(dump_xstart=True, seed=2)),
    "loop/dump_buffer": ("sample_loop", (5, 2, E.SAMPLER_DDPM), lambda: dict(dump_xstart=True, noise=_t(4, *SHAPE))),
    "loop/guide_gradient": ("sample_loop", (6, 6, E.SAMPLER_DDIM, 0.25), lambda: dict(guide=grad_guide(), noise=_t(*SHAPE), dump_xstart=True)),
    "loop/guide_target": ("sample_loop", (6, 1), lambda: dict(guide=target_guide(), seed=11, cfg=True, scale=[1.5])),
    "loop/guide_target_follow": ("sample_loop", (6, 1, E.SAMPLER_DDIM), lambda: dict(guide=target_guide(True), seed=11)),
    "loop/reverse": ("sample_loop", (0, 3, E.SAMPLER_DDIM_REVERSE), lambda: dict(mask=MASK_FULL(), motion=_t(*SHAPE), mask_noise=False)),
    # ---- sample_loop_windows(schedule, x, plan, t_start, t_end, ...)
    "windows/plain": ("sample_loop_windows", (_plan, 4, 0), lambda: dict()),
    "windows/cfg": ("sample_loop_windows", (_plan, 4, 0), lambda: dict(cfg=True, scale=2.0)),
    "windows/mask_alone": ("sample_loop_windows", (_plan, 4, 0), lambda: dict(mask=MASK_B11T())),
    "windows/pair_mask_noise_off": ("sample_loop_windows", (_plan, 4, 0), lambda: dict(mask=MASK_FULL(), motion=_t(*SHAPE), mask_noise=False,
                                                                                      clip_denoised=True)),
    "windows/dump": ("sample_loop_windows", (_plan, 4, 3), lambda: dict(dump_xstart=True)),
    "windows/fold": ("sample_loop_windows", (_plan, 4, 0), lambda: dict(fold_out=_fold())),
    "windows/fold_dump_cfg": ("sample_loop_windows", (_plan, 2, 0), lambda: dict(fold_out=_fold(), dump_xstart=True, cfg=True,
                                                                                scale=torch.tensor([1.0, 2.0, 3.0]))),
    # ---- window_sample_loop(schedule, x, plan, t_start, t_end, sampler, eta, ...)
    "window/ddpm_buffer": ("window_sample_loop", (_plan, 4, 2), lambda: dict(noise=_t(3, *SHAPE))),
    "window/ddim_eta_buffer_cfg": ("window_sample_loop", (_plan, 4, 2, E.SAMPLER_DDIM, 0.5), lambda: dict(noise=_t(3, *SHAPE), cfg=True, scale=2.5)),
    "window/ddim_deterministic": ("window_sample_loop", (_plan, 4, 0, E.SAMPLER_DDIM, 0.0), lambda: dict()),
    "window/ddpm_no_buffer": ("window_sample_loop", (_plan, 4, 0), lambda: dict()),       # (refused by the library, not here)
    "window/single_step_noise_x_shape": ("window_sample_loop", (_plan, 3, 3), lambda: dict(noise=_t(*SHAPE))),
    "window/mask_alone": ("window_sample_loop", (_plan, 4, 2), lambda: dict(noise=_t(3, *SHAPE), mask=MASK_B11T())),
    "window/pair_mask_noise_off": ("window_sample_loop", (_plan, 4, 2), lambda: dict(noise=_t(3, *SHAPE), mask=MASK_FULL(), motion=_t(*SHAPE),
                                                                                    mask_noise=False, clip_denoised=True)),
    "window/dump": ("window_sample_loop", (_plan, 4, 2), lambda: dict(noise=_t(3, *SHAPE), dump_xstart=True)),
    "window/fold": ("window_sample_loop", (_plan, 4, 2), lambda: dict(noise=_t(3, *SHAPE), fold_out=_fold())),
    "window/guide_target": ("window_sample_loop", (_plan, 4, 2), lambda: dict(noise=_t(3, *SHAPE), guide=target_guide())),
    "window/guide_gradient_fold": ("window_sample_loop", (_plan, 3, 3, E.SAMPLER_DDIM, 0.0), lambda: dict(guide=grad_guide(), fold_out=_fold(),
                                                                                                         dump_xstart=True)),
    # ---- sample_loop_plms(schedule, x, t_start, t_end, order, steps_done, hist, ...)
    "plms/order1": ("sample_loop_plms", (9, 0, 1), lambda: dict()),
    "plms/order3_ring": ("sample_loop_plms", (9, 5, 3, 2), lambda: dict(hist=_ring())),
    "plms/order4_ring_cfg_dump": ("sample_loop_plms", (9, 5, 4), lambda: dict(hist=_ring(), cfg=True, scale=2.0, dump_xstart=True)),
    "plms/order1_ring_given": ("sample_loop_plms", (9, 5, 1), lambda: dict(hist=_ring())),
    "plms/pair_clip": ("sample_loop_plms", (9, 5, 2), lambda: dict(hist=_ring(), mask=MASK_FULL(), motion=_t(*SHAPE), clip_denoised=True)),
    "plms/mask_alone": ("sample_loop_plms", (9, 5, 2), lambda: dict(hist=_ring(), mask=MASK_B11T())),
    "plms/seed_eta_mask_noise": ("sample_loop_plms", (9, 5, 2), lambda: dict(hist=_ring(), seed=9, eta=0.5, mask_noise=True)),
    "plms/noise_of_any_shape": ("sample_loop_plms", (9, 5, 3), lambda: dict(hist=_ring(), noise=_t(2), seed=9, eta=0.25, mask_noise=True)),
    "plms/noise_of_any_shape_no_seed": ("sample_loop_plms", (9, 5, 1), lambda: dict(noise=_t(2, 3))),
}


def _fields(obj):
    return {name: bool(getattr(obj, name)) if ctype is C.c_void_p else getattr(obj, name) for name, ctype in obj._fields_}


def _snapshot(name, args):
    if name == "mst_window_plan_set_fold":
        return {"fold": "set" if args[1] is not None else "cleared"}
    rec = {"null_args": [a is None for a in args]}
    for a in args:
        obj = getattr(a, "_obj", None)                     # (what C.byref points to)
        if isinstance(obj, (N.MstLoopArgs, N.MstPlmsArgs, N.MstGuideArgs)):
            rec[type(obj).__name__] = _fields(obj)
    return rec


def record(name):
    """The record of one row: every library call in order, as it was made, and what the method returned."""
    method, args, kwargs = CASES[name]
    with pytest.MonkeyPatch.context() as mp:
        stub = install(mp, _snapshot)
        x = _x()
        out = getattr(stub_engine(F), method)(stub_schedule(), x, *[a() if callable(a) else a for a in args], **kwargs())
        dump = None
        if isinstance(out, tuple):
            out, dump = out
        assert out is x
        return {"calls": [dict(rec, entry=fn) for fn, rec in stub.lib.calls], "dump_shape": None if dump is None else list(dump.shape)}


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_is_the_recorded_one():
    assert sorted(_golden()) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_loop_request(name):
    got = json.loads(json.dumps(record(name)))             # (as the fixture went through JSON)
    assert got == _golden()[name]


def test_the_windowed_entries_sit_inside_the_fold_bracket():
    """The fixture itself says what the issue's order means: set (or NULL), the entry, cleared -- and nothing else for the plain ones."""
    for name, row in _golden().items():
        entries = [c["entry"] for c in row["calls"]]
        if name.startswith(("windows/", "window/")):
            assert entries == ["mst_window_plan_set_fold", "mst_sample_loop_windows" if name.startswith("windows/") else
                               "mst_window_sample_loop", "mst_window_plan_set_fold"], name
            assert row["calls"][0]["fold"] == ("set" if "fold" in name else "cleared") and row["calls"][2]["fold"] == "cleared", name
        else:
            assert len(entries) == 1, name


if __name__ == "__main__":
    json.dump({name: record(name) for name in sorted(CASES)}, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")
