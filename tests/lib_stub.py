"""The native library replaced by a recording stub, for tests of the Python handles' plumbing without a GPU: every `mst_*` entry point
returns 0 and records its arguments, `N.ptr` records the tensors it is given, and the device check of `engine` (which is separate from
the shape logic) is switched off."""
import ctypes as C
import types

import torch

from mst_amd import _native as N
from mst_amd import engine as E


class RecordingLib:
    """Every entry point returns 0 and records (name, snapshot(args)): the arguments themselves unless a test asks for a copy taken
    at the moment of the call."""

    def __init__(self, snapshot=None):
        self.calls = []
        self._snapshot = snapshot or (lambda name, args: args)

    def __getattr__(self, name):
        if not name.startswith("mst_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, self._snapshot(name, args)))
            return 0
        return fn


def install(monkeypatch, snapshot=None):
    """Put the stub in place of the library for the life of `monkeypatch` -> a namespace: lib (the RecordingLib), seen (the tensors
    handed to N.ptr, in order)."""
    lib, seen = RecordingLib(snapshot), []

    def ptr(t):
        if t is None:
            return None
        seen.append(t)
        return C.c_void_p(t.data_ptr())
    monkeypatch.setattr(N, "lib", lambda: lib)
    monkeypatch.setattr(N, "ptr", ptr)
    monkeypatch.setattr(N, "stream_ptr", lambda device: None)
    monkeypatch.setattr(E, "_need_gpu", lambda t, what: t)
    return types.SimpleNamespace(lib=lib, seen=seen)


def stub_schedule():
    s = E.Schedule.__new__(E.Schedule)
    s.handle, s.num_steps, s.device = None, 20, torch.device("cpu")
    return s


def stub_engine(feats):
    e = E.DenoiserEngine.__new__(E.DenoiserEngine)
    e.handle, e.device, e.feats, e._precise_on = None, torch.device("cpu"), feats, False
    return e
