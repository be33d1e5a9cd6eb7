"""Golden vectors of the joint-space likelihood: the reference's own `recover_from_ric`
(data_loaders/humanml/scripts/motion_process.py:389-410, :444-461) run on the CPU in float64 under torch.autograd on a few seeded cases
of tests/joint_guide_fixture.py.  Run in the authoring container only (imports the reference checkout that make_golden.py puts on the
path):
    python tests/golden/make_golden_joint_guide.py -> joint_guide.npz

The reference casts to float32 inside `qrot`, so its run in double needs `Tensor.float` neutralised (as make_golden_rotdec.py does).
Stored per case `J<j>|F<f>|T<t>|B<b>|<pattern>`: the inputs (`x0`, `mean`, `std`, `target`, `weight`, `scale`, `lengths`, float32 as
the fixture makes them), and in float64 `pos` [B,T,J,3], `logp` [B] and `grad` [B,F,1,T] = d logp / d (normalised row), with
logp[b] = -1/2 scale[b] sum_{t < len_b, j, c} w (p - y)^2.
Asserted before anything is written: the fixture's float64 equals all three to 1e-12 of the largest magnitude; the file is smaller than
300 KiB."""
import contextlib
import importlib
import os
import sys

import numpy as np
import numpy.ma  # noqa: F401
import scipy.spatial  # noqa: F401
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import joint_guide_fixture as jf  # noqa: E402


@contextlib.contextmanager
def in_double():
    """The reference in float64: new tensors default to double and `.float()` keeps the type."""
    orig = torch.Tensor.float
    torch.set_default_dtype(torch.float64)
    torch.Tensor.float = lambda self, *a, **k: self.double()
    try:
        yield
    finally:
        torch.Tensor.float = orig
        torch.set_default_dtype(torch.float32)


def key_of(J, F, T, B, pattern):
    return f"J{J}|F{F}|T{T}|B{B}|{pattern}"


def main():
    mg.install_shims()
    mp = importlib.import_module("data_loaders.humanml.scripts.motion_process")
    out = {}
    for J, F, T, B, pattern in jf.GOLDEN_CASES:
        case = jf.make_case(J, F, T, B, pattern)
        key = key_of(J, F, T, B, pattern)
        with in_double():
            t = {k: torch.from_numpy(case[k]).double() for k in ("x0", "mean", "std", "target", "weight", "scale")}
            x0 = t["x0"].clone().requires_grad_()
            rows = x0[:, :, 0, :].permute(0, 2, 1) * t["std"] + t["mean"]          # dataset.inv_transform of the permuted sample
            pos = mp.recover_from_ric(rows, J)
            assert pos.dtype == torch.float64 and pos.shape == (B, T, J, 3), (pos.dtype, pos.shape)
            live = (torch.arange(T)[None, :] < torch.from_numpy(case["lengths"].astype(np.int64))[:, None]).double()
            logp = -0.5 * t["scale"] * (t["weight"] * live[:, :, None, None] * (pos - t["target"]) ** 2).sum(dim=(1, 2, 3))
            grad, = torch.autograd.grad(logp.sum(), x0)
        ref = dict(pos=pos.detach().numpy(), logp=logp.detach().numpy(), grad=grad.numpy())
        own = jf.evaluate(case, torch.float64)
        for k in ("pos", "logp", "grad"):
            gap = jf.distance(own[k], ref[k])
            print(f"{key} {k}: fixture f64 vs reference f64 {gap:.3e}")
            assert gap <= 1e-12, (key, k, gap)
            out[f"{key}|{k}"] = ref[k]
        for k in ("x0", "mean", "std", "target", "weight", "scale", "lengths"):
            out[f"{key}|{k}"] = case[k]
    path = os.path.join(HERE, "joint_guide.npz")
    np.savez_compressed(path, **out)
    print("joint_guide.npz", os.path.getsize(path) // 1024, "KiB;", len(out), "arrays")
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
