"""Golden vectors of the foot-skate cleanup: the reference's `remove_fs` (data_loaders/humanml/common/bvh_utils.py:1685-1809) run on the
seeded clips of tests/foot_fixture.py, and the demo's composition (sample/demo_style_transfer.py:310-313: recover_from_ric, then two
passes) on a seeded (263, 1, 196) sample.
Run in the authoring container only (imports /root/reference):  python tests/golden/make_golden_fs.py -> fs.npz

Stored: the reference's outputs only (inputs are rebuilt from the seeds) -- per case every frame of the four foot joints, every k-th
frame of all joints and the last frame; per detector the contacts and the velocities; the demo's result; the seconds per clip the
reference takes for the demo's two passes at T = 196; the parameter names and defaults of `remove_fs`.

Asserted here, before anything is written: every value a detector compares, on every input of every case (the demo's SECOND pass reads the
first pass's output), is at least 10 % of its threshold away from it; the reference's contacts equal the fixture's; the fixture in the
reference's precision is bit-equal to the reference."""
import inspect
import json
import os
import sys
import time

import numpy as np
import numpy.ma  # noqa: F401  (the reference's bvh_utils uses np.ma without importing it)
import scipy.spatial  # noqa: F401
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
from make_golden import SEED  # noqa: E402
import foot_fixture as ff  # noqa: E402


def speed_margin(clip, thr):
    c = clip[:, list(ff.FID22)].astype(np.float64)
    return float(np.abs(np.linalg.norm(c[1:] - c[:-1], axis=-1) - thr).min() / thr)


def main():
    mg.install_shims()
    import importlib
    bu = importlib.import_module("data_loaders.humanml.common.bvh_utils")
    mp = importlib.import_module("data_loaders.humanml.scripts.motion_process")
    out = {}
    sig = inspect.signature(bu.remove_fs)
    out["signature"] = np.array(json.dumps([[n, None if p.default is inspect.Parameter.empty else p.default]
                                            for n, p in sig.parameters.items()]))
    names = list(ff.NAMES22)
    assert bu.get_ee_id_by_names(list(names), ff.EE_NAMES) == list(ff.FID22)
    worst = {}
    for T in ff.GOLDEN_T:
        glb, other = ff.golden_inputs(SEED, T)
        for c in (glb, other):
            for k, v in ff.margins(c, ff.FID22).items():
                worst[k] = min(worst.get(k, 1e9), v)
                assert v >= ff.MARGIN, (T, k, v)
        if T == 2:                                               # vel_acc at two frames: an empty contact array, IndexError on its first read
            try:
                bu.remove_fs("", glb, glb, list(names), ff.EE_NAMES)
                raise AssertionError("the reference was expected to raise at T = 2 in vel_acc mode")
            except IndexError:
                pass
        every = ff.GOLDEN_EVERY[T]
        for case in ff.golden_cases(T):
            ref = glb if case["ref"] == "self" else other
            got, vels, contacts, butter = bu.remove_fs("", glb, ref, list(names), ff.EE_NAMES, **case["kw"])
            mine, mvels, mcontacts = ff.remove_fs(glb, ref, ff.FID22, **case["kw"])
            assert got.dtype == np.float32 and np.array_equal(contacts, mcontacts), (T, case["tag"])
            assert np.array_equal(got, mine) and np.array_equal(vels, mvels), (T, case["tag"])
            assert np.array_equal(butter, ref)
            key = f"T{T}|{case['tag']}"
            out[f"{key}|feet"] = got[:, list(ff.FID22)]
            out[f"{key}|some"] = got[::every]
            out[f"{key}|last"] = got[-1]
            dkey = f"T{T}|{case['det']}|{case['ref']}"
            out[f"{dkey}|contacts"] = contacts.astype(np.uint8)
            out[f"{dkey}|vels"] = vels.astype(np.float32)
    # the demo's composition
    demo_kw = dict(force_on_floor=True, after_butterworth=True, use_vel3=True, vel3_thr=0.05)
    for variant in range(400):
        sample, mean, std, content = ff.demo_inputs(SEED, variant)
        den = (torch.from_numpy(sample).permute(0, 2, 3, 1) * torch.from_numpy(std) + torch.from_numpy(mean)).float()
        joints = mp.recover_from_ric(den.clone(), 22)[0, 0].numpy()[:ff.DEMO_LEN].copy()
        ref = content[:ff.DEMO_LEN]
        p1 = bu.remove_fs("", joints, ref, list(names), ff.EE_NAMES, **demo_kw)[0]
        m1, m2 = speed_margin(ref, 0.05), speed_margin(p1, 0.05)
        if min(m1, m2) >= ff.MARGIN:
            break
    else:
        raise AssertionError("no demo variant keeps the second pass's speeds away from the threshold")
    p2, _, c2, _ = bu.remove_fs("", p1, p1, list(names), ff.EE_NAMES, **demo_kw)
    assert int(c2.sum()) > 0
    mine = ff.demo_passes(joints[None], ref[None], ff.FID22)[0]
    assert np.array_equal(mine, p2)
    out["demo|variant"] = np.array(variant)
    out["demo|out"] = p2
    out["demo|margins"] = np.array([m1, m2])
    # what the reference takes for the demo's two passes on one (196, 22, 3) clip
    glb, other = ff.golden_inputs(SEED, 196)
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        a = bu.remove_fs("", glb, other, list(names), ff.EE_NAMES, **demo_kw)[0]
        bu.remove_fs("", a, a, list(names), ff.EE_NAMES, **demo_kw)
        best = min(best, time.perf_counter() - t0)
    out["ref_seconds_per_clip"] = np.array(best)
    out["margins"] = np.array(json.dumps(worst))
    path = os.path.join(HERE, "fs.npz")
    np.savez_compressed(path, **out)
    print("fs.npz", os.path.getsize(path) // 1024, "KiB;", len(out), "arrays; demo variant", variant, "margins", worst, (m1, m2),
          "reference", f"{best * 1e3:.1f} ms per clip")
    assert os.path.getsize(path) < 500 * 1024


if __name__ == "__main__":
    main()
