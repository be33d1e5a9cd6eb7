"""Golden vectors of the motion encoder: the reference's `process_file_with_rotation` (data_loaders/humanml/common/bvh_utils.py:1091-1287)
and `process_file` (:898-1088) run on the seeded skeletons and clips of tests/encode_fixture.py, and its `recover_from_ric` (:1348-1363)
of what they return.
Run in the authoring container only (imports the reference checkout that make_golden.py puts on the path):
    python tests/golden/make_golden_encode.py -> encode.npz

Stored: the reference's outputs only (inputs are rebuilt from the seed) -- per case (encode_fixture.GOLDEN_CASES) the 4-tuple (data and
l_velocity whole; of global_positions every second frame and the last; of positions, whose other rows are columns of data, the last
frame), every fourth frame of recover_from_ric(data) and its last (encode_fixture.golden_frames), and the seconds per clip the reference
takes.

Asserted here, before anything is written, every distance printed: the inputs are clear of the computation's discontinuities
(encode_fixture.assert_clear); per output the fixture in float64 is no further from the reference than the fixture in float32 is from the
fixture in float64 (the reference casts to float32 inside qbetween_np and before q2cont6d, and filters in float64); the foot contacts are
equal exactly; the reference's recover_from_ric of its rows is within the suite's bar (4 x the float32 fixture's own distance, floor
1e-6) of the float64 fixture's -- float32 arithmetic on float32 rows on both sides, so neither is the more exact."""
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
import encode_fixture as ef  # noqa: E402

NAMES = ("data", "global_positions", "positions", "l_velocity")


def reference(bu, sk, mode, pos, rot):
    """-> (the 4-tuple, recover_from_ric(data), seconds).  The reference writes into its arguments: it gets copies."""
    raw, best = torch.from_numpy(sk.raw.copy()), 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        if mode == ef.POSROT:
            got = bu.process_file_with_rotation(pos.copy(), rot.copy(), sk.face, sk.fid_l, sk.fid_r, ef.FEET_THRE, raw, sk.chains)
        else:
            got = bu.process_file(pos.copy(), sk.face, sk.fid_l, sk.fid_r, ef.FEET_THRE, raw, sk.chains)
        best = min(best, time.perf_counter() - t0)
    rec = bu.recover_from_ric(torch.from_numpy(np.asarray(got[0])).float(), sk.J).numpy()
    return [np.asarray(g) for g in got], rec, best


def main():
    mg.install_shims()
    import importlib
    bu = importlib.import_module("data_loaders.humanml.common.bvh_utils")
    torch.set_num_threads(8)
    out = {}
    for mode, J, T in ef.GOLDEN_CASES:
        sk, pos, rot = ef.golden_inputs(SEED, mode, J, T)
        got, rec, seconds = reference(bu, sk, mode, pos, rot)
        assert all(np.isfinite(g).all() for g in got), (mode, J, T)
        m32, _ = ef.encode(pos[None], rot[None], sk, mode, np.float32, frames_out=T - 1)
        m64, diags = ef.encode(pos[None], rot[None], sk, mode, np.float64, frames_out=T - 1)
        ef.assert_clear(diags, mode)
        key = f"{mode}|J{J}T{T}"
        mine = lambda m: (m["sample"][0, :, 0].T, m["global_positions"][0], m["positions"][0], m["l_velocity"][0])
        for name, r, a32, a64 in zip(NAMES, got, mine(m32), mine(m64)):
            assert r.shape == a64.shape, (key, name, r.shape, a64.shape)
            own, ref = ef.rel(a32, a64), ef.rel(r, a64)
            print(f"{key} {name}: reference ({r.dtype}) vs fixture f64 {ref:.3e}; fixture f32 vs fixture f64 {own:.3e}")
            assert ref <= own, (key, name, ref, own)
            out[f"{key}|{name}"] = r.astype(np.float32)[ef.golden_frames(name, len(r))]
        if mode == ef.HML:
            assert np.array_equal(got[0][:, -4:], m64["sample"][0, -4:, 0].T) and np.array_equal(got[0][:, -4:], m32["sample"][0, -4:, 0].T)
            print(f"{key} contacts: equal; {int(got[0][:, -4:].sum())} of {got[0][:, -4:].size} set")
        r32, r64 = (ef.recover_from_ric(a, J, dt) for a, dt in ((mine(m32)[0], np.float32), (mine(m64)[0], np.float64)))
        own, ref = ef.rel(r32, r64), ef.rel(rec, r64)
        print(f"{key} recover_from_ric: reference vs fixture f64 {ref:.3e}; fixture f32 vs f64 {own:.3e}; the reference's own round trip "
              f"{np.abs(rec - got[1][:-1]).max():.3e}, the fixture's f64 {np.abs(r64 - mine(m64)[1][:-1]).max():.3e}")
        assert ref <= ef.bar(own), (key, "recover", ref, own)      # float32 arithmetic on float32 rows on both sides: peers, the suite's rule
        out[f"{key}|recover"] = rec.astype(np.float32)[ef.golden_frames("recover", len(rec))]
        out[f"{key}|seconds"] = np.array(seconds)
        print(f"{key}: {seconds * 1e3:.1f} ms per clip")
    path = os.path.join(HERE, "encode.npz")
    np.savez_compressed(path, **out)
    print("encode.npz", os.path.getsize(path) // 1024, "KiB;", len(out), "arrays")
    assert os.path.getsize(path) < 500 * 1024


if __name__ == "__main__":
    main()
