"""Golden vectors of the rotation-channel decoders: the reference's `output_bvh`, `recover_from_rot`, `output_bvh_with_pos`,
`output_bvh_from_real_rot`, `recover_from_real_rot` and `process_pos_from_real_rot` (data_loaders/humanml/common/bvh_utils.py:1299-1441, :1538-1563) run on the seeded
cases of tests/rotdec_fixture.py.  Run in the authoring container only (imports the reference checkout that make_golden.py puts on the
path):
    python tests/golden/make_golden_rotdec.py -> rotdec.npz

Stored: what the reference produced, nothing else (inputs are rebuilt from the seed).
  `<route>|<tree>|T<n>|<output>`      clip 0 of the case in float32, for n in rotdec_fixture.STORED: quats (what `save_bvh` was handed),
                                      root_pos, joints, local ('real_rot'); `...|f64` beside it at n = 7, the reference run in double
  `<route>|<tree>|parents / offsets`  of the animation it wrote, and `...|hierarchy`, the HIERARCHY block of the file, as bytes
  `dist|<route>|<tree>|T<n>|<output>` for EVERY case the GPU test runs (three clips of lengths n, 1, ceil(n / 2); every n of FRAMES and
                                      LONG): the reference's float32 result against float64, max error over the largest magnitude,
                                      quaternions up to sign -- the yardstick of tests/test_gpu_rotdec.py
  `local` is the reference's `process_pos_from_real_rot` with its aliased in-place subtraction removed (Reference.local_rows); at 7 frames
  the function as it runs is asserted to equal the fixture's `local_as_run`, the rows without any subtraction.
  `real_rot|<tree>|T7|local_as_run` (+ `|f64`) is that function's own output, as it runs, on the 7-frame clip.
  `dist|consistency|rot / ric`        the same distance for `recover_from_rot` and `recover_from_ric` on rotdec_fixture.consistency_case()
  `seconds|<function>`                the reference's seconds per 196-frame clip on this CPU

The reference casts to float32 inside `qrot` and `qmultipy`, so its run in double needs `Tensor.float` neutralised; that run is used
for cases of 7 frames, where it is stored and asserted equal to the fixture's float64 to 1e-12.  Everywhere else the fixture's float64,
validated that way, stands for it.

Asserted before anything is written, every distance printed: fixture f64 equals reference f64 to 1e-12; fixture f32 is no further from
reference f32 than reference f32 is from f64 (floor 1e-6); `expand_chains` (the package's and the fixture's) equals the reference's
parents and offsets exactly; the file is smaller than 500 KiB."""
import contextlib
import importlib
import os
import sys
import tempfile
import time

import numpy as np
import numpy.ma  # noqa: F401
import scipy.spatial  # noqa: F401
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import rotdec_fixture as rf  # noqa: E402
from mst_amd.utils import rot_decode as rd  # noqa: E402


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


def npy(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


class Reference:
    def __init__(self):
        mg.install_shims()
        self.bu = importlib.import_module("data_loaders.humanml.common.bvh_utils")
        self.sk = importlib.import_module("data_loaders.humanml.common.skeleton")
        self.real_save = self.bu.save_bvh
        self.captured = None
        self.write = False

        def capture(path, anim, frametime=1.0 / 24.0, *a, **k):
            self.captured = dict(quats=npy(anim.quats).copy(), pos=npy(anim.pos).copy(), offsets=npy(anim.offsets).copy(),
                                 parents=[int(p) for p in anim.parents], frametime=frametime)
            if self.write:
                anim.quats, anim.pos, anim.offsets = npy(anim.quats), npy(anim.pos), npy(anim.offsets)
                self.real_save(path, anim, frametime, *a, **k)

        self.bu.save_bvh = capture
        self.tmp = tempfile.mkdtemp()

    def skeleton(self, chains, off, dtype):
        sk = self.sk.Skeleton(torch.from_numpy(off.astype(np.float32)), chains, "cpu")
        sk._offset = torch.from_numpy(off.astype(dtype))
        return sk

    def local_rows(self, data, J, sk):
        """`process_pos_from_real_rot` (bvh_utils.py:1366-1378) statement by statement from the reference's own functions, except that the
        root's x and z are read before they are overwritten: `pos[..., 0] -= pos[..., 0:1, 0]` subtracts in place from the storage it
        reads, and what the reference returns then depends on how torch splits the loop."""
        bu = self.bu
        r_rot_quat, _ = bu.recover_root_rot_pos(data)
        pos = bu.recover_from_real_rot(data, J, sk)
        pos[..., 0] -= pos[..., 0:1, 0].clone()
        pos[..., 2] -= pos[..., 0:1, 2].clone()
        pos = pos[..., 1:, :]
        pos = bu.qrot(bu.qinv(r_rot_quat)[..., None, :], pos)
        return pos.reshape(pos.shape[:-2] + (-1,))

    def run(self, route, rows, J, chains, off, dtype, write=False):
        """One clip [T, F] -> dict of numpy arrays (+ text when written)."""
        bu = self.bu
        data = torch.from_numpy(rows.astype(dtype))
        sk = self.skeleton(chains, off, dtype)
        path = os.path.join(self.tmp, "clip.bvh")
        self.write = write
        if route == rf.HML:
            bu.output_bvh(path, data.clone(), J, [list(c) for c in chains], torch.from_numpy(off.astype(dtype)))
            joints = bu.recover_from_rot(data.clone(), J, sk)
            out = dict(joints=npy(joints))
        elif route == rf.POS:
            raw = torch.from_numpy(rf.raw_of(off).astype(dtype))
            bu.output_bvh_with_pos(path, data.clone(), J, [list(c) for c in chains], torch.from_numpy(off.astype(dtype)), raw, list(rf.face_of(J)))
            out = dict(joints=npy(bu.recover_from_ric(data.clone(), J)))
        else:
            bu.output_bvh_from_real_rot(path, data.clone(), J, [list(c) for c in chains], off.astype(dtype))
            out = dict(joints=npy(bu.recover_from_real_rot(data.clone(), J, sk)), local=npy(self.local_rows(data.clone(), J, sk)),
                       local_as_run=npy(bu.process_pos_from_real_rot(data.clone(), J, sk)))
        c = self.captured
        out.update(quats=c["quats"], root_pos=c["pos"][:, 0], parents=c["parents"], offsets=c["offsets"])
        assert abs(c["frametime"] - 1 / 20) < 1e-12
        if write:
            text = open(path).read()
            out["hierarchy"] = text[:text.index("MOTION")]
        return out


def best(fn, n=3):
    t = 1e9
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        t = min(t, time.perf_counter() - t0)
    return t


def main():
    ref = Reference()
    torch.set_num_threads(8)
    out = {}
    worst = 0.0
    for route in rf.ROUTES:
        for name in rf.TREES:
            J, chains, off = rf.tree(name)
            for T in tuple(sorted(set(rf.FRAMES + rf.STORED))) + (rf.LONG,):
                data = rf.make_rows(name, route, T)
                lengths = rf.lengths_of(T)
                key = f"{route}|{name}|T{T}"
                r32 = {}
                for b, n in enumerate(lengths):
                    one = ref.run(route, data[b, :n], J, chains, off, np.float32, write=(b == 0 and T == 7))
                    for k in rf.OUTPUTS[route]:
                        assert one[k].dtype == np.float32, (key, k, one[k].dtype)
                        r32.setdefault(k, np.zeros((3, T) + one[k].shape[1:], np.float32))[b, :n] = one[k]
                    if b == 0:
                        first = one
                f32 = rf.decode_batch(route, data, J, chains, off, lengths, np.float32)
                f64 = rf.decode_batch(route, data, J, chains, off, lengths, np.float64)
                if T == 7:
                    with in_double():
                        d64 = ref.run(route, data[0], J, chains, off, np.float64)
                    for k in rf.OUTPUTS[route]:
                        assert d64[k].dtype == np.float64, (key, k)
                        gap = rf.distance(k, f64[k][0], d64[k])
                        print(f"{key} {k}: fixture f64 vs reference f64 {gap:.3e}")
                        assert gap <= 1e-12, (key, k, gap)
                        out[f"{key}|{k}|f64"] = d64[k]
                    if route == rf.REAL:                        # the reference as it runs on a short clip: no subtraction at all
                        as_run = rf.real_rot(data[0], J, chains, off, np.float64)["local_as_run"]
                        assert rf.relmax(as_run, d64["local_as_run"]) <= 1e-12, key
                        out[f"{key}|local_as_run"], out[f"{key}|local_as_run|f64"] = first["local_as_run"], d64["local_as_run"]
                    # the skeleton it wrote
                    fixture = rf.DECODE[route](data[0], J, chains, off)
                    assert list(fixture["parents"]) == list(first["parents"]), (key, fixture["parents"], first["parents"])
                    assert np.array_equal(fixture["offsets"], first["offsets"]), key
                    if route != rf.REAL:
                        par, xoff, _ = rd.expand_chains(chains, off)
                        assert list(par) == list(first["parents"]) and np.array_equal(xoff, first["offsets"]), key
                    else:
                        assert rd.chain_parents(chains, J) == list(first["parents"]), key
                    out[f"{route}|{name}|parents"] = np.array(first["parents"], np.int32)
                    out[f"{route}|{name}|offsets"] = first["offsets"].astype(np.float32)
                    out[f"{route}|{name}|hierarchy"] = np.frombuffer(first["hierarchy"].encode(), np.uint8)
                for k in rf.OUTPUTS[route]:
                    own = rf.distance(k, r32[k], f64[k])
                    peer = rf.distance(k, f32[k], r32[k])
                    print(f"{key} {k}: reference f32 vs f64 {own:.3e}; fixture f32 vs reference f32 {peer:.3e}")
                    assert peer <= max(own, rf.FLOOR), (key, k, peer, own)
                    out[f"dist|{key}|{k}"] = np.array(own)
                    worst = max(worst, own)
                    if T in rf.STORED:
                        out[f"{key}|{k}"] = r32[k][0]
                if route == rf.REAL:
                    j = rf.identity_joint(chains)
                    assert (r32["quats"][0, :, j] == np.array([1, 0, 0, 0], np.float32)).all(), key
    # the consistency case of the GPU test: the reference's two decoders on one encoded clip
    import encode_fixture as ef
    sk, _, off, rows32, rows64 = rf.consistency_case()
    rot64 = rf.hml_rot(rows64, sk.J, sk.chains, off, np.float64)["joints"]
    ric64 = ef.recover_from_ric(rows64, sk.J, np.float64)
    rot32 = npy(ref.bu.recover_from_rot(torch.from_numpy(rows32), sk.J, ref.skeleton(sk.chains, off, np.float32)))
    ric32 = npy(ref.bu.recover_from_ric(torch.from_numpy(rows32), sk.J))
    assert rot32.dtype == ric32.dtype == np.float32
    for k, a, b in (("rot", rot32, rot64), ("ric", ric32, ric64)):
        out[f"dist|consistency|{k}"] = np.array(rf.relmax(a, b))
        print(f"consistency {k}: reference f32 vs f64 {rf.relmax(a, b):.3e}")
    print(f"consistency: reference rot vs ric f32 {rf.relmax(rot32, ric32):.3e}; f64 {rf.relmax(rot64, ric64):.3e}")
    # seconds per 196-frame clip
    for route, name, fns in ((rf.HML, "t2m22", ("output_bvh", "recover_from_rot")), (rf.POS, "t2m22", ("output_bvh_with_pos",)),
                             (rf.REAL, "mid21", ("output_bvh_from_real_rot", "recover_from_real_rot", "process_pos_from_real_rot"))):
        J, chains, off = rf.tree(name)
        rows = torch.from_numpy(rf.make_rows(name, route, 196, B=1)[0])
        sk = ref.skeleton(chains, off, np.float32)
        path = os.path.join(ref.tmp, "t.bvh")
        ref.write = True
        calls = {"output_bvh": lambda: ref.bu.output_bvh(path, rows.clone(), J, [list(c) for c in chains], torch.from_numpy(off)),
                 "output_bvh_with_pos": lambda: ref.bu.output_bvh_with_pos(path, rows.clone(), J, [list(c) for c in chains], torch.from_numpy(off),
                                                                           torch.from_numpy(rf.raw_of(off)), list(rf.face_of(J))),
                 "recover_from_rot": lambda: ref.bu.recover_from_rot(rows.clone(), J, sk),
                 "output_bvh_from_real_rot": lambda: ref.bu.output_bvh_from_real_rot(path, rows.clone(), J, [list(c) for c in chains], off.copy()),
                 "recover_from_real_rot": lambda: ref.bu.recover_from_real_rot(rows.clone(), J, sk),
                 "process_pos_from_real_rot": lambda: ref.bu.process_pos_from_real_rot(rows.clone(), J, sk)}
        for fn in fns:
            s = best(calls[fn])
            out[f"seconds|{fn}"] = np.array(s)
            print(f"{fn} ({name}, 196 frames): {s * 1e3:.2f} ms per clip")
    print(f"largest reference f32-to-f64 distance: {worst:.3e}")
    path = os.path.join(HERE, "rotdec.npz")
    np.savez_compressed(path, **out)
    print("rotdec.npz", os.path.getsize(path) // 1024, "KiB;", len(out), "arrays")
    assert os.path.getsize(path) < 500 * 1024


if __name__ == "__main__":
    main()
