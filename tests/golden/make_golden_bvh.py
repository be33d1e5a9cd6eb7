"""Golden vectors of the motion-file path: the reference's `save_bvh`, `read_bvh` (plain, end_sites=True and downsample_rate=3), `quat_fk`,
`q2eul` (data_loaders/humanml/common/bvh_utils.py:84-295, :499-614; utils/rotation.py:364-382, :646-663) and `uniform_skeleton_basic`
(data_loaders/humanml/scripts/motion_process.py:12-35) run on the seeded cases of tests/bvh_fixture.py.
Run in the authoring container only (imports the reference checkout that make_golden.py puts on the path):
    python tests/golden/make_golden_bvh.py -> bvh.npz

Stored: what the reference produced, nothing else (inputs are rebuilt from the seed) -- per writer case (bvh_fixture.GOLDEN_WRITE) the
file's text as bytes, the float32 degrees `q2eul` returned and the float32 channel rows `save_bvh` formatted from them; what `read_bvh`
returns for that file with End Sites (quats, pos, offsets, parents, bones, end_offsets), without them what is not a slice of that, the
three phases of downsample_rate=3 for two of the cases (asserted equal to slices for all) and
`quat_fk`'s positions of it; per decode case (drifting channels written with this package's `format_bvh`, whose text the CPU test pins to
the reference's byte for byte) the same; per retarget case the retargeted joints; and the seconds per call, among them the 4096-frame
24-joint clip and the 60-frame 22-joint retarget tools/bvh_bench.py prints beside its own.

Asserted here, before anything is written, every distance printed: the inputs are clear of the discontinuities
(bvh_fixture.assert_clear); per output the reference is no further from the fixture in float64 than the suite's bar allows its peer, the
fixture in float32 (4 x its own distance, floor 1e-6: the reference computes these in float32 too, so neither is the more exact) -- and
where the reference works in float64 (the retarget's accumulation) no further than the float32 fixture itself; signs, hierarchies and
joint orders are equal exactly."""
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
from make_golden import SEED  # noqa: E402
import bvh_fixture as bf  # noqa: E402
from mst_amd.utils import bvh  # noqa: E402

DS3_KEPT = ("w6", "d31")
ANIM = ("quats", "pos", "offsets", "parents", "end_offsets")


def best(fn, n=3):
    t, out = 1e9, None
    for _ in range(n):
        t0 = time.perf_counter()
        out = fn()
        t = min(t, time.perf_counter() - t0)
    return out, t


def peers(key, ref, a32, a64, strict=False):
    own, got = bf.rel(a32, a64), bf.rel(ref, a64)
    print(f"{key}: reference vs fixture f64 {got:.3e}; fixture f32 vs f64 {own:.3e}")
    assert got <= (own if strict else bf.bar(own)), (key, got, own)


def store_anim(out, key, a, skip=()):
    for n in ANIM:
        v = getattr(a, n)
        if v is not None and n not in skip:
            out[f"{key}|{n}"] = np.asarray(v)
    out[f"{key}|bones"] = np.array(a.bones)


def read_all(bu, ru, out, key, path, sk, ch):
    """The reference's readers on one file; checked against the fixture's decode of the channel rows `ch` of skeleton `sk`."""
    f32, f64 = bf.decode(ch, sk, np.float32), bf.decode(ch, sk, np.float64)
    bf.assert_clear(dots=f64["dots"])
    flips = int((f64["signs"][1:] != f64["signs"][:-1]).sum())
    assert flips > 0, key
    plain = bu.read_bvh(path)
    ends, seconds = best(lambda: bu.read_bvh(path, end_sites=True))
    assert ends.quats.shape[1] == sk.joints and list(ends.parents) == list(sk.parents) and list(ends.bones) == sk.names, key
    assert ((ends.quats * f64["rotations"]).sum(-1) > 0).all(), key                      # every sign decision
    peers(f"{key} quats ({flips} sign changes)", ends.quats, f32["rotations"], f64["rotations"])
    peers(f"{key} pos", ends.pos, f32["local_positions"], f64["local_positions"])
    gp = ru.wrap(ru.quat_fk, ends.quats, ends.pos, ends.parents)[1]
    peers(f"{key} quat_fk", gp, f32["positions"], f64["positions"])
    keep = sk.not_end_index
    assert np.array_equal(plain.quats, ends.quats[:, keep]) and list(plain.parents) == sk.simple_parents, key
    assert np.array_equal(plain.pos, ends.pos[:, keep]), key
    store_anim(out, f"{key}|read", plain, skip=("quats", "pos"))      # both equal the End Site read's without its End Sites, asserted above
    store_anim(out, f"{key}|read_ends", ends)
    out[f"{key}|fk"] = gp.astype(np.float32)
    for i, a in enumerate(bu.read_bvh(path, downsample_rate=3)):
        assert np.array_equal(a.quats, plain.quats[i::3]) and np.array_equal(a.pos, plain.pos[i::3]), key
        if key in DS3_KEPT:                                             # the others equal the slices too: asserted, not stored
            out[f"{key}|ds3|{i}|quats"], out[f"{key}|ds3|{i}|pos"] = a.quats, a.pos
    out[f"{key}|read_seconds"] = np.array(seconds)


def main():
    mg.install_shims()
    bu = importlib.import_module("data_loaders.humanml.common.bvh_utils")
    ru = importlib.import_module("utils.rotation")
    mp = importlib.import_module("data_loaders.humanml.scripts.motion_process")
    torch.set_num_threads(8)
    out = {}
    tmp = tempfile.mkdtemp()
    for name in bf.GOLDEN_WRITE:
        names, par, off, end, order, positions, q, pos = bf.writer_case(SEED, name)
        bf.assert_clear(writer=q, order=order)
        path = os.path.join(tmp, name + ".bvh")
        _, seconds = best(lambda: bu.save_bvh(path, bu.Anim(q.copy(), pos.copy(), off.copy(), np.array(par), list(names), end.copy()), 1 / 30, order,
                                              positions))
        text = open(path, "rb").read()
        seq = bvh.writer_sequence(par)
        assert seq == list(range(len(par))), name            # depth-first joints: the reference's unpermuted reads are the right ones
        rad = ru.wrap(ru.q2eul, q[:, seq], order[::-1])
        deg = np.degrees(rad)
        assert deg.dtype == np.float32
        cols = ["xyz".index(a) for a in order]
        rows = np.concatenate([pos[:, :, :], deg[..., cols]], -1).reshape(len(q), -1) if positions else \
            np.concatenate([pos[:, 0], deg[..., cols].reshape(len(q), -1)], -1)
        sk, seq2 = bvh.writer_skeleton(names, par, off, end, order, positions, 1 / 30)
        assert seq2 == seq and bvh.format_bvh(sk, rows).encode() == text, name
        f32, f64 = (bf.channels_from_quats(q, pos[:, 0], par, order, pos if positions else None, dt) for dt in (np.float32, np.float64))
        d = np.abs((rows - f64 + 180) % 360 - 180).max()
        own = np.abs((f32 - f64 + 180) % 360 - 180).max()
        print(f"{name} degrees: reference vs fixture f64 {d:.3e}; fixture f32 vs f64 {own:.3e} (absolute, modulo 360)")
        assert d <= bf.bar(own / 180) * 180, (name, d, own)
        out[f"{name}|text"] = np.frombuffer(text, np.uint8)
        out[f"{name}|deg"], out[f"{name}|channels"] = deg, rows.astype(np.float32)
        out[f"{name}|save_seconds"] = np.array(seconds)
        psk, pch = bvh.parse_bvh(text.decode())
        read_all(bu, ru, out, name, path, psk, pch)
    for name, (Jf, T, layout, order) in bf.GOLDEN_DECODE.items():
        sk = bf.file_skeleton(SEED, name, Jf, layout, order)
        ch = bf.channels(SEED, name, sk, T)[0]
        path = os.path.join(tmp, name + ".bvh")
        with open(path, "w") as fh:
            fh.write(bvh.format_bvh(sk, ch))
        psk, pch = bvh.parse_bvh(path)
        assert psk.same_hierarchy(sk), name
        read_all(bu, ru, out, name, path, psk, pch)
    for J, T in bf.GOLDEN_RETARGET:
        sk, pos, tgt, l_idx = bf.retarget_case(SEED, J, T)
        got, seconds = best(lambda: mp.uniform_skeleton_basic(pos[0].copy(), torch.from_numpy(tgt.copy()), torch.from_numpy(sk.raw.copy()),
                                                              sk.chains, l_idx, sk.face))
        f32, _ = bf.retarget(pos[0], tgt, sk.raw, sk.chains, l_idx, sk.face, np.float32)
        f64, diag = bf.retarget(pos[0], tgt, sk.raw, sk.chains, l_idx, sk.face, np.float64)
        bf.assert_clear(retarget_diag=diag)
        peers(f"retarget J{J}T{T} ({got.dtype})", got, f32, f64, strict=True)
        out[f"retarget|J{J}T{T}"] = np.asarray(got, np.float32)
        out[f"retarget|J{J}T{T}|seconds"] = np.array(seconds)
        print(f"retarget J{J}T{T}: {seconds * 1e3:.1f} ms")
    # the sizes tools/bvh_bench.py measures: seconds only
    sk = bf.file_skeleton(SEED, "bench", 32, "root6", "zyx")
    ch = bf.channels(SEED, "bench", sk, 4096)[0]
    path = os.path.join(tmp, "bench.bvh")
    with open(path, "w") as fh:
        fh.write(bvh.format_bvh(sk, ch))
    a, t_read = best(lambda: bu.read_bvh(path), 2)
    _, t_save = best(lambda: bu.save_bvh(path, bu.Anim(a.quats.copy(), a.pos.copy(), a.offsets.copy(), a.parents.copy(), list(a.bones))), 2)
    out["seconds|read_bvh|T4096J24"], out["seconds|save_bvh|T4096J24"] = np.array(t_read), np.array(t_save)
    print(f"4096 frames, {a.quats.shape[1]} joints: read_bvh {t_read:.3f} s, save_bvh {t_save:.3f} s")
    assert a.quats.shape[1] == 24
    path = os.path.join(HERE, "bvh.npz")
    np.savez_compressed(path, **out)
    print("bvh.npz", os.path.getsize(path) // 1024, "KiB;", len(out), "arrays")
    assert os.path.getsize(path) < 500 * 1024


if __name__ == "__main__":
    main()
