"""Golden vectors of the pose-track path: the reference's own utils/process_smpl_from_hybrik.py -- `downsample`, `joints_downsample`,
`amass_to_pose`, `pos2hmlrep` -- and the fractional branch of its `read_bvh` (data_loaders/humanml/common/bvh_utils.py:251-287), imported
unmodified and run on the CPU on the seeded cases of tests/track_fixture.py.  Run in the authoring container only (the reference
checkout on the path):
    python tests/golden/make_golden_track.py -> track.npz

What is the reference's and what is not.  `human_body_prior` and `imageio` are not installed, so both are stubbed in sys.modules; the
`BodyModel` stub returns `Jtr` from the seeded joint table (tests/track_fixture.py's 40-vertex body) by the restated Rodrigues form and
chain in float32, as make_golden_smplify.py stubs `smplx`.  The module reads an example clip from a fixed relative path when it is
imported: that file is written into a temporary working directory.  `pos2hmlrep` reads `t2m_raw_offsets` when it is called: the module's
name is bound to the fixture's unit bone directions first, so no table of the reference enters the file; `tgt_offsets` is what the module
computed at import from the example clip, and is stored.  Everything else -- the file readers, `rotm2q`, `qslerp`, `lerp`,
`q2axangle`, the frame loop, the re-axing, `uniform_skeleton_basic`, `process_file`, `read_bvh` -- is the reference's code as it stands.

Stored:
  `ds|T<frames>|<num>_<den>|rot, pos, joints`   `downsample` and `joints_downsample` of a seeded track (rot float32, pos and joints float64)
  `file|<case>|model, est`                      `amass_to_pose` per case of track_fixture.GOLDEN_FILES (float64), and
  `file|<case>|rotm2q`                          the quaternions `rotm2q` returned for its matrices, LAPACK's signs included
  `hml|joints, tgt_offsets, rows`               `pos2hmlrep` of a seeded humanoid clip
  `bvh|r15|...`, `bvh|r15e|...`                 `read_bvh(path, downsample_rate=1.5)` without and with End Sites of a file this package's
                                                `format_bvh` wrote
Asserted before anything is written, every distance printed: the output counts equal track_fixture.COUNTS; the float64 restatement with
the reference's formula (on the recorded `rotm2q` quaternions for matrix input) is no further from every stored array than the suite's
bar allows the float32 restatement (4 x its own distance from float64, floor 1e-6), translations to 1e-12; the closed-form `rotm2q` equals
the recorded quaternions up to sign; the file stays below 200 KB."""
import importlib
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import bvh_fixture as bf  # noqa: E402
import track_fixture as tf  # noqa: E402
from mst_amd.utils import bvh  # noqa: E402

TABLE = tf.joint_table(tf.body())


class BodyModel:
    """What process_smpl_from_hybrik.py asks of human_body_prior's BodyModel: `.to`, `.f`, and a call that returns `.Jtr`."""

    def __init__(self, bm_fname=None, num_betas=10, num_dmpls=None, dmpl_fname=None):
        self.f = torch.zeros(1, 3, dtype=torch.long)

    def to(self, device):
        return self

    def __call__(self, pose_body=None, betas=None, root_orient=None):
        theta = torch.cat([root_orient, pose_body], 1).reshape(1, tf.CHAIN, 3).numpy().astype(np.float32)
        J0, Jd = TABLE
        J = J0.copy()
        b = betas.numpy().astype(np.float32).reshape(-1)
        for n in range(tf.NB):
            J = J + Jd[..., n] * b[n]
        return types.SimpleNamespace(Jtr=torch.from_numpy(tf.chain(tf.rodrigues(theta), J).astype(np.float32)))


def stub_modules():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
    mod("human_body_prior")
    mod("human_body_prior.tools")
    mod("human_body_prior.tools.omni_tools", copy2cpu=lambda t: t.detach().cpu().numpy())
    mod("human_body_prior.body_model")
    mod("human_body_prior.body_model.body_model", BodyModel=BodyModel)
    mod("imageio")


def peers(key, ref, a32, a64, dist=tf.distance):
    own, got = dist(a32, a64), dist(ref, a64)
    print(f"{key}: reference vs fixture f64 {got:.3e}; fixture f32 vs f64 {own:.3e}")
    assert got <= tf.bar(own), (key, got, own)


def main():
    mg.install_shims()                                      # np.float, which the reference's quaternion.py needs, and the path
    stub_modules()
    out = {}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "processed_data", "HumanML3D", "new_joints"))
        example = tf.human_clip("example", 4, scale=1.1)
        np.save(os.path.join(tmp, "processed_data", "HumanML3D", "new_joints", "001234.npy"), example.reshape(len(example), -1))
        os.chdir(tmp)
        try:
            psh = importlib.import_module("utils.process_smpl_from_hybrik")
        finally:
            os.chdir(cwd)
        bu = importlib.import_module("data_loaders.humanml.common.bvh_utils")
        assert psh.__file__.startswith(mg.REF) and bu.__file__.startswith(mg.REF)
        recorded = []
        rotm2q = psh.rotm2q
        psh.rotm2q = lambda R: recorded.append(rotm2q(R)) or recorded[-1]

        # ---- downsample, joints_downsample
        for (T, rate), count in tf.COUNTS.items():
            tr = tf.track(tf.SEED, T, flips=T == 9)
            q, p, j = (torch.from_numpy(tr[k]) for k in ("quats", "transl", "joints"))
            rot, pos = psh.downsample(q, p, float(rate))
            jo = psh.joints_downsample(j, float(rate))
            key = f"ds|T{T}|{rate.numerator}_{rate.denominator}"
            assert rot.shape[0] == pos.shape[0] == jo.shape[0] == count == tf.out_frames(T, rate), (key, rot.shape, count)
            assert rot.dtype == torch.float32 and pos.dtype == torch.float64 and jo.dtype == torch.float64
            peers(key + " rot", rot.numpy(), tf.resample_quats(tr["quats"], rate, np.float32), tf.resample_quats(tr["quats"], rate, np.float64))
            for name, got, src in (("pos", pos, tr["transl"]), ("joints", jo, tr["joints"])):
                d = tf.distance(got.numpy(), tf.lerp64(src, rate, as_reference=True))
                print(f"{key} {name}: reference vs fixture f64 {d:.3e}")
                assert d < 1e-12, (key, name, d)
            out[key + "|rot"], out[key + "|pos"], out[key + "|joints"] = rot.numpy(), pos.numpy(), jo.numpy()

        # ---- amass_to_pose
        for name, (kind, T, fps, with_trans, cut) in tf.GOLDEN_FILES.items():
            tr, extra = tf.golden_track(name)
            path = os.path.join(tmp, f"{name}.{kind}")
            tf.write_track(path, tr, kind)
            trans_path = ""
            if cut:
                trans_path = os.path.join(tmp, name + "_trans.pkl")
                tf.write_trans(trans_path, extra)
            del recorded[:]
            model, est = psh.amass_to_pose(path, fps=fps, trans_path=trans_path, with_trans=with_trans)
            rate = tf.Fraction(fps, 20)
            n = cut or T
            case = {"betas": tr["betas"], "transl": extra if cut else tr["transl"]}
            if "joints" in tr:
                case["joints"] = tr["joints"][:n]
            if kind == "pkl":
                assert not recorded and est is model
                case["quats"] = tr["quats"]
            else:
                assert len(recorded) == 1
                rq = recorded[0].numpy().astype(np.float32)
                out[f"file|{name}|rotm2q"] = rq
                d = tf.quat_distance(tf.rotm2q(tr["mats"][:n].astype(np.float64)), rq)
                print(f"{name}: closed-form rotm2q vs the reference's eigenvector, up to sign {d:.3e}; "
                      f"{int((rq[..., 0] < 0).sum())} of {rq[..., 0].size} came back with w < 0")
                assert d < 1e-5, (name, d)
                case["quats"] = rq                          # the reference's formula on the reference's own signs
            assert model.shape == (tf.out_frames(n, rate), 22, 3), (name, model.shape)
            f32, f64 = (tf.track_joints(case, TABLE, rate, dt, with_trans) for dt in (np.float32, np.float64))
            peers(f"{name} model joints", model, f32[0], f64[0])
            if kind != "pkl":
                peers(f"{name} estimator joints", est, f32[1], f64[1])
                out[f"file|{name}|est"] = np.asarray(est, np.float64)
            out[f"file|{name}|model"] = np.asarray(model, np.float64)

        # ---- pos2hmlrep
        sk = tf.human()
        psh.t2m_raw_offsets = sk.raw.copy()
        tgt = psh.tgt_offsets.numpy() if torch.is_tensor(psh.tgt_offsets) else np.asarray(psh.tgt_offsets)
        joints = tf.human_clip("hml", 9)
        rows = psh.pos2hmlrep(joints.copy())
        assert rows.shape == (8, 263), rows.shape
        peers("pos2hmlrep", rows, tf.hml_rows(joints, tgt, np.float32), tf.hml_rows(joints, tgt, np.float64))
        out["hml|joints"], out["hml|tgt_offsets"], out["hml|rows"] = joints, np.asarray(tgt, np.float32), np.asarray(rows, np.float32)

        # ---- read_bvh at a fractional rate
        fsk = bf.file_skeleton(bf.SEED, "track/r15", 9, "all6", "zyx")
        ch = bf.channels(bf.SEED, "track/r15", fsk, 9)[0]
        path = os.path.join(tmp, "r15.bvh")
        with open(path, "w") as fh:
            fh.write(bvh.format_bvh(fsk, ch))
        psk, pch = bvh.parse_bvh(path)
        f32, f64 = bf.decode(pch, psk, np.float32), bf.decode(pch, psk, np.float64)
        bf.assert_clear(dots=f64["dots"])
        rate = tf.Fraction(3, 2)
        for key, ends in (("bvh|r15", False), ("bvh|r15e", True)):
            got = bu.read_bvh(path, downsample_rate=1.5, end_sites=ends)
            assert isinstance(got, list) and len(got) == 1
            a = got[0]
            keep = list(range(psk.joints)) if ends else psk.not_end_index
            assert a.quats.shape == (tf.out_frames(9, rate), len(keep), 4) and a.quats.dtype == np.float32 and a.pos.dtype == np.float32
            peers(key + " quats", a.quats, *(tf.resample_quats(f["rotations"], rate, dt)[:, keep] for f, dt in ((f32, np.float32), (f64, np.float64))))
            peers(key + " pos", a.pos, *(tf.resample_points(f["local_positions"], rate, dt)[:, keep] for f, dt in ((f32, np.float32), (f64, np.float64))))
            out[key + "|quats"], out[key + "|pos"], out[key + "|offsets"] = a.quats, a.pos, np.asarray(a.offsets)
            out[key + "|parents"], out[key + "|bones"] = np.asarray(a.parents), np.array(a.bones)
    path = os.path.join(HERE, "track.npz")
    np.savez_compressed(path, **out)
    print("track.npz", os.path.getsize(path), "bytes;", len(out), "arrays")
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
