"""Golden vectors of the SMPL stage: the reference's own `model.smpl.SMPL` and `model.rotation2xyz.Rotation2xyz`, imported unmodified
and run for real on the seeded cases of tests/smpl_fixture.py.  Run in the authoring container only (the reference checkout on the
path):
    python tests/golden/make_golden_smpl.py -> smpl.npz

What is the reference's and what is not.  `smplx` and a SMPL body file do not exist here, so `smplx.SMPLLayer` and
`smplx.lbs.vertices2joints` are stubbed in sys.modules by tests/smpl_fixture.py's float64 `lbs` over a synthetic body, and `utils.config`
by a module that names a temporary J_regressor_extra file.  Everything above that layer is the reference's code as it stands: the
joint tables and `maps` of model/smpl.py, the extra-regressor concatenation of its `forward`, and all of Rotation2xyz.__call__ --
the conversions of utils/rotation_conversions.py, masking, root subtraction, translation.  The `lbs` under them is a restatement,
not smplx.  The runs are in float64 (x, betas and glob_rot handed over as float64), stored as float32.

Stored (inputs are rebuilt from the seed):
  `maps|<name>`, `root|<name>`                  SMPL.maps and JOINTSTYPE_ROOT
  `r2x|<pose_rep>|<jointstype>|g<0/1>|t<0/1>v<0/1>|b<0/1>`   Rotation2xyz outputs [3, n, 3, 5] at V = 83, lengths (5, 3, 1); b0: betas=None,
                                                beta=0.7; b1: given betas.  translation=False reads the sample without its last row.
                                                t0v1 and t1v0 are asserted equal to t0v0 here and stored once: `alias|<key>` names the key
                                                that holds the array.
  `conv|rot6d / rotvec / rotquat` (+ `|in`)     rotation_6d_to_matrix, axis_angle_to_matrix (small angles included) and
                                                quaternion_to_matrix on seeded float64 inputs
Asserted before anything is written: the fixture's float64 pipeline equals every reference output to 1e-12, the package's index tables
equal the reference's, and the file is smaller than 1 MB."""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import smpl_fixture as sf  # noqa: E402

REF = os.environ.get("MST_REFERENCE", "/root/reference")
V, B, T, LENGTHS = 83, 3, 5, (5, 3, 1)
BODY = sf.synthetic_body(V)


def install_stubs(tmp):
    class Output:
        pass

    class SMPLLayer(torch.nn.Module):
        def __init__(self, model_path=None, **kwargs):
            super().__init__()
            self.num_betas = sf.NB
            self.faces = BODY["faces"]

        def forward(self, body_pose=None, global_orient=None, betas=None, **kwargs):
            n = body_pose.shape[0]
            rot = torch.cat([global_orient.reshape(n, 1, 3, 3), body_pose.reshape(n, -1, 3, 3)], 1)
            verts, joints = sf.lbs(BODY, rot, betas, torch.float64)
            o = Output()
            o.vertices, o.joints = verts, joints[:, :sf.NJ + sf.NIDS]
            return o

    smplx, lbs = types.ModuleType("smplx"), types.ModuleType("smplx.lbs")
    smplx.SMPLLayer, smplx.lbs = SMPLLayer, lbs
    lbs.vertices2joints = lambda J, v: torch.einsum("bik,ji->bjk", v, J.to(v.dtype))
    sys.modules["smplx"], sys.modules["smplx.lbs"] = smplx, lbs
    extra = os.path.join(tmp, "J_regressor_extra.npy")
    np.save(extra, BODY["J_regressor_extra"])
    cfg = types.ModuleType("utils.config")
    cfg.SMPL_MODEL_PATH, cfg.JOINT_REGRESSOR_TRAIN_EXTRA = os.path.join(tmp, "SMPL_NEUTRAL.pkl"), extra
    sys.path.insert(0, REF)
    import utils  # noqa: F401  (the reference's package)
    sys.modules["utils.config"] = cfg


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        install_stubs(tmp)
        import model.smpl as rsmpl
        import model.rotation2xyz as rr2x
        import utils.rotation_conversions as geo
        assert rsmpl.__file__.startswith(REF) and rr2x.__file__.startswith(REF)
        r2x = rr2x.Rotation2xyz(device="cpu")
        # the extra regressor is registered in float32 by the reference; the stubbed vertices2joints casts it, so hand it over in double
        r2x.smpl_model.J_regressor_extra = torch.as_tensor(BODY["J_regressor_extra"])
        maps = {k: np.asarray(v) for k, v in r2x.smpl_model.maps.items()}
        roots = dict(rsmpl.JOINTSTYPE_ROOT)
        for k, v in maps.items():
            out[f"maps|{k}"] = v.astype(np.int64)
        for k, v in roots.items():
            out[f"root|{k}"] = np.int64(v)
        import mst_amd  # noqa: F401
        from mst_amd.model import smpl as mine
        assert sorted(mine.joint_maps()) == sorted(maps) and all(np.array_equal(mine.joint_maps()[k], maps[k]) for k in maps)
        assert mine.JOINTSTYPE_ROOT == roots and sorted(mine.JOINTSTYPES) == sorted(rr2x.JOINTSTYPES)

        mask = sf.lengths_mask(LENGTHS, T)
        live = int(mask.sum())
        worst = 0.0
        for rep in sf.FEATS:
            x25 = sf.sample(rep, B, T, rows=25).double()
            for jt in sf.JOINTSTYPES:
                for glob in (1, 0):
                    full = x25 if glob else x25[:, 1:]                          # glob=False: 23 rotation rows and the translation
                    for bt in (0, 1):
                        betas = sf.given_betas(live).double() if bt else None
                        base = None
                        for tr, vt in ((0, 0), (0, 1), (1, 0), (1, 1)):
                            x = full if tr else full[:, :-1]
                            kw = dict(mask=mask, pose_rep=rep, translation=bool(tr), glob=bool(glob), jointstype=jt, vertstrans=bool(vt),
                                      betas=betas, beta=0.7, glob_rot=None if glob else np.asarray(sf.GLOB_ROT, np.float64))
                            got = r2x(x.clone(), **kw).numpy()
                            want = sf.rotation2xyz(BODY, maps, roots, x, **kw).numpy()
                            d = sf.distance(want, got)
                            worst = max(worst, d)
                            assert d < 1e-12, (rep, jt, glob, tr, vt, bt, d)
                            key = f"r2x|{rep}|{jt}|g{glob}|t{tr}v{vt}|b{bt}"
                            if (tr, vt) == (0, 0):
                                base = got
                            if (tr, vt) in ((0, 1), (1, 0)):
                                assert np.array_equal(got, base), key
                                out[f"alias|{key}"] = np.array(f"r2x|{rep}|{jt}|g{glob}|t0v0|b{bt}")
                            else:
                                out[key] = got.astype(np.float32)
        print(f"fixture float64 vs reference: worst distance {worst:.3e}")
        g = np.random.default_rng(11)
        d6 = sf.sample("rot6d", 2, 4, rows=6).double().permute(0, 3, 1, 2)[..., :5, :]
        aa = torch.as_tensor(g.standard_normal((40, 3)))
        aa[:4] = torch.as_tensor([[0.0, 0.0, 0.0], [3e-7, -2e-7, 1e-7], [9.9e-7, 0.0, 0.0], [1.1e-6, 0.0, 0.0]])
        q = torch.as_tensor(g.standard_normal((40, 4)))
        for name, fn, mine_fn, inp in (("rot6d", geo.rotation_6d_to_matrix, sf.rot6d_to_matrix, d6), ("rotvec", geo.axis_angle_to_matrix, sf.rotvec_to_matrix, aa),
                                       ("rotquat", geo.quaternion_to_matrix, sf.quat_to_matrix, q)):
            res = fn(inp).numpy()
            assert sf.distance(mine_fn(inp).numpy(), res) < 1e-12, name
            out[f"conv|{name}|in"], out[f"conv|{name}"] = inp.numpy(), res
    path = os.path.join(HERE, "smpl.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"{path}: {len(out)} arrays, {size} bytes")
    assert size < 1_000_000


if __name__ == "__main__":
    main()
