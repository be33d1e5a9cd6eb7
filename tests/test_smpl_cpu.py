"""The SMPL stage without a GPU: the index tables against the reference's (tests/golden/smpl.npz), SMPLBody's validation and file
constructors, the OBJ writer, save_npy's keys, and the bad-argument codes of the mst_smpl_* entry points."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
import smpl_fixture as sf
from conftest import GOLDEN
from mst_amd import _native
from mst_amd.model import smpl
from mst_amd.model.rotation2xyz import JOINTSTYPES, Rotation2xyz
from mst_amd.visualize import vis_utils


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "smpl.npz"))


def body_arrays(V=40, **kw):
    return sf.synthetic_body(V, **kw)


def test_index_tables_equal_the_reference(gold):
    maps = smpl.joint_maps()
    assert sorted(maps) == sorted(k.split("|")[1] for k in gold.files if k.startswith("maps|"))
    for k, v in maps.items():
        assert np.array_equal(v, gold[f"maps|{k}"]), k
    assert smpl.JOINTSTYPE_ROOT == {k.split("|")[1]: int(gold[k]) for k in gold.files if k.startswith("root|")}
    assert sorted(JOINTSTYPES) == ["a2m", "a2mpl", "smpl", "vertices", "vibe"]
    assert smpl.SMPL.num_betas == 10 and list(smpl.SMPL_PARENTS) == sf.PARENTS


def test_fixture_conversions_equal_the_reference(gold):
    for name, fn in (("rot6d", sf.rot6d_to_matrix), ("rotvec", sf.rotvec_to_matrix), ("rotquat", sf.quat_to_matrix)):
        got = fn(torch.as_tensor(gold[f"conv|{name}|in"])).numpy()
        assert sf.distance(got, gold[f"conv|{name}"]) < 1e-12, name


def test_body_is_built_on_the_host_and_keeps_its_arrays():
    a = body_arrays()
    b = smpl.SMPLBody.from_arrays(**a)
    assert b.num_vertices == 40 and b.shapedirs.shape == (40, 3, 10) and b.posedirs.shape == (207, 120)
    assert np.array_equal(b.faces, a["faces"]) and np.array_equal(b.vertex_ids, a["vertex_ids"])
    assert np.allclose(b.J0, a["J_regressor"] @ a["v_template"], atol=1e-6)
    assert np.allclose(b.Jdirs, np.einsum("jv,vci->jci", a["J_regressor"], a["shapedirs"]), atol=1e-7)
    # the files' [V, 3, 207] posedirs and more than 10 shape directions
    pd = a["posedirs"].T.reshape(40, 3, 207)
    sd = np.concatenate([a["shapedirs"], np.ones((40, 3, 6))], -1)
    c = smpl.SMPLBody.from_arrays(**dict(a, posedirs=pd, shapedirs=sd))
    assert np.array_equal(c.posedirs, b.posedirs) and np.array_equal(c.shapedirs, b.shapedirs)
    m = smpl.SMPL(b)
    assert m.faces is b.faces and m.eval() is m and sorted(m.maps) == ["a2m", "a2mpl", "smpl", "vibe"]


@pytest.mark.parametrize("change, word", [
    (lambda a: a.update(v_template=a["v_template"][:, :2]), "v_template"),
    (lambda a: a.update(shapedirs=a["shapedirs"][..., :9]), "shapedirs"),
    (lambda a: a.update(posedirs=a["posedirs"][:-1]), "posedirs"),
    (lambda a: a.update(J_regressor=a["J_regressor"][:23]), "J_regressor"),
    (lambda a: a.update(parents=a["parents"][:23]), "24"),
    (lambda a: a.update(parents=np.r_[0, a["parents"][1:]]), "parents[0]"),
    (lambda a: a.update(parents=np.r_[a["parents"][:5], 5, a["parents"][6:]]), "parents[5]"),
    (lambda a: a.update(lbs_weights=a["lbs_weights"] * 1.001), "lbs_weights"),
    (lambda a: a.update(J_regressor=a["J_regressor"] * 0.999), "J_regressor"),
    (lambda a: a.update(faces=a["faces"] + 40), "faces"),
    (lambda a: a.update(J_regressor_extra=a["J_regressor_extra"][:8]), "J_regressor_extra"),
    (lambda a: a.update(vertex_ids=a["vertex_ids"][:20]), "vertex_ids"),
    (lambda a: a.update(vertex_ids=np.r_[a["vertex_ids"][:20], 40]), "vertex id 40"),
    (lambda a: a.update(v_template=a["v_template"] * np.nan), "finite"),
])
def test_body_validation(change, word):
    a = body_arrays()
    change(a)
    with pytest.raises(ValueError, match=word.replace("[", r"\[").replace("]", r"\]")):
        smpl.SMPLBody.from_arrays(**a)


def test_rows_within_the_tolerance_pass():
    a = body_arrays()
    smpl.SMPLBody.from_arrays(**dict(a, lbs_weights=a["lbs_weights"] * (1 + 5e-5)))


def smpl_file_dict(a):
    kin = np.stack([np.r_[2 ** 32 - 1, a["parents"][1:]], np.arange(24)]).astype(np.int64)
    return {"v_template": a["v_template"], "shapedirs": a["shapedirs"], "posedirs": a["posedirs"].T.reshape(-1, 3, 207), "J_regressor": a["J_regressor"],
            "kintree_table": kin, "weights": a["lbs_weights"], "f": a["faces"]}


def same_body(b, c):
    return all(np.array_equal(getattr(b, n), getattr(c, n)) for n in ("v_template", "shapedirs", "posedirs", "J_regressor", "parents", "lbs_weights",
                                                                      "faces", "J_regressor_extra", "vertex_ids", "J0", "Jdirs"))


def test_from_npz_and_from_pkl_round_trip(tmp_path):
    a = body_arrays()
    ref = smpl.SMPLBody.from_arrays(**a)
    d = smpl_file_dict(a)
    np.savez(tmp_path / "body.npz", **d)
    np.save(tmp_path / "extra.npy", a["J_regressor_extra"])
    assert same_body(ref, smpl.SMPLBody.from_npz(str(tmp_path / "body.npz"), str(tmp_path / "extra.npy"), a["vertex_ids"]))
    np.savez(tmp_path / "own.npz", **a)                                           # this class's own names, everything inside
    assert same_body(ref, smpl.SMPLBody.from_npz(str(tmp_path / "own.npz")))
    import scipy.sparse
    with open(tmp_path / "body.pkl", "wb") as fh:
        pickle.dump(dict(d, J_regressor=scipy.sparse.csc_matrix(a["J_regressor"])), fh, protocol=2)
    assert same_body(ref, smpl.SMPLBody.from_pkl(str(tmp_path / "body.pkl"), a["J_regressor_extra"], a["vertex_ids"]))
    with pytest.raises(KeyError, match="vertex_ids"):
        smpl.SMPLBody.from_pkl(str(tmp_path / "body.pkl"), a["J_regressor_extra"])


def test_pickle_that_needs_a_missing_module_says_so(tmp_path):
    p = tmp_path / "chumpy_like.pkl"
    p.write_bytes(b"cmodule_that_is_not_installed_xyz\nCh\n.")        # GLOBAL of a module that does not exist
    with pytest.raises(ImportError, match="module_that_is_not_installed_xyz.*not installed"):
        smpl.SMPLBody.from_pkl(str(p))


def test_no_cpu_path_and_no_bundled_body():
    b = smpl.SMPLBody.from_arrays(**body_arrays())
    with pytest.raises(TypeError, match="SMPLBody"):
        Rotation2xyz("cpu")
    r = Rotation2xyz("cpu", body=b)
    x = sf.sample("rot6d", 1, 2)
    assert r(x, None, "xyz", True, True, "smpl", True) is x
    with pytest.raises(RuntimeError, match="GPU only"):
        r(x, None, "rot6d", True, True, "smpl", True)
    with pytest.raises(TypeError, match="global rotation"):
        r(x, None, "rot6d", True, False, "smpl", True)
    with pytest.raises(NotImplementedError):
        r(x, None, "rot6d", True, True, "bones", True)
    with pytest.raises(RuntimeError, match="GPU only"):
        smpl.SMPL(b).forward(torch.zeros(1, 23, 3, 3), torch.zeros(1, 3, 3))


def test_obj_writer_is_read_back(tmp_path):
    g = np.random.default_rng(2)
    v = (g.standard_normal((57, 3)) * 3).astype(np.float32)
    f = g.integers(0, 57, (30, 3))
    vis_utils.write_obj(str(tmp_path / "m.obj"), v, f)
    lines = open(tmp_path / "m.obj").read().splitlines()
    assert len(lines) == 87 and all(l.startswith("v ") for l in lines[:57]) and all(l.startswith("f ") for l in lines[57:])
    assert min(int(t) for l in lines[57:] for t in l.split()[1:]) >= 1
    rv, rf = vis_utils.read_obj(str(tmp_path / "m.obj"))
    assert np.array_equal(rv.astype(np.float32), v) and np.array_equal(rf, f)


def test_save_npy_writes_the_reference_keys(tmp_path):
    o = object.__new__(vis_utils.npy2obj)
    clip = np.arange(25 * 6 * 7, dtype=np.float32).reshape(1, 25, 6, 7)
    o.motions = {"motion": clip, "text": ["a person walks"]}
    o.real_num_frames, o.faces, o.vertices = 5, np.zeros((4, 3), np.int64), torch.zeros(1, 30, 3, 7)
    o.save_npy(str(tmp_path / "out.npy"))
    d = np.load(tmp_path / "out.npy", allow_pickle=True).item()
    assert sorted(d) == ["faces", "length", "motion", "root_translation", "text", "thetas", "vertices"]
    assert d["motion"].shape == (25, 6, 5) and d["thetas"].shape == (24, 6, 5) and d["root_translation"].shape == (3, 5)
    assert tuple(d["vertices"].shape) == (30, 3, 5) and d["length"] == 5 and d["text"] == "a person walks"
    assert np.array_equal(d["root_translation"], clip[0, -1, :3, :5])


def test_entry_points_report_bad_arguments_without_a_gpu():
    lib = _native.lib()
    one = C.c_void_p(256)                                   # never dereferenced: every call below is refused on the host
    par = (C.c_int32 * 24)(*sf.PARENTS)
    rot = (C.c_float * 3)(0, 0, 0)

    def pose(joints=24, vertices=83, parents=par, x=one, live=4, rep=0, rows=24, ws=one, ids=one):
        return lib.mst_smpl_pose(x, 1, 1, 1, 1, ids, live, 2, 4, rows, joints, vertices, 0, rep, 1, rot, None, 0.0, one, one, parents, -1, ws,
                                 None, None, None)
    err = lambda: lib.mst_last_error().decode()
    assert pose(joints=22) != 0 and "24" in err()
    assert pose(vertices=0) != 0 and "vertices" in err()
    assert pose(x=None) != 0 and "null" in err()
    assert pose(ws=None) != 0 and "null" in err()
    assert pose(live=0) != 0 and "live" in err()
    assert pose(rep=4) != 0 and "pose_rep" in err()
    assert pose(rows=23) != 0 and "rotation rows" in err()
    assert pose(ids=None) != 0 and "frame ids" in err()
    bad = list(sf.PARENTS)
    bad[7] = 7
    assert pose(parents=(C.c_int32 * 24)(*bad)) != 0 and "parents[7]" in err()
    bad = list(sf.PARENTS)
    bad[0] = 0
    assert pose(parents=(C.c_int32 * 24)(*bad)) != 0 and "parents[0]" in err()

    assert lib.mst_smpl_pack_body(one, one, 0, one, None) != 0 and "vertices" in err()
    assert lib.mst_smpl_pack_body(None, one, 83, one, None) != 0 and "null" in err()
    assert lib.mst_smpl_packed_bytes(0) == -1
    assert lib.mst_smpl_packed_bytes(83) == 3 * 224 * 96 * 4 and lib.mst_smpl_packed_bytes(6890) == 216 * 224 * 96 * 4
    assert lib.mst_smpl_workspace_bytes(0, 83, 0) == -1 and lib.mst_smpl_workspace_bytes(4, -1, 0) == -1
    small, big = lib.mst_smpl_workspace_bytes(9, 83, 0), lib.mst_smpl_workspace_bytes(9, 83, 1)
    assert small >= 9 * (288 + 224 + 72) * 4 and big - small >= 9 * 83 * 12 and big % 256 == 0

    def skin(packed=one, vertices=83, out=one, keep=0, ws=one):
        return lib.mst_smpl_skin(packed, one, one, vertices, keep, one, 4, 2, 4, ws, None, 0, 0, 0, out, 1, 1, 1, 1, None)
    assert skin(packed=None) != 0 and "null" in err()
    assert skin(vertices=0) != 0 and "vertices" in err()
    assert skin(ws=None) != 0 and "null" in err()
    assert skin(out=None) != 0 and "no output" in err()

    ids = (C.c_int32 * 21)(*range(21))
    jm = (C.c_int32 * 3)(0, 24, 53)

    def regress(ws=one, vertices=83, ids=ids, jm=jm, n=3, root=0):
        return lib.mst_smpl_regress(ws, one, ids, vertices, one, 4, 2, 4, jm, n, root, None, 0, 0, 0, one, None)
    assert regress(ws=None) != 0 and "null" in err()
    assert regress(vertices=0) != 0 and "vertices" in err()
    assert regress(vertices=20) != 0 and "vertex id 20" in err()
    assert regress(jm=(C.c_int32 * 3)(0, 24, 54)) != 0 and "map[2]" in err()
    assert regress(root=3) != 0 and "root" in err()
    assert regress(n=55) != 0 and "joints" in err()
