"""The evaluators' host side, without a GPU: the numpy restatement (tests/eval_fixture.py) against the reference's recorded outputs
(tests/golden/eval.npz), the state-dict packing of mst_amd.data_loaders.evaluator_wrapper, the reference's row order, every refusal, and
the host Frechet path of mst_amd.utils.metrics."""
import os

import numpy as np
import pytest
import torch

import eval_fixture as ef
import mst_amd  # noqa: F401
from conftest import GOLDEN
from mst_amd.data_loaders import evaluator_wrapper as ew
from mst_amd.utils import metrics as mt


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "eval.npz"))


def tensors(sd):
    return {k: torch.from_numpy(v) for k, v in sd.items()}


def small_evaluator(text=True):
    mv, mo, tx = ef.nets(ef.SMALL_POSE)
    return ew.MotionEvaluator(tensors(mv), tensors(mo), tensors(tx) if text else None, dim_pose=ef.SMALL_POSE, device="cpu")


@pytest.mark.parametrize("name", ef.STORED)
def test_restatement_equals_the_reference_motion(gold, name):
    F, motions, lens = ef.motion_case(name)
    parts = {}
    f64 = ef.embed_motions(ef.nets(F), motions, lens, np.float64, parts=parts)
    f32 = ef.embed_motions(ef.nets(F), motions, lens, np.float32)
    assert ef.relmax(f64, gold[f"motion|{name}|f64"]) < 1e-12
    assert gold[f"motion|{name}|f32"].dtype == np.float32 and f32.dtype == np.float32
    assert ef.relmax(f32, gold[f"motion|{name}|f32"]) <= ef.bar(gold[f"dist|motion|{name}"])
    assert ef.relmax(gold[f"motion|{name}|f32"], gold[f"motion|{name}|f64"]) == pytest.approx(float(gold[f"dist|motion|{name}"]), rel=1e-9)
    if name == ef.STORED[0]:
        assert ef.relmax(parts["movement"], gold[f"movement|{name}|f64"]) < 1e-12


@pytest.mark.parametrize("name", ef.STORED_TEXT)
def test_restatement_equals_the_reference_text(gold, name):
    words, pos, lens = ef.text_case(name)
    assert ef.relmax(ef.embed_text(ef.nets(263), words, pos, lens, np.float64), gold[f"text|{name}|f64"]) < 1e-12
    assert ef.relmax(ef.embed_text(ef.nets(263), words, pos, lens, np.float32), gold[f"text|{name}|f32"]) <= ef.bar(gold[f"dist|text|{name}"])


def test_golden_lists_every_case_of_the_fixture(gold):
    want = [f"dist|motion|{n}" for n in ef.MOTION_CASES] + [f"dist|text|{n}" for n in ef.TEXT_CASES] + \
        [f"dist|small|B{b}" for b in ef.SMALL_BATCHES] + ["dist|fid|gen", "dist|fid|real", "stat|dist_matrix|dist", "stat|fid|f32", "stat|fid|f64",
                                                          "stat|ranks", "stat|top3", "stat|top3_sum", "stat|matching", "stat|matching_sum",
                                                          "stat|diversity", "stat|multimodality", "stat|frechet", "seconds|embed32"]
    for k in want:
        assert k in gold.files, k
    for k in gold.files:
        if k.startswith("dist|"):
            assert 0 < float(gold[k]) < 2e-6, (k, float(gold[k]))       # fp32 against f64 at these widths: a few ulp
    assert gold["stat|ranks"].shape == (ef.STAT_N,) and gold["stat|top3"].shape == (ef.STAT_N, 3)
    assert set(gold.files) - set(want) == {f"{kind}|{n}|{p}" for kind, names in (("motion", ef.STORED), ("text", ef.STORED_TEXT))
                                           for n in names for p in ("f32", "f64")} | {f"movement|{ef.STORED[0]}|{p}" for p in ("f32", "f64")}


def test_case_list_covers_the_shapes_that_matter():
    cases = ef.MOTION_CASES.values()
    assert {c[0] for c in cases} == {263, 251}
    assert {c[1] for c in cases} == {1, 2, 17, 33} and {c[0] for c in ef.TEXT_CASES.values()} == {1, 2, 17, 33}
    assert {c[2] for c in cases} == {4, 5, 7, 196, 200}
    assert {c[3] for c in cases} == {"full", "one", "mixed"}
    _, _, lens = ef.motion_case("h263_b33_t196_mixed")
    assert lens.index(max(lens)) != 0 and len(set(lens)) < len(lens)                 # the longest clip is not first; duplicates
    steps = {n // 4 for b in ef.SMALL_BATCHES for n in ef.small_case(b)[2]}
    assert steps == {1, 2, 3, 4, 5}
    assert ef.small_case(34)[2].index(max(ef.small_case(34)[2])) != 0


def test_state_dict_packing():
    mv, mo, tx = ef.nets(ef.SMALL_POSE)
    pm = ew.pack_movement(tensors(mv))
    w = mv["main.0.weight"]                                                         # [out, in, 4] -> [out, tap * in + channel]
    assert pm["conv1_w"].shape == (w.shape[0], 4 * w.shape[1])
    assert np.array_equal(pm["conv1_w"].numpy()[:, 2 * w.shape[1] + 3], w[:, 3, 2])
    assert np.array_equal(pm["conv2_w"].numpy().reshape(64, 4, 64)[5, 1], mv["main.3.weight"][5, :, 1])
    assert np.array_equal(pm["out_w"].numpy(), mv["out_net.weight"])
    for sd, text in ((mo, False), (tx, True)):
        p = ew.pack_recurrent(tensors(sd), "net", text=text)
        H = sd["hidden"].shape[2]
        assert np.array_equal(p["w_ih"].numpy()[:3 * H], sd["gru.weight_ih_l0"]) and np.array_equal(p["w_ih"].numpy()[3 * H:], sd["gru.weight_ih_l0_reverse"])
        assert np.array_equal(p["b_ih"].numpy()[3 * H:], sd["gru.bias_ih_l0_reverse"])
        assert np.array_equal(p["w_hh"].numpy()[0], sd["gru.weight_hh_l0"]) and np.array_equal(p["w_hh"].numpy()[1], sd["gru.weight_hh_l0_reverse"])
        assert np.array_equal(p["b_hh"].numpy()[1], sd["gru.bias_hh_l0_reverse"])
        assert np.array_equal(p["hidden"].numpy(), sd["hidden"][:, 0])
        assert np.array_equal(p["ln_w"].numpy(), sd["output_net.1.weight"]) and np.array_equal(p["o3_b"].numpy(), sd["output_net.3.bias"])
        assert ("pos_w" in p) == text
        assert all(v.dtype == torch.float32 and v.is_contiguous() for v in p.values())
    assert set(ew.MOTION_KEYS) == set(mo) and set(ew.TEXT_KEYS) == set(tx) and set(ew.MOVEMENT_KEYS) == set(mv)
    broken = dict(tensors(mo))
    del broken["gru.weight_hh_l0_reverse"]
    with pytest.raises(KeyError, match="weight_hh_l0_reverse"):
        ew.pack_recurrent(broken, "motion_encoder")
    half = {k: v.double() for k, v in tensors(mo).items()}                          # a float64 checkpoint is uploaded as fp32
    assert ew.pack_recurrent(half, "motion_encoder")["w_hh"].dtype == torch.float32


def test_from_checkpoint_reads_the_finest_tar_layout(tmp_path):
    mv, mo, tx = ef.nets(ef.SMALL_POSE)
    path = os.path.join(tmp_path, "finest.tar")
    torch.save({"movement_encoder": tensors(mv), "text_encoder": tensors(tx), "motion_encoder": tensors(mo), "epoch": 3}, path)
    ev = ew.MotionEvaluator.from_checkpoint(path, dim_pose=ef.SMALL_POSE, device="cpu")
    assert ev.text is not None and ev.motion["w_hh"].shape == (2, 192, 64) and ev.unit_length == 4
    with pytest.raises(ValueError, match="dim_pose"):
        ew.MotionEvaluator.from_checkpoint(path, dim_pose=263, device="cpu")


def test_align_index_is_the_references_expression_with_ties():
    lens = [8, 20, 8, 12, 20, 8]
    want = np.argsort(lens)[::-1].copy()
    for given in (lens, np.array(lens), torch.tensor(lens)):
        assert np.array_equal(ew.align_index(given), want)
    assert [lens[i] for i in want] == sorted(lens, reverse=True)
    assert np.array_equal(ef.align_index(lens), want)


def test_refusals_without_a_gpu():
    ev = small_evaluator()
    F = ef.SMALL_POSE
    x = torch.zeros(3, 20, F)
    with pytest.raises(ValueError, match="unit_length"):
        ev.embed_motions(x, [20, 3, 8])                                  # 3 // 4 == 0: pack_padded_sequence raises there
    with pytest.raises(ValueError, match="movement frames"):
        ev.embed_motions(x, [20, 24, 8])                                 # 6 steps, 20 frames yield 5
    with pytest.raises(ValueError, match="features"):
        ev.embed_motions(torch.zeros(3, 20, F + 1), [20, 8, 8])
    with pytest.raises(ValueError, match="at least 4"):
        ev.embed_motions(torch.zeros(3, 3, F), [3, 3, 3])
    with pytest.raises(ValueError, match="lengths for"):
        ev.embed_motions(x, [20, 8])
    with pytest.raises(ValueError, match="features"):
        ev.embed_samples(torch.zeros(3, F - 1, 1, 20), [20, 8, 8])
    with pytest.raises(ValueError, match=r"\[B, 12, 1, T\]"):
        ev.embed_samples(x, [20, 8, 8])
    with pytest.raises(ValueError, match="come together"):
        ev.embed_samples(torch.zeros(3, F, 1, 20), [20, 8, 8], scale=np.ones(F))
    with pytest.raises(ValueError, match="entries"):
        ev.embed_samples(torch.zeros(3, F, 1, 20), [20, 8, 8], scale=np.ones(F - 4), shift=np.zeros(F - 4))
    with pytest.raises(ValueError, match="unit_length"):
        ev.get_motion_embeddings(x, torch.tensor([20, 0, 8]))
    words, pos = torch.zeros(2, 5, 20), torch.zeros(2, 5, 15)
    with pytest.raises(ValueError, match="caption lengths"):
        ev.embed_text(words, pos, [5, 0])
    with pytest.raises(ValueError, match="caption lengths"):
        ev.embed_text(words, pos, [6, 1])
    with pytest.raises(ValueError, match="word_embs"):
        ev.embed_text(torch.zeros(2, 5, 21), pos, [5, 1])
    bare = small_evaluator(text=False)
    with pytest.raises(ValueError, match="without text weights"):
        bare.embed_text(words, pos, [5, 1])
    with pytest.raises(ValueError, match="without text weights"):
        bare.get_co_embeddings(words, pos, [5, 1], torch.zeros(2, 20, F), [20, 8])
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # valid arguments on the CPU: refused, never computed in torch
        ev.embed_motions(x, [20, 8, 8])
    with pytest.raises(ValueError, match="dim_pose"):
        mv, mo, _ = ef.nets(ef.SMALL_POSE)
        ew.MotionEvaluator(tensors(mv), tensors(mo), dim_pose=263, device="cpu")


def test_native_refusals_without_a_gpu():
    """The library refuses the shapes its kernels cannot take before any launch."""
    from mst_amd import _native
    lib = _native.lib()
    one = 16                                                             # any non-null, 16-byte aligned address: nothing is launched
    assert lib.mst_eval_gru(one, one, one, one, one, 4, 5, 96, 5, one, one, None) != 0
    assert b"multiple of 64" in lib.mst_last_error()
    assert lib.mst_eval_gru(one, one, one, one, one, 4, 5, 64, 6, one, one, None) != 0
    assert b"steps" in lib.mst_last_error()
    assert lib.mst_eval_gemm(one, one, None, None, one, 10, 64, 16, 16, 64, 0, 1, 2, 7, 5, 5, 35, None, None, 0, None) != 0
    assert b"K 16 != 4 * channels 5" in lib.mst_last_error()
    assert lib.mst_eval_gemm(one, one, None, None, one, 10, 64, 20, 20, 64, 0, 2, 2, 7, 5, 5, 35, None, None, 0, None) != 0
    assert b"M 10 != batch 2 * output frames 3" in lib.mst_last_error()
    assert lib.mst_eval_gemm(one, one, None, None, one, 10, 64, 20, 20, 64, 0, 3, 0, 0, 0, 0, 0, None, None, 0, None) != 0
    assert b"mode 3" in lib.mst_last_error()
    assert lib.mst_eval_cov(one, 1, 8, one, one, None) != 0 and b"at least 2" in lib.mst_last_error()
    assert lib.mst_eval_dist_rank(one, one, 4, 4, 8193, one, None, None) != 0 and b"8192" in lib.mst_last_error()
    assert lib.mst_eval_dist_rank(one, one, 4, 5, 8, one, one, None) != 0 and b"square" in lib.mst_last_error()
    assert lib.mst_eval_pair_norms(one, one, one, one, 0, 4, 4, 8, one, None) != 0
    assert lib.mst_eval_layernorm(one, one, None, one, 4, 64, 1e-5, 1, None) != 0


def test_host_frechet_path_against_the_reference(gold):
    a, b = ef.frechet_sets()
    (mu_a, cov_a), (mu_b, cov_b) = ef.statistics(a), ef.statistics(b)
    assert cov_a.dtype == np.float64
    want = float(gold["stat|frechet"])
    got = mt.calculate_frechet_distance(mu_a, cov_a, mu_b, cov_b)
    assert abs(got - want) <= 1e-10 * abs(want), (got, want)
    got_t = mt.calculate_frechet_distance(torch.from_numpy(mu_a), torch.from_numpy(cov_a), torch.from_numpy(mu_b), torch.from_numpy(cov_b))
    assert got_t == got
    assert abs(ef.frechet(mu_a, cov_a, mu_b, cov_b) - want) <= 1e-10 * abs(want)
    with pytest.raises(ValueError, match="means"):
        mt.calculate_frechet_distance(mu_a[:-1], cov_a, mu_b, cov_b)


def test_frechet_singular_and_imaginary_handling(capsys):
    """A singular product is taken again with eps on both diagonals when the root is not finite; a root with a large imaginary diagonal is
    an error; a small imaginary part is dropped."""
    d = 6
    rank1 = np.outer(np.arange(1.0, d + 1), np.arange(1.0, d + 1))
    val = mt.calculate_frechet_distance(np.zeros(d), rank1, np.zeros(d), rank1)
    assert np.isfinite(val) and abs(val) < 1e-3 * np.trace(rank1)               # the same Gaussian twice: 0 up to the root's error
    neg = np.diag([1.0, -4.0])                                                   # sqrt(-4) = 2i on the diagonal
    with pytest.raises(ValueError, match="Imaginary component"):
        mt.calculate_frechet_distance(np.zeros(2), neg, np.zeros(2), np.eye(2))


def test_top_k_and_the_metric_names(gold):
    e1, e2 = ef.stat_embeddings()
    order = np.argsort(ef.euclidean_distance_matrix(e1, e2, np.float64), axis=1)
    assert np.array_equal(mt.calculate_top_k(order, 3), gold["stat|top3"])
    assert np.array_equal(mt.calculate_top_k(torch.from_numpy(order), 3).numpy(), gold["stat|top3"])
    assert np.array_equal(ef.diagonal_ranks(e1, e2, np.float64), gold["stat|ranks"])
    assert np.array_equal(gold["stat|ranks"][:, None] < np.arange(1, 4)[None], gold["stat|top3"])       # top-k is rank < k
    for name in ("euclidean_distance_matrix", "calculate_top_k", "calculate_R_precision", "calculate_matching_score",
                 "calculate_activation_statistics", "calculate_diversity", "calculate_multimodality", "calculate_frechet_distance",
                 "fid_from_embeddings"):
        assert callable(getattr(mt, name))
