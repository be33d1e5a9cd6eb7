"""The T2M evaluators and their statistics on the GPU (data_loaders/evaluator_wrapper.py, utils/metrics.py, csrc/mst_eval.h) against the
float64 restatement (tests/eval_fixture.py).  Nothing here reads the reference: bars come from tests/golden/eval.npz.

The embedding bar: max error over the largest magnitude of the float64 result at most 4 x the reference's own float32-to-float64
distance for that case, floor 1e-6 (eval_fixture.bar).  Every case prints `eval: <case> ref <dist> got <dist> bar <bar>`.

Exact, bit for bit: a clip against the same clip alone, elsewhere in the batch and beside other clips; frames past 4 steps + 2 changed;
the samplers' layout against rows; `get_motion_embeddings` against `embed_motions[align_idx]`; a side stream against the default one;
ranks and R-precision against the reference's recorded result.

Measured on an MI355X (reference fp32 / kernels / bar): motion embeddings at the real widths 3.2e-7 .. 7.7e-7 / 7.2e-7 .. 1.1e-6 /
1.3e-6 .. 3.1e-6, the closest approach 0.56 of the bar (2 clips x 5 frames); text 3.6e-7 .. 6.5e-7 / 5.5e-7 .. 7.3e-7 / 1.4e-6 .. 2.6e-6;
H = 64 at most 3.4e-7 against bars from 1.0e-6; the affine path 7.8e-7 against host-renormalised rows, 1.0e-6 against float64, bar
2.2e-6; distance matrix 1.1e-7 / 8.1e-8 / 1.0e-6; covariance at most 3.2e-14 against a bound of 8.6e-11; matching score and diversity
equal to the recorded values, multimodality within 6.6e-8; FID 1.1e-7 relative against 4.0e-6.  The file takes 4 s."""
import os

import numpy as np
import pytest
import torch

import eval_fixture as ef
import mst_amd  # noqa: F401
from conftest import GOLDEN
from mst_amd.data_loaders import evaluator_wrapper as ew
from mst_amd.utils import metrics as mt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "eval.npz"))


def dev():
    return torch.device("cuda")


def cu(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=dev(), dtype=dtype)


def host(t):
    return t.detach().cpu().numpy()


_evaluators = {}


def evaluator(dim_pose):
    if dim_pose not in _evaluators:
        mv, mo, tx = ef.nets(dim_pose)
        t = lambda sd: {k: torch.from_numpy(v) for k, v in sd.items()}
        _evaluators[dim_pose] = ew.MotionEvaluator(t(mv), t(mo), t(tx), dim_pose=dim_pose, device=dev())
    return _evaluators[dim_pose]


def held(tag, got, f64, distance):
    d, b = ef.relmax(got, f64), ef.bar(distance)
    print(f"eval: {tag} ref {float(distance):.3e} got {d:.3e} bar {b:.3e}")
    assert np.isfinite(got).all()
    assert d <= b, (tag, d, b)


# ------------------------------------------------------------------------------------------ embeddings at the real widths
@pytest.mark.parametrize("name", list(ef.MOTION_CASES))
def test_motion_embeddings(gold, name):
    F, motions, lens = ef.motion_case(name)
    ev = evaluator(F)
    got = host(ev.embed_motions(cu(motions), lens))
    assert got.shape == (len(lens), 512) and got.dtype == np.float32
    held("motion " + name, got, ef.embed_motions(ef.nets(F), motions, lens, np.float64), gold[f"dist|motion|{name}"])
    if name in ef.STORED:                                                # the reference's own float32 rows are as near
        assert ef.relmax(got, gold[f"motion|{name}|f32"]) <= 2 * ef.bar(gold[f"dist|motion|{name}"])
    aligned = host(ev.get_motion_embeddings(cu(motions), torch.tensor(lens)))
    assert np.array_equal(aligned, got[ef.align_index(lens)])


@pytest.mark.parametrize("name", list(ef.TEXT_CASES))
def test_text_embeddings(gold, name):
    words, pos, lens = ef.text_case(name)
    ev = evaluator(263)
    got = host(ev.embed_text(cu(words), cu(pos), lens))
    held("text " + name, got, ef.embed_text(ef.nets(263), words, pos, lens, np.float64), gold[f"dist|text|{name}"])
    B = len(lens)
    motions = ef.syn.normal(ef.SEED, "eval/co/" + name, (B, 8, 263))
    m_lens = [4 + (3 * b) % 5 for b in range(B)]                         # tied lengths
    text, motion = ev.get_co_embeddings(cu(words), cu(pos), lens, cu(motions), torch.tensor(m_lens))
    idx = ef.align_index(m_lens)
    assert np.array_equal(host(text), got[idx])
    assert np.array_equal(host(motion), host(ev.embed_motions(cu(motions), m_lens))[idx])


def test_small_width_sweep(gold):
    """H = 64: every batch size 1 .. 34 (one, two and three clip tiles, full and ragged), step counts 1 .. 5 mixed in every batch."""
    ev = evaluator(ef.SMALL_POSE)
    net = ef.nets(ef.SMALL_POSE)
    for B in ef.SMALL_BATCHES:
        F, motions, lens = ef.small_case(B)
        got = host(ev.embed_motions(cu(motions), lens))
        held(f"small B{B}", got, ef.embed_motions(net, motions, lens, np.float64), gold[f"dist|small|B{B}"])


# ------------------------------------------------------------------------------------------ invariants, bit for bit
def invariant_case():
    B, T, F = 19, 24, 263
    motions = ef.syn.normal(ef.SEED, "eval/invariant", (B, T, F))
    lens = [4 * (1 + (b + 3) % 6) + b % 3 for b in range(B)]
    lens = [min(n, T) for n in lens]
    return motions, lens


def test_a_clip_does_not_depend_on_its_batch():
    ev = evaluator(263)
    motions, lens = invariant_case()
    base = host(ev.embed_motions(cu(motions), lens))
    for b in (0, 7, 18):                                                 # alone
        assert np.array_equal(host(ev.embed_motions(cu(motions[b:b + 1]), lens[b:b + 1]))[0], base[b])
    perm = np.roll(np.arange(len(lens)), 5)                              # elsewhere: clips cross the 16-clip tile
    moved = host(ev.embed_motions(cu(motions[perm]), [lens[i] for i in perm]))
    assert np.array_equal(moved, base[perm])
    other = motions.copy()                                               # beside other clips
    other[1:] = ef.syn.normal(ef.SEED, "eval/invariant/other", other[1:].shape)
    other_lens = [lens[0]] + [8] * (len(lens) - 1)
    assert np.array_equal(host(ev.embed_motions(cu(other), other_lens))[0], base[0])


def test_frames_past_a_clips_length_are_not_read():
    """Movement frame s reads input frames 4 s - 3 .. 4 s + 6: with `steps` movement frames, frames from 4 steps + 3 on are free."""
    ev = evaluator(263)
    motions, lens = invariant_case()
    base = host(ev.embed_motions(cu(motions), lens))
    changed = motions.copy()
    for b, n in enumerate(lens):
        changed[b, 4 * (n // 4) + 3:] = 7.0
    assert any(4 * (n // 4) + 3 < motions.shape[1] for n in lens)
    assert np.array_equal(host(ev.embed_motions(cu(changed), lens)), base)
    changed[0, 4 * (lens[0] // 4) + 2] += 1.0                            # the last frame that IS read
    assert not np.array_equal(host(ev.embed_motions(cu(changed), lens))[0], base[0])


def test_samples_layout_and_affine(gold):
    name = "h263_b2_t196_full"
    F, motions, lens = ef.motion_case(name)
    ev = evaluator(F)
    rows = host(ev.embed_motions(cu(motions), lens))
    sample = np.ascontiguousarray(motions.transpose(0, 2, 1)[:, :, None, :])
    assert np.array_equal(host(ev.embed_samples(cu(sample), lens)), rows)          # the same numbers read in the same order
    scale = (0.5 + ef.syn.uniform01(ef.SEED, "eval/affine/scale", F)).astype(np.float32)
    shift = ef.syn.normal(ef.SEED, "eval/affine/shift", (F,))
    raw = ((sample - shift[None, :, None, None]) / scale[None, :, None, None]).astype(np.float32)
    renorm = (raw * scale[None, :, None, None] + shift[None, :, None, None]).astype(np.float32)       # the host's renormalisation
    renorm_rows = np.ascontiguousarray(renorm[:, :, 0].transpose(0, 2, 1))
    got = host(ev.embed_samples(cu(raw), lens, scale=scale, shift=shift))
    held("affine against rows", got, host(ev.embed_motions(cu(renorm_rows), lens)), gold[f"dist|motion|{name}"])
    held("affine against f64", got, ef.embed_motions(ef.nets(F), renorm_rows, lens, np.float64), gold[f"dist|motion|{name}"])
    assert np.array_equal(host(ev.embed_samples(cu(raw), lens, scale=cu(scale), shift=cu(shift))), got)


def test_side_stream_gives_the_same_bits():
    ev = evaluator(263)
    motions, lens = invariant_case()
    words, pos, caps = ef.text_case("b17_l20_one")
    e1, e2 = ef.stat_embeddings()
    x, w, p = cu(motions), cu(words), cu(pos)
    a, b = cu(e1), cu(e2)
    base = (ev.embed_motions(x, lens), ev.embed_text(w, p, caps), mt.calculate_R_precision(a, b, 3), mt.calculate_activation_statistics(a)[1])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = (ev.embed_motions(x, lens), ev.embed_text(w, p, caps), mt.calculate_R_precision(a, b, 3), mt.calculate_activation_statistics(a)[1])
    side.synchronize()
    for u, v in zip(base, again):
        assert torch.equal(u, v)


# ------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("D", [1, 20, 512])
@pytest.mark.parametrize("n", [2, 63, 64, 65, 1000])
def test_covariance_against_numpy(n, D):
    """np.cov on the same fp32 rows.  Element-wise within 2 N 2^-52 max|x - mu|^2, the bound of an N-term double sum; the mean within
    2^-24 |mu| of the float64 mean (columns are offset from zero so that |mu| is no rounding artefact)."""
    rows = (ef.syn.normal(ef.SEED, f"eval/cov/{n}/{D}", (n, D)) * 3.0 + (1.0 + np.arange(D, dtype=np.float32) % 7)).astype(np.float32)
    mu, cov = mt.calculate_activation_statistics(cu(rows))
    assert mu.dtype == torch.float64 and cov.dtype == torch.float64 and cov.shape == (D, D)
    mu64 = rows.astype(np.float64).mean(0)
    want = np.cov(rows, rowvar=False).reshape(D, D)
    assert want.dtype == np.float64
    assert (np.abs(host(mu) - mu64) <= 2.0 ** -24 * np.abs(mu64)).all()
    bound = 2 * n * 2.0 ** -52 * np.abs(rows.astype(np.float64) - mu64).max() ** 2
    err = np.abs(host(cov) - want).max()
    print(f"eval: cov N {n} D {D} err {err:.3e} bound {bound:.3e}")
    assert err <= bound
    mu_np, cov_np = mt.calculate_activation_statistics(rows)            # numpy in, numpy out
    assert isinstance(cov_np, np.ndarray) and np.array_equal(cov_np, host(cov)) and np.array_equal(mu_np, host(mu))


def test_distance_matrix_ranks_and_r_precision(gold):
    e1, e2 = ef.stat_embeddings()                                        # asserts the rank margin in float64
    dist = mt.euclidean_distance_matrix(cu(e1), cu(e2))
    assert dist.dtype == torch.float32
    held("distance matrix", host(dist), ef.euclidean_distance_matrix(e1, e2, np.float64), gold["stat|dist_matrix|dist"])
    assert np.array_equal(host(mt.diagonal_ranks(cu(e1), cu(e2))), gold["stat|ranks"])
    top3 = mt.calculate_R_precision(cu(e1), cu(e2), 3)
    assert np.array_equal(host(top3), gold["stat|top3"])
    assert np.array_equal(mt.calculate_R_precision(e1, e2, 3, sum_all=True), gold["stat|top3_sum"])
    assert np.array_equal(host(mt.calculate_R_precision(cu(e1), cu(e2), 1))[:, 0], gold["stat|ranks"] == 0)
    rect = mt.euclidean_distance_matrix(e1[:5], e2)                      # a rectangle, numpy in and out
    assert rect.shape == (5, ef.STAT_N) and np.array_equal(rect, host(dist)[:5])
    same = host(mt.euclidean_distance_matrix(cu(e1), cu(e1)))            # a radicand that rounds below zero is 0, never NaN
    assert np.isfinite(same).all() and (same >= 0).all()


def test_pair_statistics_under_a_seed(gold):
    e1, e2 = ef.stat_embeddings()
    rel = lambda got, want: abs(float(got) - float(want)) / abs(float(want))
    match = mt.calculate_matching_score(cu(e1), cu(e2))
    assert ef.relmax(host(match), gold["stat|matching"]) <= 1e-6
    assert rel(mt.calculate_matching_score(e1, e2, sum_all=True), gold["stat|matching_sum"]) <= 1e-6
    np.random.seed(ef.NP_SEED)
    div = mt.calculate_diversity(cu(e1), ef.DIVERSITY_TIMES)
    np.random.seed(ef.NP_SEED)
    mm = mt.calculate_multimodality(cu(ef.multimodal_embeddings()), ef.MM_TIMES)
    print(f"eval: matching {rel(host(match).sum(), gold['stat|matching_sum']):.3e} diversity {rel(div, gold['stat|diversity']):.3e} "
          f"multimodality {rel(mm, gold['stat|multimodality']):.3e}")
    assert rel(div, gold["stat|diversity"]) <= 1e-6
    assert rel(mm, gold["stat|multimodality"]) <= 1e-6
    with pytest.raises(AssertionError):
        mt.calculate_diversity(cu(e1), ef.STAT_N)


def test_fid_end_to_end(gold):
    """Two sets of clips embedded on the GPU, then the FID of the embeddings, against the reference's FID from its float64 embeddings.
    The bar: 4 x the distance between the reference's FID from float32 and from float64 embeddings, floor 1e-6, relative."""
    ev = evaluator(ef.SMALL_POSE)
    gen, real, lens = ef.fid_sets()
    eg, er = ev.embed_motions(cu(gen), lens), ev.embed_motions(cu(real), lens)
    net = ef.nets(ef.SMALL_POSE)
    held("fid gen", host(eg), ef.embed_motions(net, gen, lens, np.float64), gold["dist|fid|gen"])
    held("fid real", host(er), ef.embed_motions(net, real, lens, np.float64), gold["dist|fid|real"])
    f32, f64 = float(gold["stat|fid|f32"]), float(gold["stat|fid|f64"])
    bar = max(4 * abs(f32 - f64) / abs(f64), 1e-6)
    got = mt.fid_from_embeddings(eg, er)
    print(f"eval: fid reference {f64:.9f} (from fp32 {f32:.9f}) got {got:.9f} distance {abs(got - f64) / f64:.3e} bar {bar:.3e}")
    assert abs(got - f64) / abs(f64) <= bar
