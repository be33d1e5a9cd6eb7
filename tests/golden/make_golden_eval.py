"""Golden vectors of the T2M evaluators and their statistics: the reference's `MovementConvEncoder`, `MotionEncoderBiGRUCo` and
`TextEncoderBiGRUCo` (data_loaders/humanml/networks/modules.py) chained as `EvaluatorMDMWrapper` chains them
(networks/evaluator_wrapper.py:154-187), and data_loaders/humanml/utils/metrics.py, run on the seeded weights and cases of
tests/eval_fixture.py.  Run in the authoring container only (imports the reference checkout that make_golden.py puts on the path):
    python tests/golden/make_golden_eval.py -> eval.npz

Stored: what the reference produced, nothing else (weights and inputs are rebuilt from the seed).
  `motion|<case>|f32` / `|f64`   the reference's embeddings in INPUT order, for the cases of eval_fixture.STORED
  `movement|<case>|f32` / `|f64` its movement features for STORED[0]
  `text|<case>|f32` / `|f64`     the text embeddings for STORED_TEXT
  `dist|motion|<case>`, `dist|text|<case>`, `dist|small|B<n>`, `dist|fid|gen` / `real`
                                 for EVERY case the GPU test runs: the reference's float32 result against its float64 one, max error
                                 over the largest magnitude -- the yardstick of tests/test_gpu_evaluator.py
  `stat|...`                     on eval_fixture.stat_embeddings() / multimodal_embeddings(): `dist_matrix|dist` (fp32 against f64),
                                 `ranks` (position of i in the argsort of row i), `top3`, `top3_sum`, `matching`, `matching_sum`,
                                 `diversity` and `multimodality` under np.random.seed(NP_SEED), each from float32 inputs;
                                 `frechet`: calculate_frechet_distance on the float64 statistics of two seeded activation sets;
                                 `fid|f32` / `fid|f64`: the FID of eval_fixture.fid_sets() from the reference's float32 and float64
                                 embeddings
  `seconds|embed32`              the reference's wall time for get_motion_embeddings on 32 clips of 196 x 263 on this CPU

The reference packs sequences in the order it is given and needs descending lengths: motions are sorted by `align_idx` as its wrapper
does, captions by a stable descending sort, and both are put back in input order before they are stored.

Asserted before anything is written, every distance printed: the fixture's float64 equals the reference's float64 to 1e-12; the
fixture's float32 is within the bar of the reference's float32; the reference's float32 ranks equal its float64 ones on the
rank-margin inputs; the file is smaller than 500 KiB."""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402

mg.install_shims()
import eval_fixture as ef  # noqa: E402
from data_loaders.humanml.networks import modules as M  # noqa: E402
from data_loaders.humanml.utils import metrics as RM  # noqa: E402

DT = {np.float32: torch.float32, np.float64: torch.float64}


def reference_nets(dim_pose, dtype):
    s = ef.SMALL if dim_pose == ef.SMALL_POSE else ef.REAL
    mv_sd, mo_sd, tx_sd = ef.nets(dim_pose)
    mv = M.MovementConvEncoder(dim_pose - 4, s["hid"], s["lat"])
    mo = M.MotionEncoderBiGRUCo(s["lat"], s["Hm"], s["out"], "cpu")
    tx = M.TextEncoderBiGRUCo(s["word"], s["pos"], s["Ht"], s["out"], "cpu")
    for mod, sd in ((mv, mv_sd), (mo, mo_sd), (tx, tx_sd)):
        mod.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        mod.eval()
        mod.to(DT[dtype])
    return mv, mo, tx


_nets = {}


def refs(dim_pose, dtype):
    key = (dim_pose, dtype)
    if key not in _nets:
        _nets[key] = reference_nets(dim_pose, dtype)
    return _nets[key]


def ref_motion(dim_pose, motions, m_lens, dtype):
    """-> (embeddings, movement features), input order."""
    mv, mo, _ = refs(dim_pose, dtype)
    with torch.no_grad():
        x = torch.from_numpy(np.asarray(motions)).to(DT[dtype])
        lens = torch.tensor(list(m_lens))
        align = np.argsort(lens.data.tolist())[::-1].copy()
        movements = mv(x[align][..., :-4]).detach()
        emb = mo(movements, lens[align] // 4).numpy()
    out, feats = np.empty_like(emb), np.empty_like(movements.numpy())
    out[align], feats[align] = emb, movements.numpy()
    return out, feats


def ref_text(words, pos, cap_lens, dtype, dim_pose=263):
    tx = refs(dim_pose, dtype)[2]
    order = np.argsort(-np.asarray(cap_lens), kind="stable")
    with torch.no_grad():
        emb = tx(torch.from_numpy(words[order]).to(DT[dtype]), torch.from_numpy(pos[order]).to(DT[dtype]),
                 torch.tensor(np.asarray(cap_lens)[order])).numpy()
    out = np.empty_like(emb)
    out[order] = emb
    return out


def both(tag, ref32, ref64, fix32, fix64):
    """Check the fixture against the reference; -> the reference's own fp32-to-f64 distance."""
    d = ef.relmax(ref32, ref64)
    exact = ef.relmax(fix64, ref64)
    f32 = ef.relmax(fix32, ref32)
    print(f"{tag}: ref32~ref64 {d:.3e}  fixture64~ref64 {exact:.3e}  fixture32~ref32 {f32:.3e}")
    assert exact < 1e-12, (tag, exact)
    assert f32 <= ef.bar(d), (tag, f32, d)
    return np.float64(d)


def main():
    out = {}
    for name in ef.MOTION_CASES:
        F, motions, lens = ef.motion_case(name)
        r32, m32 = ref_motion(F, motions, lens, np.float32)
        r64, m64 = ref_motion(F, motions, lens, np.float64)
        p32, p64 = {}, {}
        f32 = ef.embed_motions(ef.nets(F), motions, lens, np.float32, parts=p32)
        f64 = ef.embed_motions(ef.nets(F), motions, lens, np.float64, parts=p64)
        out[f"dist|motion|{name}"] = both("motion " + name, r32, r64, f32, f64)
        if name in ef.STORED:
            out[f"motion|{name}|f32"], out[f"motion|{name}|f64"] = r32, r64
        if name == ef.STORED[0]:
            both("movement " + name, m32, m64, p32["movement"], p64["movement"])
            out[f"movement|{name}|f32"], out[f"movement|{name}|f64"] = m32, m64
    for name in ef.TEXT_CASES:
        words, pos, lens = ef.text_case(name)
        r32, r64 = ref_text(words, pos, lens, np.float32), ref_text(words, pos, lens, np.float64)
        f32 = ef.embed_text(ef.nets(263), words, pos, lens, np.float32)
        f64 = ef.embed_text(ef.nets(263), words, pos, lens, np.float64)
        out[f"dist|text|{name}"] = both("text " + name, r32, r64, f32, f64)
        if name in ef.STORED_TEXT:
            out[f"text|{name}|f32"], out[f"text|{name}|f64"] = r32, r64
    small = ef.nets(ef.SMALL_POSE)
    for B in ef.SMALL_BATCHES:
        F, motions, lens = ef.small_case(B)
        r32, r64 = ref_motion(F, motions, lens, np.float32)[0], ref_motion(F, motions, lens, np.float64)[0]
        out[f"dist|small|B{B}"] = both(f"small B{B}", r32, r64, ef.embed_motions(small, motions, lens, np.float32),
                                       ef.embed_motions(small, motions, lens, np.float64))

    # ---- the end-to-end FID case
    gen, real, lens = ef.fid_sets()
    e = {}
    for tag, clips in (("gen", gen), ("real", real)):
        for dt in (np.float32, np.float64):
            e[tag, dt] = ref_motion(ef.SMALL_POSE, clips, lens, dt)[0]
        out[f"dist|fid|{tag}"] = both("fid " + tag, e[tag, np.float32], e[tag, np.float64], ef.embed_motions(small, clips, lens, np.float32),
                                      ef.embed_motions(small, clips, lens, np.float64))
    for dt, key in ((np.float32, "f32"), (np.float64, "f64")):
        mu_g, cov_g = RM.calculate_activation_statistics(e["gen", dt])
        mu_r, cov_r = RM.calculate_activation_statistics(e["real", dt])
        out[f"stat|fid|{key}"] = np.float64(RM.calculate_frechet_distance(mu_g, cov_g, mu_r, cov_r))
        assert abs(ef.fid(e["gen", dt], e["real", dt]) - out[f"stat|fid|{key}"]) <= 1e-10 * abs(out[f"stat|fid|{key}"])
    print("fid f32 / f64:", out["stat|fid|f32"], out["stat|fid|f64"])

    # ---- the statistics on seeded embeddings
    e1, e2 = ef.stat_embeddings()
    d32 = RM.euclidean_distance_matrix(e1, e2)
    d64 = RM.euclidean_distance_matrix(e1.astype(np.float64), e2.astype(np.float64))
    assert d32.dtype == np.float32
    out["stat|dist_matrix|dist"] = both("distance matrix", d32, d64, ef.euclidean_distance_matrix(e1, e2, np.float32),
                                        ef.euclidean_distance_matrix(e1, e2, np.float64))
    order32, order64 = np.argsort(d32, axis=1), np.argsort(d64, axis=1)
    ranks = np.array([int(np.nonzero(order32[i] == i)[0][0]) for i in range(len(order32))], np.int32)
    assert np.array_equal(order32, order64) or np.array_equal(ranks, [int(np.nonzero(order64[i] == i)[0][0]) for i in range(len(ranks))])
    assert np.array_equal(ranks, ef.diagonal_ranks(e1, e2, np.float64))
    top3 = RM.calculate_R_precision(e1, e2, 3)
    assert np.array_equal(top3, ef.r_precision(e1, e2, 3, np.float64)) and np.array_equal(top3, RM.calculate_top_k(order32, 3))
    out["stat|ranks"], out["stat|top3"] = ranks, top3
    out["stat|top3_sum"] = RM.calculate_R_precision(e1, e2, 3, sum_all=True)
    print("ranks", ranks.tolist(), "top-k sums", out["stat|top3_sum"].tolist())
    assert 0 < out["stat|top3_sum"][0] < out["stat|top3_sum"][1] < out["stat|top3_sum"][2]
    out["stat|matching"] = RM.calculate_matching_score(e1, e2)
    out["stat|matching_sum"] = np.float64(RM.calculate_matching_score(e1, e2, sum_all=True))
    np.random.seed(ef.NP_SEED)
    out["stat|diversity"] = np.float64(RM.calculate_diversity(e1, ef.DIVERSITY_TIMES))
    np.random.seed(ef.NP_SEED)
    assert ef.diversity(e1, ef.DIVERSITY_TIMES, np.float32) == out["stat|diversity"]
    mm = ef.multimodal_embeddings()
    np.random.seed(ef.NP_SEED)
    out["stat|multimodality"] = np.float64(RM.calculate_multimodality(mm, ef.MM_TIMES))
    np.random.seed(ef.NP_SEED)
    assert ef.multimodality(mm, ef.MM_TIMES, np.float32) == out["stat|multimodality"]
    a, b = ef.frechet_sets()
    sa, sb = RM.calculate_activation_statistics(a), RM.calculate_activation_statistics(b)
    out["stat|frechet"] = np.float64(RM.calculate_frechet_distance(sa[0], sa[1], sb[0], sb[1]))
    assert abs(ef.frechet(*sa, *sb) - out["stat|frechet"]) <= 1e-10 * out["stat|frechet"]
    print("frechet", out["stat|frechet"], "diversity", out["stat|diversity"], "multimodality", out["stat|multimodality"])

    # ---- the reference's time for 32 full-length clips
    clips = torch.from_numpy(ef.syn.normal(ef.SEED, "eval/timing", (32, 196, 263)))
    lens = torch.tensor([196 - 4 * (b % 8) for b in range(32)])
    mv, mo, _ = refs(263, np.float32)
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        with torch.no_grad():
            align = np.argsort(lens.data.tolist())[::-1].copy()
            mo(mv(clips[align][..., :-4]).detach(), lens[align] // 4)
        best = min(best, time.perf_counter() - t0)
    out["seconds|embed32"] = np.float64(best)
    print(f"reference, 32 clips of 196 x 263 on {torch.get_num_threads()} CPU threads: {best:.3f} s")

    path = os.path.join(HERE, "eval.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"wrote {path}: {len(out)} arrays, {size} bytes")
    assert size < 500 * 1024


if __name__ == "__main__":
    main()
