"""Proof without a GPU that the per-stage checks of tests/test_gpu_clip_stages.py can fail (tests/clip_stage_fixture.py):

  1. the fixture's float64 stage statements, chained without f16 rounding, are the tower: cf.forward64 to 1e-12;
  2. every fp32 restatement, rounded where its stage rounds, passes its own stage's bar -- and so does the host's operand dict;
  3. every mutant -- a float64 stage output with one thing wrong, rounded the way the stage rounds -- fails the bar of its stage on row
     set A; the eps mutant on small-2, whose LayerNorm input rows all have a variance within a factor 10 of eps;
  4. the row sets and the towers are what the GPU test relies on."""
import numpy as np
import pytest

import clip_stage_fixture as sf
import clip_text_fixture as cf


@pytest.fixture(scope="module")
def W():
    return sf.stage_weights()


@pytest.fixture(scope="module")
def A(W):
    return sf.host_operands("A", W)


@pytest.fixture(scope="module")
def small():
    w = sf.site_weights()
    return sf.host_sites(w), w


def chained(sd, ids, lens, layers):
    w = [sf.weights(sd, i) for i in range(layers)]
    x = sf.embed(ids, lens, w[0]["tok"], w[0]["pos"], np.float64)
    for i in range(layers):
        x, _ = sf.layer(x, w[i], lens, np.float64, lambda a: a)
    return sf.final(x, lens, w[0]["lnf_g"], w[0]["lnf_b"], w[0]["proj"], np.float64)


def test_chained_statements_are_the_tower():
    sd = cf.state_dict(2)
    ids = cf.case_ids("l2")
    lens = [e + 1 for e in cf.CASES["l2"][2]]
    d = cf.distance(chained(sd, ids, lens, 2), cf.forward64(sd, ids))
    ids, lens = sf.rowset_ids("A")
    e = cf.distance(chained(sd, ids, lens, 2), cf.forward64(sd, ids))
    print(f"clip_stage chain: l2 {d.max():.2e} A {e.max():.2e}")
    assert d.max() <= 1e-12 and e.max() <= 1e-12


def test_row_sets_cover_what_they_claim():
    assert sum(sf.ROWSETS["A"]) == 350 and 350 % 32 == 30
    assert {n % 4 for n in sf.ROWSETS["A"]} == {0, 1, 2, 3} and min(sf.ROWSETS["A"]) == 1 and max(sf.ROWSETS["A"]) == 77
    assert {63, 64, 65, 66} <= set(sf.ROWSETS["A"])                                # keys 63 | 64: the lane + 64 half begins at row 64
    b = [sum(sf.ROWSETS[k]) for k in sf.STAGE_SETS[1:]]
    assert {m % 32 for m in b} == {0, 1, 16, 17} and 1 in b and 33 in b
    assert all(len(sf.ROWSETS[k]) <= 3 for k in sf.STAGE_SETS[1:])
    for name in sf.ROWSETS:
        ids, lens = sf.rowset_ids(name)
        assert (ids.argmax(1) + 1 == np.asarray(lens)).all() and ids.max() == cf.EOT and ids.min() >= 0
        assert sum(lens) <= len(lens) * ids.shape[1]                               # the ABI's bound on packed rows


def test_tower_edits_are_f16_and_do_what_the_combination_needs():
    real, mid, emb, nxt, small = (sf.tower_sd(n) for n in ("real-1", "mid-1", "emb-1", "next-2", "small-2"))
    for sd in (real, mid, emb, nxt, small):
        for k, v in sd.items():
            assert np.array_equal(cf._f16(v), v), k
    p = "transformer.resblocks.0."
    changed = lambda a, b: sorted(k for k in a if not np.array_equal(a[k], b[k]))
    assert changed(real, mid) == [p + "mlp.c_proj.bias", p + "mlp.c_proj.weight"] and not mid[p + "mlp.c_proj.weight"].any()
    assert len(changed(real, emb)) == 6 and np.array_equal(emb[p + "attn.in_proj_weight"][:512], np.eye(512))
    assert np.array_equal(emb[p + "attn.in_proj_weight"][512:], real[p + "attn.in_proj_weight"][512:])
    assert not emb[p + "attn.in_proj_bias"][:512].any() and not emb[p + "attn.out_proj.bias"].any()
    assert all(np.array_equal(real[k], nxt[k]) for k in real)                      # next-2's layer 0 and ends are real-1's
    assert np.array_equal(nxt["transformer.resblocks.1.attn.in_proj_weight"][:512], np.eye(512))
    assert not nxt["transformer.resblocks.1.mlp.c_proj.bias"].any() and not small[p + "attn.out_proj.bias"].any()
    assert np.array_equal(small[p + "attn.in_proj_weight"][:512], np.eye(512))


def test_small_tower_puts_every_layernorm_row_within_ten_of_eps(small):
    S, w = small
    assert np.array_equal(S["x"].astype(np.float64), sf.embed(S["ids"], S["lens"], w["tok"], w["pos"], np.float64))
    v = S["x"].astype(np.float64).var(-1)                                         # the stream at all four sites is the embedding
    print(f"clip_stage small-2: shift {sf.small_shift()} variance {v.min():.3e} .. {v.max():.3e} (eps {sf.EPS:g})")
    assert v.shape == (350,) and sf.EPS / 10 <= v.min() and v.max() <= 10 * sf.EPS


@pytest.mark.parametrize("stage", sf.STAGES[1:])
def test_fp32_restatement_and_host_operands_pass_the_bar(stage, A, W):
    own, d32 = sf.judge(stage, A, W)
    rest, _ = sf.judge(stage, A, W, got=sf.stored(stage, sf.statement(stage, A, W, np.float32)))
    print(f"clip_stage: host {stage} rows A worst {own:.3f} restatement {rest:.3f} d32 {d32:.3e}")
    assert own <= 1.0 and rest <= 1.0 and 0.0 < d32 < 1e-5


@pytest.mark.parametrize("site", list(sf.SITES))
def test_fp32_restatement_passes_the_bar_at_small_variance(site, small):
    S, w = small
    own, d32 = sf.judge_site(site, S, w)
    out = sf.site_statement(site, S, w, np.float32)
    rest, _ = sf.judge_site(site, S, w, got=sf.f16(out) if sf.SITES[site][1] else out)
    print(f"clip_stage: host small-2 {site} rows A worst {own:.3f} restatement {rest:.3f} d32 {d32:.3e}")
    assert own <= 1.0 and rest <= 1.0 and 0.0 < d32 < 1e-5


@pytest.mark.parametrize("name", list(sf.MUTANTS))
def test_mutant_fails_its_stage(name, A, W):
    stage, wrong = sf.MUTANTS[name]
    got, d32 = sf.judge(stage, A, W, got=sf.stored(stage, wrong(A, W)))
    print(f"clip_stage mutant: {name}: {got:.2f} of the bar of {stage} (d32 {d32:.3e})")
    assert got > 1.0


@pytest.mark.parametrize("site", list(sf.SITES))
def test_eps_mutant_fails_at_every_site_of_the_small_tower(site, small):
    S, w = small
    wrong = sf.site_statement(site, S, w, np.float64, eps=1e-6)
    got, _ = sf.judge_site(site, S, w, got=sf.f16(wrong) if sf.SITES[site][1] else wrong.astype(np.float32))
    print(f"clip_stage mutant: eps 1e-6 at {site}: {got:.1f} of the bar on small-2")
    assert got > 1.0


def test_shifted_position_table_is_not_the_embedding(A, W):
    wrong = sf.embed(A["ids"], A["lens"], W["tok"], W["pos"], np.float32, shift=1)
    assert A["x_emb"].dtype == np.float32 and wrong.shape == A["x_emb"].shape
    assert np.array_equal(A["x_emb"].view(np.uint32), sf.embed(A["ids"], A["lens"], W["tok"], W["pos"], np.float32).view(np.uint32))
    assert (A["x_emb"].view(np.uint32) != wrong.view(np.uint32)).any(axis=1).all()   # every row differs


def test_half_ulp_is_f16s():
    for v in (1.0, 1.9990234375, 2.0, 0.33, 1000.0, 6.103515625e-05, 3e-6, 0.0):
        h = np.float16(v)
        want = 0.5 * float(np.spacing(np.abs(h)))
        assert float(sf.half_ulp16(np.float64(h))) == want, v
    assert float(sf.half_ulp16(np.float64(1.99999))) == 2.0 ** -11                # the binade of the reference, not of its rounding
