"""tests/token_profile.py on the CPU: known answers, the dilution the pooled relative L2 suffers and the profiles do not, the rounding
model inside its own bars on every case of tests/test_gpu_token_profile.py, and a wrong oracle input that only the profiles catch."""
import numpy as np
import pytest
import torch

import token_cases as tc
import token_profile as tp
from conftest import rel_l2
from token_profile import C_ROW, C_ROW_CAP, C_TOK, C_TOK_CAP


def test_known_answers_on_a_tiny_tensor():
    # two clips, two features, two frames; ref[b, f, 0, t]
    ref = np.array([[[[3.0, 0.0]], [[4.0, 5.0]]], [[[1.0, 1.0]], [[1.0, 1.0]]]])
    out = ref.copy()
    out[0, 0, 0, 0] += 0.3          # clip 0, frame 0: (0.3, 0.4)
    out[0, 1, 0, 0] += 0.4
    out[1, 1, 0, 1] -= 0.2          # clip 1, frame 1: (0, -0.2)
    # clip 0: token norms 5 and 5 -> RMS 5; clip 1: token norms sqrt 2 -> RMS sqrt 2
    np.testing.assert_allclose(tp.token_errors(out, ref), [[0.5 / 5, 0.0], [0.0, 0.2 / np.sqrt(2)]], rtol=1e-12)
    # row 0: ref (3, 0, 1, 1) -> sqrt 11, difference 0.3; row 1: ref (4, 5, 1, 1) -> sqrt 43, difference sqrt(0.16 + 0.04)
    np.testing.assert_allclose(tp.row_errors(out, ref), [0.3 / np.sqrt(11), np.sqrt(0.2) / np.sqrt(43)], rtol=1e-12)
    np.testing.assert_allclose(tp.clip_errors(out, ref), [0.5 / np.sqrt(50), 0.2 / 2], rtol=1e-12)
    # a loop's dump counts every step's clip as a clip, and float32 / torch inputs are taken to float64
    dump = torch.from_numpy(np.stack([out, ref]).astype(np.float32))
    assert tp.token_errors(dump, np.stack([ref, ref])).shape == (4, 2) and tp.clip_errors(dump, np.stack([ref, ref]))[2:].tolist() == [0, 0]
    # ratios: the floor is the clip's median model error (tokens), the median over rows (rows)
    model = ref.copy()
    model[0, :, 0, 0] += 0.05       # clip 0: model token errors (0.05 sqrt 2 / 5, 0): median = half of the first
    m0 = 0.05 * np.sqrt(2) / 5
    np.testing.assert_allclose(tp.token_ratios(out, ref, model)[0], [0.1 / m0, 0.0], rtol=1e-12)
    assert np.isinf(tp.token_ratios(out, ref, model)[1, 1]) or tp.token_ratios(out, ref, model)[1, 1] > 1e100        # no model error at all there


def test_one_token_and_one_row_off_by_a_percent_hide_in_the_pooled_figure_and_fail_the_profiles():
    rng = np.random.default_rng(5)
    shape = (64, 263, 1, 196)
    ref = rng.standard_normal(shape).astype(np.float32)
    model = ref + 4e-4 * rng.standard_normal(shape).astype(np.float32)
    clean = ref + 4e-4 * rng.standard_normal(shape).astype(np.float32)
    assert tp.assert_profiles(clean, ref, model, C_TOK, C_ROW)[1] < 1.5            # two realisations of the same noise: far inside
    tok = clean.copy()
    tok[37, :, 0, 128] *= 1.01                   # frame row 37 x 196 + 128 = 7380: the 20th row of its 64-frame tile
    assert rel_l2(tok, ref) < 4.2e-4 < 1e-3
    with pytest.raises(AssertionError, match=r"clip 37, frame 128, feature \d+: frame row 7380 \(% 64 = 20\), stream token 7418 \(% 64 = 58, % 48 = 26\)"):
        tp.assert_tokens(tok, ref, model, C_TOK_CAP, ntb=3, what="one token")
    assert tp.token_ratios(tok, ref, model).max() > 20
    tp.assert_rows(tok, ref, model, C_ROW)                                       # ... and the rows do not see a token
    row = clean.copy()
    row[11, 250, 0, :] *= 1.01                   # one feature row of ONE clip: 1 / 64 of what the row profile pools
    assert rel_l2(row, ref) < 4.2e-4 < 1e-3
    with pytest.raises(AssertionError, match=r"clip 11, frame \d+, feature 250: .*feature % 16 = 10"):
        tp.assert_tokens(row, ref, model, C_TOK_CAP, what="one row of one clip")             # every token of the clip carries it
    allrows = clean.copy()
    allrows[:, 250, 0, :] *= 1.01                # the row in every clip: sqrt(4e-4^2 + 1e-4 / 263) = 7.3e-4 pooled
    assert rel_l2(allrows, ref) < 8e-4 < 1e-3
    with pytest.raises(AssertionError, match=r"feature 250: .*feature % 16 = 10"):
        tp.assert_rows(allrows, ref, model, C_ROW_CAP, what="one row")
    assert tp.row_ratios(allrows, ref, model).max() > 20


def nudged(monkeypatch):
    """A second realisation of the rounding: operands nudged by 1 + 2^-13 before they are rounded."""
    from oracle import denoiser
    monkeypatch.setattr(denoiser, "_rnd", lambda x, dt: x if dt is None else (x * (1 + 2.0 ** -13)).to(dt).to(torch.float32))


def second_realisation(F, T, B, guided):
    from oracle import denoiser
    w, pe = tc.weights(F)
    i = tc.forward_inputs(F, T, B)
    if guided:
        return denoiser.cfg_forward(w, pe, i["x"], i["t"], i["txt"], i["scale"], dt=torch.float16).numpy()
    return denoiser.forward(w, pe, i["x"], i["t"], i["txt"], dt=torch.float16).numpy()


def forward_shapes():
    return ([(F, T, tc.WIDTH_CLIPS) for F, T in tc.width_cases()] + [(tc.FEATS, T, tc.TRUNK_CLIPS) for T in tc.TRUNK_FRAMES]
            + [(tc.FEATS, T, B) for B, T in tc.SMALL_SHAPES])


def test_the_rounding_model_keeps_inside_its_own_bars_on_every_gpu_case(monkeypatch):
    """The fp16 model as "kernel" passes every assertion of every GPU case (trivially at ratio <= 1: what the test pins is that the
    bars exist -- no zero median, no empty row -- at every shape), and a second rounding realisation with about twice the pooled
    error is reported against the factors in use: the factors must not let it pass as rounding."""
    for F, T, B in forward_shapes():
        for guided in (False, True):
            ref, model = tc.oracle_forward(F, T, B, guided)
            # (the clip bar is absolute, not the model's: the model rounds the projections' activations once, the kernels split them,
            # and at one feature the model itself reads 1.13e-3 on a guided clip)
            _, tok, row = tp.assert_profiles(model, ref, model, C_TOK, C_ROW, what=f"model {F} x {T} x {B}", clip_bar=np.inf)
            assert (tok is None or 0 < tok <= 1) and (row is None or 0 < row <= 1)
            assert (tok is None) == (F < tp.TOKEN_MIN_FEATS) and (row is None) == (B * T < tp.ROW_MIN_SAMPLES)
    for F, T in tc.width_cases():
        for name, _, eta in tc.LOOPS:
            for guided in (False, True):
                ref, model = tc.oracle_loop(F, T, tc.WIDTH_CLIPS, name, eta, guided)
                tp.assert_profiles(model, ref, model, C_TOK, C_ROW, what=f"model {F} x {T} {name} loop, guided {guided}", clip_bar=np.inf)
    nudged(monkeypatch)
    worst_tok, worst_row, least_tok, least_row = (0, None), (0, None), (np.inf, None), (np.inf, None)
    for F, T, B in forward_shapes():
        for guided in (False, True):
            ref, model = tc.oracle_forward(F, T, B, guided)
            other = second_realisation(F, T, B, guided)
            assert not np.array_equal(other, model)
            if F >= tp.TOKEN_MIN_FEATS:
                r = (float(tp.token_ratios(other, ref, model).max()), (F, T, B, guided))
                worst_tok, least_tok = max(worst_tok, r), min(least_tok, r)
            if B * T >= tp.ROW_MIN_SAMPLES:
                r = (float(tp.row_ratios(other, ref, model).max()), (F, T, B, guided))
                worst_row, least_row = max(worst_row, r), min(least_row, r)
    print(f"second realisation, worst ratio of a case: tokens {least_tok[0]:.2f} at {least_tok[1]} .. {worst_tok[0]:.2f} at {worst_tok[1]} "
          f"(c_tok {C_TOK:.2f}), rows {least_row[0]:.2f} at {least_row[1]} .. {worst_row[0]:.2f} at {worst_row[1]} (c_row {C_ROW:.2f})")
    # the nudge doubles the pooled error: a kernel twice as wrong as the model in the bulk does not pass as rounding
    assert worst_tok[0] > C_TOK and worst_row[0] > C_ROW


def test_a_wrong_oracle_input_fails_the_profiles_under_a_clean_pooled_figure():
    """One output feature's bias zeroed on the oracle side only: the pooled relative L2 of the (model) "kernel" against that oracle
    stays under 1e-3, the row assertion names the feature."""
    from oracle import denoiser
    F, T, B = 263, 68, 2
    w, pe = tc.weights(F)
    i = tc.forward_inputs(F, T, B)
    ref, model = tc.oracle_forward(F, T, B, False)
    key = denoiser.PRIOR + "output_process.poseFinal.bias"
    bias = w[key].copy()
    # zeroing b_f moves row f by |b_f| / RMS(row f) and the pooled figure by about 1 / sqrt(263) of that: the feature nearest 8e-3
    # is far above the rows' rounding error (measured: 13 x the row's bar) and adds about 5e-4 to the pooled 4e-4 in quadrature (6.0e-4)
    rms = np.sqrt((tp._bft(ref) ** 2).mean((0, 2)))
    f = int(np.argmin(np.abs(np.abs(bias) / rms - 8e-3)))
    bias[f] = 0
    wrong, wrong_model = tp.rounding_model(denoiser.forward, {**w, key: bias}, pe, i["x"], i["t"], i["txt"])
    pooled = rel_l2(model, wrong)
    print(f"bias of feature {f} ({w[key][f]:.3e}) zeroed in the oracle: pooled {pooled:.3e}, row ratio {tp.row_ratios(model, wrong, wrong_model)[f]:.1f}")
    assert pooled < 1e-3
    with pytest.raises(AssertionError, match=rf"feature {f}: .*feature % 16 = {f % 16}"):
        tp.assert_rows(model, wrong, wrong_model, C_ROW_CAP, what="zeroed bias")
