"""Several styles in one batch on the GPU (csrc/mst_style.h, model/style_bank.py): three synthetic styles (their own seeded stacks,
one shared prior) through the style-aware kernels of both launch paths.

Isolation is checked BITWISE: every stage of the stack is row-independent and the in-kernel noise is keyed by position, so the rows of
a style-s clip in a mixed batch are the rows of the same clip in a batch where every clip uses style s."""
import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
from mst_amd import synthetic as syn
from conftest import SEED, rel_l2
import style_fixture as sf

pytestmark = pytest.mark.gpu

TOL = 1e-3
SHAPES = {"xia": (181, 76), "hml": (263, 196)}
K = 3
PRIOR, LP = sf.PRIOR, sf.LP
_dev, cu, _pe = sf.dev, sf.cu, sf.pe


def style_weights(tag, s):
    return sf.style_weights(SHAPES[tag][0], s)


def _layer_list(w, nl=8):
    return sf.layer_list(w, nl)


def make_engine(tag, max_rows, slots=K):
    F, T = SHAPES[tag]
    return sf.make_engine(F, T, max_rows, slots)


def interleaved(B):
    return [(0, 1, 1, 2, 0, 2)[i % 6] for i in range(B)]


def _inputs(tag, B):
    F, T = SHAPES[tag]
    x = cu(syn.normal(SEED, f"sb/{tag}/x", (B, F, 1, T)))
    t = cu(np.array([(37 * i + 5) % 1000 for i in range(B)]))
    txt = cu(syn.normal(SEED, f"sb/{tag}/txt", (B, 512)))
    scale = cu(np.full(B, 2.5, np.float32))
    return x, t, txt, scale


_schedule = sf.schedule


def run(eng, styles, tag, B, cfg, steps):
    from mst_amd.engine import SAMPLER_DDPM
    x, t, txt, scale = _inputs(tag, B)
    eng.set_text(txt, cfg=cfg)
    eng.set_styles(styles)
    if steps == 0:
        out = eng.forward(x, t, scale=scale if cfg else None, cfg=cfg)
    else:
        out = eng.sample_loop(_schedule(), x.clone(), steps - 1, 0, SAMPLER_DDPM, cfg=cfg, scale=scale if cfg else None, seed=1234)
    torch.cuda.synchronize()
    return out


CASES = [("xia", 4), ("hml", 4), ("hml", 16), ("hml", 64), ("xia", 64)]      # small path (4 clips), fused path (16, 64)


@pytest.mark.parametrize("tag,B", CASES, ids=[f"{t}-{b}" for t, b in CASES])
@pytest.mark.parametrize("cfg", [False, True], ids=["plain", "cfg"])
def test_isolation_bitwise(tag, B, cfg):
    eng = make_engine(tag, 2 * B)
    st = interleaved(B)
    for steps in (0, 50):
        mixed = run(eng, st, tag, B, cfg, steps)
        for s in range(K):
            rows = [i for i in range(B) if st[i] == s]
            alone = run(eng, [s] * B, tag, B, cfg, steps)
            assert torch.equal(mixed[rows], alone[rows]), (steps, s)
        assert not torch.equal(mixed[[0]], run(eng, [1] * B, tag, B, cfg, steps)[[0]])    # the styles do differ


@pytest.mark.parametrize("tag,B", [("xia", 4), ("hml", 16)], ids=["small", "fused"])
def test_one_style_unchanged(tag, B):
    plain = make_engine(tag, B, slots=1)
    bank = make_engine(tag, B)
    for steps in (0, 20):
        a = run(plain, None, tag, B, False, steps)
        b = run(bank, [0] * B, tag, B, False, steps)
        assert torch.equal(a, b), steps


def _oracle_forward(tag, s, x, t, txt):
    return sf.oracle_forward(SHAPES[tag][0], s, x, t, txt)


@pytest.mark.parametrize("tag,B", [("xia", 4), ("hml", 16)], ids=["small", "fused"])
def test_parity_vs_oracle(tag, B):
    from mst_amd.engine import SAMPLER_DDPM
    from oracle import diffusion, schedule
    eng = make_engine(tag, B)
    st = interleaved(B)
    x, t, txt, _ = _inputs(tag, B)
    got = run(eng, st, tag, B, False, 0).cpu().numpy()
    xn, tn, tx = x.cpu().numpy(), t.cpu().numpy(), txt.cpu().numpy()
    for s in range(K):
        rows = [i for i in range(B) if st[i] == s]
        ref = np.asarray(_oracle_forward(tag, s, xn[rows], tn[rows], tx[rows]))
        assert rel_l2(got[rows], ref) < TOL, s
    # a 10-step DDPM loop with recorded noise, one clip per style against the oracle loop of that style
    F, T = SHAPES[tag]
    n = 10
    tab, tmap = schedule.make("cosine", 1000, "")
    nz = syn.normal(SEED, f"sb/{tag}/loopnz", (n + 1, B, F, 1, T))
    eng.set_text(txt)
    eng.set_styles(st)
    sch = _schedule()
    xT = sch.q_sample(torch.zeros(B, F, 1, T, device=_dev()), cu(np.full(B, n - 1)), cu(nz[0]))
    out = eng.sample_loop(sch, xT, n - 1, 0, SAMPLER_DDPM, noise=cu(nz[1:])).cpu().numpy()
    for s in range(K):
        i = st.index(s)
        ref = diffusion.sample_loop(lambda xx, tt: _oracle_forward(tag, s, xx, tt, tx[i:i + 1]), tab, tmap, (1, F, 1, T),
                                    lambda k: torch.from_numpy(nz[k][i:i + 1]), "ddpm", False, None, None,
                                    skip_timesteps=1000 - n)
        assert rel_l2(out[i:i + 1], np.asarray(ref)) < TOL, s


def test_reupload_one_slot():
    tag, B = "hml", 16
    eng = make_engine(tag, B)
    st = interleaved(B)
    before = run(eng, st, tag, B, False, 0)
    w = dict(style_weights(tag, 1))
    w[f"{LP}3.linear1.weight"] = w[f"{LP}3.linear1.weight"] * np.float32(1.5)
    eng.load_layers_slot(1, _layer_list(w))
    after = run(eng, st, tag, B, False, 0)
    other = [i for i in range(B) if st[i] != 1]
    assert torch.equal(before[other], after[other])
    rows = [i for i in range(B) if st[i] == 1]
    x, t, txt, _ = _inputs(tag, B)
    from oracle import denoiser
    ref = np.asarray(denoiser.forward(w, _pe(), x.cpu().numpy()[rows], t.cpu().numpy()[rows], txt.cpu().numpy()[rows], prior=PRIOR))
    assert rel_l2(after[rows].cpu().numpy(), ref) < TOL


def test_refusals(monkeypatch):
    tag, B = "xia", 4
    eng = make_engine(tag, B)
    with pytest.raises(RuntimeError, match="outside"):
        eng.set_styles([0, 1, 3, 0])
    x, t, txt, _ = _inputs(tag, B)
    eng.set_text(txt)
    eng.set_styles(interleaved(B))
    eng.set_precise(True)
    with pytest.raises(RuntimeError, match="precise"):
        eng.forward(x, t)
    eng.set_precise(False)
    monkeypatch.setenv("MST_TRUNK", "1")
    eng2 = make_engine(tag, B)
    eng2.set_text(txt)
    eng2.set_styles(interleaved(B))
    with pytest.raises(RuntimeError, match="MST_TRUNK"):
        eng2.forward(x, t)


def _bank(tag):
    from mst_amd.model.mdm_forstyledataset import StyleDiffusion
    from mst_amd.model.style_bank import StyleBank
    F, _ = SHAPES[tag]
    models = []
    for s in range(K):
        m = StyleDiffusion("", F, 1, 1, True, "rot6d", True, True, latent_dim=512, ff_size=1024, num_layers=8, num_heads=4,
                           dropout=0.1, activation="gelu", data_rep="hml_vec", cond_mode="text", cond_mask_prob=0.1,
                           arch="trans_enc", dataset="stylexia_posrot")
        sd = {k: torch.from_numpy(v) for k, v in style_weights(tag, s).items()}
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not unexpected
        models.append(m.to(_dev()).eval())
    return StyleBank(models), models


def test_bank_through_the_samplers():
    """p_sample_loop / ClassifierFreeSampleModel with a bank: each style's clips equal the same clips sampled with that style alone,
    and a model call equals the member's own call; autograd samplers refuse."""
    from mst_amd.diffusion import gaussian_diffusion as gd
    from mst_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    from mst_amd.model.cfg_sampler import ClassifierFreeSampleModel
    tag, B = "xia", 8
    F, T = SHAPES[tag]
    bank, models = _bank(tag)
    d = SpacedDiffusion(use_timesteps=space_timesteps(1000, "20"), betas=gd.get_named_beta_schedule("cosine", 1000),
                        model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE)
    st = torch.tensor(interleaved(B))
    x, t, txt, scale = _inputs(tag, B)
    with torch.no_grad():
        out = bank(x, t, {"text_embed": txt, "style": st})
        for s in range(K):
            rows = (st == s).nonzero().flatten().tolist()
            own = models[s](x[rows], t[rows], {"text_embed": txt[rows]})
            assert rel_l2(out[rows].cpu().numpy(), own.cpu().numpy()) < 1e-5, s
    for model in (bank, ClassifierFreeSampleModel(bank)):
        res = {}
        for key, styles in (("mixed", st), *((s, torch.full((B,), s)) for s in range(K))):
            torch.manual_seed(7)
            y = {"text_embed": txt, "style": styles, "scale": scale}
            res[key] = d.p_sample_loop(model, (B, F, 1, T), model_kwargs={"y": y}, progress=False)
        for s in range(K):
            rows = (st == s).nonzero().flatten().tolist()
            assert torch.equal(res["mixed"][rows], res[s][rows]), s
    with pytest.raises(RuntimeError, match="StyleBank"):
        d.p_sample_loop(bank, (B, F, 1, T), model_kwargs={"y": {"text_embed": txt, "style": st}}, progress=False,
                        cond_fn_with_grad=True)
    with pytest.raises(ValueError, match="outside"):
        d.p_sample_loop(bank, (B, F, 1, T), model_kwargs={"y": {"text_embed": txt, "style": st + 1}}, progress=False)


def test_unloaded_slot_is_refused():
    """A slot that mst_style_slots allocated but mst_load_layers_slot never filled holds uninitialised memory: naming it is refused,
    and the refused call leaves the engine's styles as they were (nothing runs with that slot).  Growing keeps loaded slots loaded."""
    tag, B = "xia", 4
    eng = make_engine(tag, B)                           # slots 1-2 loaded
    eng.style_slots(4)                                  # slot 3: allocated only
    x, t, txt, _ = _inputs(tag, B)
    eng.set_text(txt)
    eng.set_styles([0, 1, 2, 1])
    before = eng.forward(x, t)
    with pytest.raises(RuntimeError, match=r"slot 3, which was never loaded \(mst_load_layers_slot\)"):
        eng.set_styles([0, 1, 3, 2])
    with pytest.raises(RuntimeError, match="outside"):                          # the range check comes first
        eng.set_styles([0, 4, 3, 0])
    assert torch.equal(eng.forward(x, t), before)
    eng.load_layers_slot(3, _layer_list(style_weights(tag, 3)))
    eng.set_styles([0, 1, 3, 2])
    out = eng.forward(x, t).cpu().numpy()
    ref = np.asarray(_oracle_forward(tag, 3, x.cpu().numpy()[[2]], t.cpu().numpy()[[2]], txt.cpu().numpy()[[2]]))
    assert rel_l2(out[[2]], ref) < TOL


def test_training_entries_refuse_styles():
    """The training stack runs slot 0 only: with styles set, mst_train_forward, mst_train_model_forward and mst_motion_encoder_forward
    refuse; after set_styles(None) they give the bits of an engine that never had slots (dropout 0)."""
    tag, B = "xia", 2
    F, T = SHAPES[tag]
    plain, bank = make_engine(tag, B, slots=1), make_engine(tag, B)
    x, t, txt, _ = _inputs(tag, B)
    h = cu(syn.normal(SEED, "sb/train/h", (B, T + 1, 512)))
    mu_q, sg_q = cu(syn.normal(SEED, "sb/train/mu", (512,))), cu(syn.normal(SEED, "sb/train/sigma", (512,)))
    x_me = x[..., :T - 1].contiguous()                  # the motion encoder adds 2 query tokens: at most T - 1 frames here
    keep = torch.ones(B, T + 1, dtype=torch.bool)

    def model_forward(e):
        e.set_text(txt)
        return e.train_model_forward(x, t, 0.0, 0.0, 5)[0]

    calls = {"mst_train_forward": lambda e: e.train_forward(h, 0.0, 5)[0],
             "mst_train_model_forward": model_forward,
             "mst_motion_encoder_forward": lambda e: e.motion_encoder_forward(x_me, mu_q, sg_q, keep, 0.0, 0.0, 5)[0]}
    bank.set_text(txt)
    bank.set_styles([1, 2])
    for name, fn in calls.items():
        with pytest.raises(RuntimeError, match=f"{name}: styles are set \\(mst_set_styles / StyleBank\\)"):
            fn(bank)
    bank.set_styles(None)
    for name, fn in calls.items():
        a, b = fn(plain), fn(bank)
        torch.cuda.synchronize()
        assert torch.equal(a, b), name
