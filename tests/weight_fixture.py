"""Weight changes shared by the weight-coherence tests (test_gpu_weight_coherence.py, test_weight_watch_cpu.py): the small Xia-shape
denoiser of tests/test_gpu_edges.py::make, a perturbation per tensor that the fp32 oracle SEES (the visibility rule), and every
consumer of an engine's derived weight copies as one function, so that a warm engine and a fresh one can be compared bit for bit.

The visibility rule.  A stale derived copy must not be able to pass for rounding: each change a test makes moves the oracle's forward
by at least VISIBLE = 5e-3 relative L2, five times the project's 1e-3 parity bar.  `assert_visible` states it inside the test, with the
oracle, so that a later change of fixture cannot silently remove it."""
import numpy as np
import torch

from mst_amd import synthetic as syn
from conftest import rel_l2

F, T = 181, 76
SEED = 77
LP, PRIOR = "seqTransEncoder.layers.", "motion_enc.mdm_model."
PE = "sequence_pos_encoder.pe"
TOL = 1e-3           # the project's parity bar against the fp32 oracle
VISIBLE = 5e-3       # what a weight change must move the oracle's forward by

# The six tensors that only shape the conditioning token (one of 77 tokens): 1.25 w + 0.01 sign(w) moves the forward by 1.1e-4 .. 4.3e-3,
# under VISIBLE; they take the larger step below (measured on the CPU: see matrix_cases' docstring).
CONDITIONING = ("embed_timestep.time_embed.0.weight", "embed_timestep.time_embed.0.bias", "embed_timestep.time_embed.2.weight",
                "embed_timestep.time_embed.2.bias", "embed_text.weight", "embed_text.bias")


def engine_names():
    from mst_amd.engine import LAYER_TENSORS, PRIOR_TENSORS
    return LAYER_TENSORS, PRIOR_TENSORS


def state_key(name):
    """Engine tensor name -> key of the reference-layout state dict (the stack's tensors are the style denoiser's own, the rest the prior's)."""
    return name if name.startswith(LP) else PRIOR + name


def bump(a, big=False):
    """The perturbation: 1.25 w + 0.01 sign(w); for the conditioning-token tensors 3 w + 0.5 sign(w) (the existing table test adds 0.5)."""
    a = np.asarray(a, np.float32)
    if big:
        return (np.float32(3.0) * a + np.float32(0.5) * np.sign(a)).astype(np.float32)
    return (np.float32(1.25) * a + np.float32(0.01) * np.sign(a)).astype(np.float32)


def bump_name(name, a):
    return bump(a, big=name.endswith(CONDITIONING))


_BASE = {}


def base_state(seed=SEED):
    """(state dict of numpy float32 arrays, positional table): never mutated -- callers copy the dict."""
    if seed not in _BASE:
        _BASE[seed] = syn.denoiser_state(seed, F)
    if "pe" not in _BASE:
        _BASE["pe"] = syn.positional_table(5000, 512)
    return _BASE[seed], _BASE["pe"]


def matrix_cases():
    """The one-tensor reload matrix: the 12 layer tensors at layers 0 and 7, the 10 non-table prior tensors, the positional table.
    Oracle movement of each cumulative step, measured on the CPU (B = 2, t = [10, 900]): see docs/LAB_NOTES.md (weight coherence)."""
    layer, prior = engine_names()
    return [f"{LP}{l}.{k}" for l in (0, 7) for k in layer] + [k for k in prior if k != PE] + [PE]


def state_after(k, seed=SEED):
    """State after the matrix's cases 0 .. k were applied on top of each other (k = -1: the base state)."""
    w, pe = base_state(seed)
    w = dict(w)
    for name in matrix_cases()[:k + 1]:
        if name == PE:
            pe = bump(pe)
        else:
            w[state_key(name)] = bump_name(name, w[state_key(name)])
    return w, pe


def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def probe_inputs(B=2):
    x = syn.normal(SEED, "wc/x", (B, F, 1, T))
    txt = syn.normal(SEED, "wc/txt", (B, 512))
    t = np.array([10, 900, 431, 7, 650, 12, 300, 880][:B])
    return x, t, txt


_ORACLE = {}


def oracle_forward(w, pe, key=None):
    """The fp32 oracle's forward of the probe inputs; `key` caches it (the matrix walks 35 cumulative states)."""
    from oracle import denoiser
    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    x, t, txt = probe_inputs()
    out = denoiser.forward(w, pe, x, t, txt).numpy()
    if key is not None:
        _ORACLE[key] = out
    return out


def assert_visible(old, new, what=""):
    """The visibility rule, on the oracle: (w, pe) pairs or ready forwards."""
    a = oracle_forward(*old) if isinstance(old, tuple) else old
    b = oracle_forward(*new) if isinstance(new, tuple) else new
    d = rel_l2(b, a)
    print(f"visibility {what}: oracle moved by {d:.3e}")
    assert d >= VISIBLE, f"{what}: the change moves the oracle's forward by {d:.3e} < {VISIBLE:g}: a stale copy could pass for rounding"
    return d


def make_engine(w, pe, max_rows, frames=T):
    from mst_amd.engine import DenoiserEngine
    eng = DenoiserEngine(F, frames, max_rows, device=dev())
    load_all(eng, w, pe)
    return eng


def load_all(eng, w, pe):
    eng.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, pe=torch.from_numpy(pe))


def layer_list(w, nl=8):
    layer, _ = engine_names()
    return [cu(w[f"{LP}{i}.{k}"]) for i in range(nl) for k in layer]


# ------------------------------------------------------------------------------------------------------------- consumers
B_SMALL, B_LARGE = 2, 26          # 2 x 77 = 154 stream rows: the small-launch path; 26 x 77 = 2002 rows: past the hand-over (1900), two-kernel path
MAX_ROWS = 2 * B_LARGE            # a guided forward doubles the rows


def _schedule():
    from mst_amd.engine import Schedule
    from oracle import schedule as osch
    if "sch" not in _ORACLE:
        tab, tmap = osch.make("cosine", 1000, "")
        _ORACLE["sch"] = Schedule(tab, tmap, dev())
    return _ORACLE["sch"]


_IN = {}


def _inputs():
    """Device inputs of every consumer, made once (the same tensors for both engines of a comparison)."""
    if _IN:
        return _IN
    n = lambda tag, shape: cu(syn.normal(SEED, "wc/" + tag, shape))
    for B, tag in ((B_SMALL, "s"), (B_LARGE, "l")):
        _IN["x" + tag] = n("x" + tag, (B, F, 1, T))
        _IN["txt" + tag] = n("txt" + tag, (B, 512))
        _IN["t" + tag] = cu(np.array([(37 * i + 10) % 1000 for i in range(B)]))
        _IN["d" + tag] = n("d" + tag, (B, F, 1, T))
        _IN["h" + tag] = n("h" + tag, (B, T + 1, 512))
        _IN["dh" + tag] = n("dh" + tag, (B, T + 1, 512))
    xp, tp, txtp = probe_inputs()
    _IN["xs"], _IN["ts"], _IN["txts"] = cu(xp), cu(tp), cu(txtp)          # the small forward IS the oracle's probe
    _IN["scale"] = cu(np.linspace(1.5, 2.5, B_SMALL).astype(np.float32))
    _IN["mask"] = cu(syn.root_horizontal_mask(B_SMALL, F, T))
    _IN["motion"] = n("motion", (B_SMALL, F, 1, T))
    _IN["xme"] = n("xme", (B_SMALL, F, 1, T - 1))                         # the motion encoder adds 2 query tokens: T - 1 frames fit
    _IN["muq"], _IN["sgq"] = n("muq", (512,)), n("sgq", (512,))
    keep = torch.ones(B_SMALL, T + 1, dtype=torch.bool)
    keep[1, T - 6:] = False
    _IN["keep_me"] = keep
    _IN["dmu"] = n("dmu", (B_SMALL, 512))
    kl = torch.ones(B_LARGE, T + 1, dtype=torch.bool)
    kl[3, T - 9:] = False
    kl[17, T - 30:] = False
    _IN["keep_l"] = kl
    return _IN


def _grads(w_shapes):
    return [torch.zeros(s, device=dev()) for s in w_shapes]


def consumers(eng, sampling=True, training=True):
    """Every reader of a derived weight copy, in one fixed order; returns {name: tensor or list of tensors}.

    forward/small        wsm_*, w_pose_*_pk, temb_table          (small_dirty, pose_in_dirty, pose_out_dirty, temb_table_valid)
    forward/large        wqkv, wtail, w_pose_*_pk                (qkv_dirty, tail_dirty)
    forward/cfg          the same copies over the doubled batch
    loop                 chained frame rows + embed-next fusion: the packed pose projections inside a 3-step inpainting loop
    train_model/small    plain [out][in] + wsm_* forward, [in][out] transposes backward, all 96 gradients
    train/large          k_layer_tail_train reads wtail; dgrad GEMMs read the transposes
    train/large/frozen   key_keep mask, no parameter gradients: k_layer_tail_bwd reads wtail_bwd (tailb_dirty)
    motion_encoder       pose embedding + masked stack forward and backward"""
    from mst_amd.engine import SAMPLER_DDPM
    i = _inputs()
    layer, _ = engine_names()
    shapes = [(1536, 512), (1536,), (512, 512), (512,), (1024, 512), (1024,), (512, 1024), (512,), (512,), (512,), (512,), (512,)] * 8
    out = {}
    if sampling:
        eng.set_text(i["txts"])
        out["forward/small"] = eng.forward(i["xs"], i["ts"])
        eng.set_text(i["txtl"])
        out["forward/large"] = eng.forward(i["xl"], i["tl"])
        eng.set_text(i["txts"], cfg=True)
        out["forward/cfg"] = eng.forward(i["xs"], i["ts"], scale=i["scale"], cfg=True)
        eng.set_text(i["txts"])
        sch = _schedule()
        x3 = sch.q_sample(i["motion"], cu(np.full(B_SMALL, 2)), i["xs"], i["mask"])
        out["loop"] = eng.sample_loop(sch, x3, 2, 0, SAMPLER_DDPM, mask=i["mask"], motion=i["motion"], seed=31)
    if training:
        eng.set_text(i["txts"])
        o, tape = eng.train_model_forward(i["xs"], i["ts"], 0.1, 0.1, 4242)
        g = _grads(shapes)
        dx = eng.train_model_backward(tape, i["ds"], 0.1, 0.1, 4242, g)
        out["train_model/small"] = [o, dx] + g
        o, tape = eng.train_forward(i["hl"], 0.1, 977)
        g = _grads(shapes)
        dh = eng.train_backward(tape, i["dhl"], 0.1, 977, g)
        out["train/large"] = [o, dh] + g
        o, tape = eng.train_forward(i["hl"], 0.0, 0, key_keep=i["keep_l"])
        dh = eng.train_backward(tape, i["dhl"], 0.0, 0, None, key_keep=i["keep_l"])
        out["train/large/frozen"] = [o, dh]
        mu, tape = eng.motion_encoder_forward(i["xme"], i["muq"], i["sgq"], i["keep_me"], 0.1, 0.1, 55)
        dxm = eng.motion_encoder_backward(tape, i["dmu"], i["keep_me"], T - 1, 0.1, 0.1, 55)
        out["motion_encoder"] = [mu, dxm]
    torch.cuda.synchronize()
    return out


def assert_same_bits(a, b, what=""):
    """Two consumer results, bit for bit (and finite: equal NaNs would be `torch.equal`-unequal anyway, equal infinities not)."""
    assert a.keys() == b.keys()
    for name in a:
        xs, ys = (a[name], b[name]) if isinstance(a[name], list) else ([a[name]], [b[name]])
        assert len(xs) == len(ys)
        for j, (x, y) in enumerate(zip(xs, ys)):
            assert torch.isfinite(x).all(), (what, name, j)
            assert torch.equal(x, y), f"{what}: {name}[{j}] differs from the fresh engine's: max |diff| {float((x - y).abs().max()):.3e}"
