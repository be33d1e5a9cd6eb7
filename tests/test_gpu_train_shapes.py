"""The native TRAINING path at every shape its dispatch tells apart (csrc/mst_engine.hip: train_stack_forward, wgrad,
train_stack_backward), against a float64 PyTorch reference of the same eight layers on the GPU, so that the tolerances measure
the kernels alone.

  A. attention tile counts: k_attention_train<NKT> / k_attention_bwd<NKT> for NKT = 3..7 (NKT = ceil(S / 32)), with a partial and
     a full last key tile, on both tile paths (query-split / split backward = 1 on the small one, = 0 on the large one);
  B. key padding at every tile count: padding from a tile boundary, last key tiles entirely padding; and the frozen MotionEncoder
     at 64 clips x 196 frames with ragged lengths (large tiles, fused backward tail);
  C. split-K plans of the four weight gradients (one split, the XCD grid, the 3-D grid, short last splits; k_ln_bwd<16>), each
     case's plan derived by a mirror of wgrad()'s arithmetic and named in its test id;
  D. a tape filled with 0xFF bytes (NaN in f16 and f32) gives bit-identical results to a zeroed one: no kernel reads tape memory
     that train_forward did not write.

Bars of tests/test_gpu_train.py: forward 1e-3, dL/dh 1.5e-3, every one of the 96 parameter-gradient tensors 1.5e-3 -- at two or three
clips too, where that file allows 2x against its fp32 reference: against fp64 the worst tensor of every case here measured <= 7.4e-4."""
import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
from mst_amd import synthetic as syn
from mst_amd.engine import LAYER_TENSORS
from conftest import SEED, rel_l2

from test_gpu_train import TOL_FWD, TOL_GRAD, D, L, _style_model, engine_masks, layer_params, torch_stack
from torch_reference import use_native, use_torch_ops

pytestmark = pytest.mark.gpu

FE = 263
MAX_FRAMES = 223                       # S up to 224: the engine's maximum
MAX_ROWS = 37                          # 37 x 197 = 7289 token rows, the largest case here
TILE_PATHS = {"small": "2048", "large": "0"}     # MST_SMALL_M, read when an engine is created
WGRADS = (("W2", 512, 1024), ("W1", 1024, 512), ("Wout", 512, 512), ("Win", 1536, 512))


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


_ENG = {}


def weights():
    if "w" not in _ENG:
        _ENG["w"] = syn.denoiser_state(SEED, FE, layer_prefix="seqTransEncoder.layers.")
    return _ENG["w"]


def engine(path):
    """One engine per tile path, shared by every case of this module."""
    from mst_amd.engine import DenoiserEngine
    if path not in _ENG:
        w = weights()
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("MST_SMALL_M", TILE_PATHS[path])
            eng = DenoiserEngine(FE, MAX_FRAMES, MAX_ROWS, device=_dev())
        eng.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, layer_prefix="seqTransEncoder.layers.",
                            pe=torch.from_numpy(syn.positional_table(5000, 512)))
        _ENG[path] = eng
    return _ENG[path]


def nkt(S):
    return (S + 31) // 32


def wgrad_plan(M):
    """Mirror of wgrad()'s split arithmetic (csrc/mst_engine.hip, default MST_WGRAD_WGS / MST_WGRAD_XCD, split_cap 64) for a layer's
    four weight gradients: name -> (grid, number of splits, tokens in the last split)."""
    cdiv = lambda a, b: -(-a // b)
    plan = {}
    for name, n_out, k_in in WGRADS:
        tiles = (n_out // 128) * (k_in // 256)
        nsplit = cdiv(128, tiles)
        slabs = cdiv(M, 32)
        xcd = M > 2048 and slabs >= 64
        if xcd:
            nsplit = cdiv(nsplit, 8) * 8
        nsplit = min(nsplit, slabs, 64)
        if M <= 2048:
            nsplit = 1
        kchunk = cdiv(slabs, nsplit) * 32
        nsplit = cdiv(M, kchunk)
        if nsplit % 8:
            xcd = False
        grid = "one" if nsplit == 1 else ("xcd" if xcd else "grid")
        plan[name] = (grid, nsplit, M - (nsplit - 1) * kchunk)
    return plan


def plan_str(M):
    return "-".join(f"{n}.{g}{k}.last{last}" for n, (g, k, last) in wgrad_plan(M).items())


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def stream(rows, S, tag):
    h = torch.from_numpy(syn.normal(SEED, f"shapes/{tag}/h/{rows}/{S}", (rows, S, D)).astype(np.float32)).to(_dev())
    r = torch.from_numpy(syn.normal(SEED, f"shapes/{tag}/r/{rows}/{S}", (rows, S, D)).astype(np.float32)).to(_dev())
    return h, r


def reference(eng, h, r, p, seed, keep=None):
    """fp64 autograd of the eight layers with the engine's own dropout masks: (output, dL/dh, the 96 parameter gradients)."""
    rows, S, _ = h.shape
    params = [q.double().requires_grad_(True) for q in layer_params(weights(), False)]
    href = h.double().requires_grad_(True)
    masks = engine_masks(eng, seed, p, rows, S) if p > 0 else None
    out = torch_stack(href, params, masks, keep)
    (out * r.double()).sum().backward()
    del masks
    return out.detach(), href.grad, [q.grad for q in params]


def run_engine(eng, h, r, p, seed, keep=None, frozen=False, tape=None):
    out, tape = eng.train_forward(h, p, seed, tape=tape, key_keep=keep)
    grads = None if frozen else [torch.zeros_like(q) for q in layer_params(weights(), False)]
    d_in = eng.train_backward(tape, r, p, seed, grads, key_keep=keep)
    return out, d_in, grads


def check(label, got, want, valid=None):
    """Forward (on the real rows when `valid` is given), dL/dh and all 96 gradient tensors; prints the worst tensor."""
    (out, d_in, grads), (r_out, r_din, r_grads) = got, want
    if valid is not None:
        out, r_out = out * valid, r_out * valid
    errs = {"out": _rel(out, r_out), "d_in": _rel(d_in, r_din)}
    gerrs = {f"L{i // 12}.{LAYER_TENSORS[i % 12]}": _rel(g, q) for i, (g, q) in enumerate(zip(grads, r_grads))}
    assert len(gerrs) == 12 * L
    worst = max(gerrs, key=gerrs.get)
    print(f"{label}: out {errs['out']:.2e}, d_in {errs['d_in']:.2e}, worst gradient {worst} {gerrs[worst]:.2e}")
    assert errs["out"] <= TOL_FWD, (label, errs)
    assert errs["d_in"] <= TOL_GRAD, (label, errs)
    assert gerrs[worst] <= TOL_GRAD, (label, worst, gerrs[worst], {k: round(v, 5) for k, v in gerrs.items()})


def label(rows, S, path, p, extra=""):
    return f"{rows}x{S} NKT {nkt(S)} {path} tiles p {p}{extra} wgrad {plan_str(rows * S)}"


# ------------------------------------------------------------------------------ A. attention tile counts
TILE_S = (96, 97, 128, 129, 160, 161, 192, 193, 224)


@pytest.mark.parametrize("path", list(TILE_PATHS))
@pytest.mark.parametrize("S", TILE_S, ids=[f"S{S}-NKT{nkt(S)}-{'full' if S % 32 == 0 else 'partial'}" for S in TILE_S])
def test_attention_tile_count_forward_backward(S, path):
    rows, p = 2, (0.0, 0.2)[TILE_S.index(S) % 2]
    eng = engine(path)
    h, r = stream(rows, S, "tiles")
    seed = 4242 + S
    want = reference(eng, h, r, p, seed)
    check(label(rows, S, path, p), run_engine(eng, h, r, p, seed), want)


# ------------------------------------------------------------------------------ B. key padding at every tile count
PAD_S = (33, 97, 161, 198, 224)


def pad_keep(S):
    """Three clips: unpadded; padding from a 32-key tile boundary; padding from 5 keys before a boundary, so that the last one (NKT 2)
    or two key tiles hold padding only."""
    n = nkt(S)
    keep = torch.ones(3, S, dtype=torch.bool, device=_dev())
    keep[1, 32 * ((n + 1) // 2):] = False
    keep[2, 32 * (n - min(2, n - 1)) - 5:] = False
    return keep


@pytest.mark.parametrize("path", list(TILE_PATHS))
@pytest.mark.parametrize("S", PAD_S, ids=[f"S{S}-NKT{nkt(S)}" for S in PAD_S])
def test_key_padding_every_tile_count(S, path):
    rows, p = 3, (0.1, 0.0)[PAD_S.index(S) % 2]
    eng = engine(path)
    keep = pad_keep(S)
    valid = keep[:, :, None].float()
    h, r = stream(rows, S, "pad")
    r = r * valid                                 # outputs at padded positions are unconstrained: score the real ones
    seed = 9000 + S
    want = reference(eng, h, r, p, seed, keep)
    got = run_engine(eng, h, r, p, seed, keep)
    check(label(rows, S, path, p, f" padded from {[int(k.sum()) for k in keep]}"), got, want, valid)
    # a padded position is no key for anybody and its own output is not scored: its whole gradient is what its K / V rows receive, and
    # that has to be exactly zero in every layer (any nonzero dK / dV there reaches dL/dh through the QKV dgrad)
    assert float(want[1][~keep].abs().max()) == 0.0
    assert float(got[1][~keep].abs().max()) == 0.0, "padded keys received a K/V gradient"


def test_motion_encoder_64_clips_humanml_lengths():
    """The fine-tune's frozen MotionEncoder at batch size: 64 clips x 196 frames (S = 198, NKT 7, large tiles, fused backward tail) with
    ragged HumanML3D-like lengths (40..196 frames), native against torch ops with src_key_padding_mask (tests/torch_reference.py)."""
    m = _style_model().eval()
    enc = m.motion_enc
    B, T = 64, 196
    x = torch.from_numpy(syn.normal(SEED, "shapes/me/x", (B, 181, 1, T))).to(_dev())
    lengths = np.random.default_rng(SEED).integers(40, T + 1, B)
    lengths[:5] = (T, 40, 62, 158, 190)          # full; shortest; key padding from 64, from 160 (last two tiles), from 192 (last tile)
    fm = (torch.arange(T)[None, :] < torch.from_numpy(lengths)[:, None]).float().view(B, 1, 1, T).to(_dev())
    y = {"mask": fm, "text_embed": torch.from_numpy(syn.normal(SEED, "shapes/me/emb", (B, 512))).to(_dev())}
    w = torch.from_numpy(syn.normal(SEED, "shapes/me/w", (B, 512))).to(_dev())
    res = {}
    for backend in ("native", "torch"):
        (use_torch_ops if backend == "torch" else use_native)(m)
        xin = x.clone().requires_grad_(True)
        mu, _ = enc(xin, y=y)
        (mu * w).sum().backward()
        res[backend] = (mu.detach(), xin.grad.clone())
    use_native(m)
    e_mu, e_dx = rel_l2(res["native"][0].cpu().numpy(), res["torch"][0].cpu().numpy()), rel_l2(res["native"][1].cpu().numpy(), res["torch"][1].cpu().numpy())
    print(f"MotionEncoder 64 x {T}: mu {e_mu:.2e}, input gradient {e_dx:.2e}")
    assert e_mu <= TOL_FWD and e_dx <= TOL_GRAD, (e_mu, e_dx)
    for b in range(B):                           # frames behind the padding never influence mu
        if lengths[b] < T:
            assert float(res["native"][1][b, ..., int(lengths[b]):].abs().max()) == 0.0, b


# ------------------------------------------------------------------------------ C. split-K plans with parameter gradients
SPLIT_CASES = ((10, 197, 0.0), (27, 77, 0.1), (11, 197, 0.0), (21, 197, 0.1), (37, 197, 0.1))


@pytest.mark.parametrize("rows,S,p", SPLIT_CASES, ids=[f"{r}x{S}-M{r * S}-{plan_str(r * S)}" for r, S, _ in SPLIT_CASES])
def test_split_k_plans_vs_fp64(rows, S, p):
    eng = engine("large")
    h, r = stream(rows, S, "split")
    seed = 31337 + rows
    want = reference(eng, h, r, p, seed)
    check(label(rows, S, "large", p) + (" k_ln_bwd<16>" if rows * S > 4096 else ""), run_engine(eng, h, r, p, seed), want)


def test_split_k_gradient_is_the_sum_of_two_parts():
    """Reference-free: 21 x 197 (3-D grid, 15 splits; XCD grid) = 10 x 197 (one split) + 11 x 197 (3-D grid, 14 splits)."""
    eng = engine("large")
    h, r = stream(21, 197, "sum")
    _, d_full, g_full = run_engine(eng, h, r, 0.0, 0)
    _, d_a, g_a = run_engine(eng, h[:10].contiguous(), r[:10].contiguous(), 0.0, 0)
    _, d_b, g_b = run_engine(eng, h[10:].contiguous(), r[10:].contiguous(), 0.0, 0)
    assert _rel(torch.cat([d_a, d_b]), d_full) < 1e-5
    errs = {f"L{i // 12}.{LAYER_TENSORS[i % 12]}": _rel(a + b, f) for i, (f, a, b) in enumerate(zip(g_full, g_a, g_b))}
    worst = max(errs, key=errs.get)
    print(f"21 x 197 vs 10 + 11 clips: worst gradient {worst} {errs[worst]:.2e}")
    assert errs[worst] < 2e-5, (worst, errs[worst])


# ------------------------------------------------------------------------------ D. poisoned tape
POISON_CASES = (("small", 2, 77, False, False), ("large", 27, 77, False, False), ("large", 3, 198, True, True))


@pytest.mark.parametrize("path,rows,S,padded,frozen", POISON_CASES,
                         ids=[f"{pa}-{r}x{S}" + ("-keypad-frozen" if fz else "") for pa, r, S, _, fz in POISON_CASES])
def test_tape_pad_rows_are_never_read(path, rows, S, padded, frozen):
    """The same pass into a zeroed tape and into one filled with 0xFF bytes (NaN as f16 and as f32): output, dL/dh and every gradient
    bit-identical and finite -- the path is bit-reproducible, so any difference is a read of tape memory train_forward did not write."""
    eng = engine(path)
    h, r = stream(rows, S, "poison")
    keep = pad_keep(S) if padded else None
    if padded:
        r = r * keep[:, :, None].float()
    p, seed = 0.1, 271828 + rows
    clean = run_engine(eng, h, r, p, seed, keep, frozen, tape=eng.train_tape(rows, S, zero=True))
    poisoned = eng.train_tape(rows, S)
    poisoned.fill_(0xFF)
    dirty = run_engine(eng, h, r, p, seed, keep, frozen, tape=poisoned)
    print(f"{rows}x{S} NKT {nkt(S)} {path} tiles{' key-padded frozen' if frozen else ''}: zeroed vs 0xFF tape")
    for name, a, b in (("out", clean[0], dirty[0]), ("d_in", clean[1], dirty[1])):
        assert torch.isfinite(a).all() and torch.equal(a, b), name
    if not frozen:
        for i, (a, b) in enumerate(zip(clean[2], dirty[2])):
            name = f"L{i // 12}.{LAYER_TENSORS[i % 12]}"
            assert torch.isfinite(a).all() and torch.equal(a, b), name
