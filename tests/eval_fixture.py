"""numpy restatement of the reference's T2M evaluators (data_loaders/humanml/networks/modules.py: `MovementConvEncoder` :79-98,
`TextEncoderBiGRUCo` :311-350, `MotionEncoderBiGRUCo` :353-386, under `EvaluatorMDMWrapper`, networks/evaluator_wrapper.py:121-187) and
of its statistics (data_loaders/humanml/utils/metrics.py).

Nothing here imports the reference and no weight is taken from it: every weight and input comes from a seed through mst_amd.synthetic,
at the modules' own init scales -- Xavier-normal for Conv1d / Linear, U(+-1/sqrt(H)) for the GRU, N(0, 1) for `hidden`.  Two departures,
both so that a path is exercised at all: biases are 0.02 N(0, 1) where `init_weight` zeroes them, and LayerNorm's gain / bias are
1 + 0.1 N / 0.1 N.  Every function takes a dtype and runs in it, so one set of inputs evaluates in float32 and in float64.

Packed sequences: clip b runs `steps[b]` positions, forward from position 0, backward from position steps[b] - 1 (the clip's end, not the
tensor's); the result is `gru_last`, both directions' final states."""
import functools
import math

import numpy as np

import mst_amd.synthetic as syn

SEED = 20261020
FLOOR = 1e-6
REAL = dict(hid=512, lat=512, Hm=1024, Ht=512, out=512, word=300, pos=15)
SMALL = dict(hid=64, lat=64, Hm=64, Ht=64, out=32, word=20, pos=15)
SMALL_POSE = 12

# name -> (dim_pose, B, T, lengths kind): the real widths.  T = 5 and 7 exercise the convolutions' floor, the mixed sets a backward
# direction that starts at the tensor's end instead of the clip's.
MOTION_CASES = {
    "h263_b33_t196_mixed": (263, 33, 196, "mixed"),
    "k251_b17_t200_mixed": (251, 17, 200, "mixed"),
    "h263_b2_t196_full": (263, 2, 196, "full"),
    "k251_b1_t196_full": (251, 1, 196, "full"),
    "h263_b33_t200_one": (263, 33, 200, "one"),
    "h263_b1_t7_full": (263, 1, 7, "full"),
    "k251_b2_t5_full": (251, 2, 5, "full"),
    "h263_b17_t4_one": (263, 17, 4, "one"),
}
# name -> (B, L, kind): the text encoder, K = 15 and 300
TEXT_CASES = {"b33_l20_mixed": (33, 20, "mixed"), "b17_l20_one": (17, 20, "one"), "b2_l5_full": (2, 5, "full"), "b1_l20_full": (1, 20, "full")}
STORED = ("h263_b1_t7_full", "k251_b2_t5_full", "h263_b2_t196_full")       # motion cases whose reference outputs eval.npz holds
STORED_TEXT = ("b2_l5_full",)
SMALL_T = 20                                                                # 5 movement frames: every step count 1 .. 5
SMALL_BATCHES = tuple(range(1, 35))
FID_CLIPS = 200                                                             # clips a set of the end-to-end FID case (small net, D = 32)
STAT_N, STAT_D = 32, 512                                                    # the R-precision batch of the reference's eval loop
DIVERSITY_TIMES, MM_SENTS, MM_PER, MM_TIMES = 20, 6, 12, 10
NP_SEED = 1234


def bar(distance):
    """4 x the reference's own fp32-to-f64 distance, floor 1e-6 (rotdec_fixture.bar)."""
    return max(4.0 * float(distance), FLOOR)


def relmax(a, b):
    """max |a - b| relative to the largest magnitude of b."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def conv_frames(T):
    return (T - 2) // 2 + 1 if T >= 2 else 0


def movement_frames(T):
    return conv_frames(conv_frames(T))


# ------------------------------------------------------------------------------------------ weights
def xavier(name, shape):
    rf = int(np.prod(shape[2:])) if len(shape) > 2 else 1
    std = math.sqrt(2.0 / ((shape[0] + shape[1]) * rf))
    return (std * syn.normal(SEED, name, shape)).astype(np.float32)


def small_vec(name, n, scale=0.02, base=0.0):
    return (base + scale * syn.normal(SEED, name, (n,))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def movement_state(C, hid, lat):
    t = f"eval/movement/{C}/{hid}/{lat}/"
    return {"main.0.weight": xavier(t + "c1", (hid, C, 4)), "main.0.bias": small_vec(t + "c1b", hid),
            "main.3.weight": xavier(t + "c2", (lat, hid, 4)), "main.3.bias": small_vec(t + "c2b", lat),
            "out_net.weight": xavier(t + "out", (lat, lat)), "out_net.bias": small_vec(t + "outb", lat)}


@functools.lru_cache(maxsize=None)
def recurrent_state(tag, in_size, H, out, word=0, pos=0):
    t = f"eval/{tag}/{in_size}/{H}/{out}/"
    sd = {}
    if word:
        sd["pos_emb.weight"], sd["pos_emb.bias"] = xavier(t + "pos", (word, pos)), small_vec(t + "posb", word)
    sd["input_emb.weight"], sd["input_emb.bias"] = xavier(t + "in", (H, in_size)), small_vec(t + "inb", H)
    k = 1.0 / math.sqrt(H)
    for r in ("", "_reverse"):
        sd[f"gru.weight_ih_l0{r}"] = syn.uniform(SEED, t + "wih" + r, (3 * H, H), -k, k)
        sd[f"gru.weight_hh_l0{r}"] = syn.uniform(SEED, t + "whh" + r, (3 * H, H), -k, k)
        sd[f"gru.bias_ih_l0{r}"] = syn.uniform(SEED, t + "bih" + r, (3 * H,), -k, k)
        sd[f"gru.bias_hh_l0{r}"] = syn.uniform(SEED, t + "bhh" + r, (3 * H,), -k, k)
    sd["output_net.0.weight"], sd["output_net.0.bias"] = xavier(t + "o0", (H, 2 * H)), small_vec(t + "o0b", H)
    sd["output_net.1.weight"], sd["output_net.1.bias"] = small_vec(t + "lng", H, 0.1, 1.0), small_vec(t + "lnb", H, 0.1)
    sd["output_net.3.weight"], sd["output_net.3.bias"] = xavier(t + "o3", (out, H)), small_vec(t + "o3b", out)
    sd["hidden"] = syn.normal(SEED, t + "hidden", (2, 1, H))
    return sd


def nets(dim_pose, sizes=None):
    """-> (movement, motion, text) state dicts, the reference's key names, float32."""
    s = sizes or (SMALL if dim_pose == SMALL_POSE else REAL)
    return (movement_state(dim_pose - 4, s["hid"], s["lat"]), recurrent_state("motion", s["lat"], s["Hm"], s["out"]),
            recurrent_state("text", s["word"], s["Ht"], s["out"], s["word"], s["pos"]))


# ------------------------------------------------------------------------------------------ inputs
def lengths_of(kind, B, T, unit, tag):
    """full: every clip T.  one: every clip one step (unit .. 2 unit - 1).  mixed: duplicates, the longest clip second, not first."""
    if kind == "full":
        return [T] * B
    if kind == "one":
        return [min(unit + b % unit, T) for b in range(B)]
    assert kind == "mixed"
    u = syn.uniform01(SEED, f"eval/len/{tag}", B)
    lens = [int(unit + math.floor(u[b] * (T - unit + 1))) for b in range(B)]
    lens[0] = max(unit, T // 2)
    for b in (1, 2):
        if b < B:
            lens[b] = T
    if B > 4:
        lens[4] = lens[3]
    return lens


def motion_case(name):
    """-> (dim_pose, motions [B, T, F] float32, m_lens list)."""
    F, B, T, kind = MOTION_CASES[name]
    return F, syn.normal(SEED, f"eval/motion/{name}", (B, T, F)), lengths_of(kind, B, T, 4, name)


def text_case(name, sizes=REAL):
    """-> (word_embs [B, L, W], pos_ohot [B, L, P] one-hot, cap_lens list)."""
    B, L, kind = TEXT_CASES[name]
    words = syn.normal(SEED, f"eval/words/{name}", (B, L, sizes["word"]))
    which = np.floor(syn.uniform01(SEED, f"eval/pos/{name}", B * L) * sizes["pos"]).astype(np.int64).reshape(B, L)
    return words, np.eye(sizes["pos"], dtype=np.float32)[which], lengths_of(kind, B, L, 1, "text/" + name)


def small_case(B):
    """The H = 64 sweep: B clips of SMALL_T frames whose step counts cycle through 1 .. 5, the longest not first."""
    lens = [4 * (1 + (b + 2) % 5) + (b % 4 if (b + 2) % 5 < 4 else 0) for b in range(B)]
    return SMALL_POSE, syn.normal(SEED, f"eval/small/{B}", (B, SMALL_T, SMALL_POSE)), lens


def fid_sets():
    """Two sets of FID_CLIPS small clips, the second shifted and scaled: 'generated' and 'real'."""
    gen = syn.normal(SEED, "eval/fid/gen", (FID_CLIPS, SMALL_T, SMALL_POSE))
    real = 0.2 + 1.2 * syn.normal(SEED, "eval/fid/real", (FID_CLIPS, SMALL_T, SMALL_POSE))
    lens = [4 * (1 + b % 5) for b in range(FID_CLIPS)]
    return gen, real.astype(np.float32), lens


def stat_embeddings():
    """-> (E1, E2) [STAT_N, STAT_D] float32: E2 a noisy copy of E1, both spread over six directions only, so that distances do not
    concentrate and top-1, top-2 and top-3 differ; asserted to keep every row's diagonal distance 1e-4 (relative) clear of the row's
    other entries."""
    z1 = syn.normal(SEED, "eval/stat/z1", (STAT_N, 6)).astype(np.float64)
    z2 = z1 + 0.8 * syn.normal(SEED, "eval/stat/z2", (STAT_N, 6))
    span = syn.normal(SEED, "eval/stat/span", (6, STAT_D)).astype(np.float64)
    e1, e2 = (z1 @ span).astype(np.float32), (z2 @ span).astype(np.float32)
    assert_rank_margin(e1, e2)
    return e1, e2


def assert_rank_margin(e1, e2, margin=1e-4):
    d = euclidean_distance_matrix(e1, e2, np.float64)
    diag = np.diag(d)[:, None]
    gap = np.abs(d - diag) / diag
    gap[np.arange(len(d)), np.arange(len(d))] = np.inf
    assert gap.min() >= margin, gap.min()


def frechet_sets():
    """Two seeded float64 activation sets [300, 24] for the host Frechet path."""
    a = syn.normal(SEED, "eval/frechet/a", (300, 24)).astype(np.float64)
    b = 0.3 + 1.1 * syn.normal(SEED, "eval/frechet/b", (300, 24)).astype(np.float64)
    return a, b


def multimodal_embeddings():
    return syn.normal(SEED, "eval/stat/mm", (MM_SENTS, MM_PER, STAT_D))


# ------------------------------------------------------------------------------------------ the modules
def leaky(x):
    return np.where(x > 0, x, x.dtype.type(0.2) * x)


def linear(x, w, b, dtype):
    return x @ np.asarray(w, dtype).T + np.asarray(b, dtype)


def conv_k4s2p1(x, w, b, dtype):
    """Conv1d(C, O, 4, 2, 1) over x [B, T, C]: output frame t reads frames 2 t - 1 .. 2 t + 2, zeros outside."""
    B, T, C = x.shape
    To = conv_frames(T)
    xp = np.zeros((B, T + 2, C), dtype)
    xp[:, 1:-1] = x
    idx = 2 * np.arange(To)[:, None] + np.arange(4)[None]
    win = xp[:, idx]                                                   # [B, To, 4, C]
    wk = np.asarray(w, dtype).transpose(0, 2, 1).reshape(w.shape[0], 4 * C)
    return (win.reshape(B * To, 4 * C) @ wk.T).reshape(B, To, -1) + np.asarray(b, dtype)


def movement(sd, motions, dtype):
    """MovementConvEncoder on motions[..., :-4] -> [B, T2, lat]."""
    x = np.asarray(motions, dtype)[..., :-4]
    x = leaky(conv_k4s2p1(x, sd["main.0.weight"], sd["main.0.bias"], dtype))
    x = leaky(conv_k4s2p1(x, sd["main.3.weight"], sd["main.3.bias"], dtype))
    return linear(x, sd["out_net.weight"], sd["out_net.bias"], dtype)


def sigmoid(x):
    return x.dtype.type(1) / (x.dtype.type(1) + np.exp(-x))


def gru_last(sd, x, steps, dtype):
    """torch's bidirectional GRU over packed sequences: x [B, L, H], steps [B] -> [B, 2 H] (forward's final state, then backward's)."""
    proj = [x @ np.asarray(sd[f"gru.weight_ih_l0{r}"], dtype).T + np.asarray(sd[f"gru.bias_ih_l0{r}"], dtype) for r in ("", "_reverse")]
    return gru_last_projected(sd, proj, steps, dtype)


def gru_last_projected(sd, proj, steps, dtype):
    """The recurrence of `gru_last` on given input projections: proj[direction] [B, L, 3 H] = W_ih x + b_ih (gates r, z, n).  A position
    that no step of its clip reaches is never read."""
    B, L, H = proj[0].shape[0], proj[0].shape[1], proj[0].shape[2] // 3
    steps = np.asarray(steps, np.int64)
    out = []
    for d, r in enumerate(("", "_reverse")):
        whh, bhh = np.asarray(sd[f"gru.weight_hh_l0{r}"], dtype), np.asarray(sd[f"gru.bias_hh_l0{r}"], dtype)
        gi_all = np.asarray(proj[d], dtype)
        h = np.repeat(np.asarray(sd["hidden"], dtype)[d], B, 0)
        for s in range(int(steps.max())):
            act = np.nonzero(steps > s)[0]
            pos = s if d == 0 else steps[act] - 1 - s
            gi = gi_all[act, pos]
            gh = h[act] @ whh.T + bhh
            rg = sigmoid(gi[:, :H] + gh[:, :H])
            zg = sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
            ng = np.tanh(gi[:, 2 * H:] + rg * gh[:, 2 * H:])
            h[act] = (dtype(1) - zg) * ng + zg * h[act]
        out.append(h)
    return np.concatenate(out, -1)


def output_net(sd, x, dtype):
    y = linear(x, sd["output_net.0.weight"], sd["output_net.0.bias"], dtype)
    mean = y.mean(-1, keepdims=True)
    var = ((y - mean) ** 2).mean(-1, keepdims=True)
    y = (y - mean) / np.sqrt(var + dtype(1e-5)) * np.asarray(sd["output_net.1.weight"], dtype) + np.asarray(sd["output_net.1.bias"], dtype)
    return linear(leaky(y), sd["output_net.3.weight"], sd["output_net.3.bias"], dtype)


def embed_motions(net, motions, m_lens, dtype, unit=4, parts=None):
    """Input order.  parts (a dict): receives the movement features."""
    mv, mo, _ = net
    feats = movement(mv, motions, dtype)
    if parts is not None:
        parts["movement"] = feats
    steps = np.asarray(m_lens, np.int64) // unit
    emb = linear(feats, mo["input_emb.weight"], mo["input_emb.bias"], dtype)
    return output_net(mo, gru_last(mo, emb, steps, dtype), dtype)


def embed_text(net, words, pos_ohot, cap_lens, dtype):
    tx = net[2]
    inputs = np.asarray(words, dtype) + linear(np.asarray(pos_ohot, dtype), tx["pos_emb.weight"], tx["pos_emb.bias"], dtype)
    emb = linear(inputs, tx["input_emb.weight"], tx["input_emb.bias"], dtype)
    return output_net(tx, gru_last(tx, emb, cap_lens, dtype), dtype)


def align_index(m_lens):
    return np.argsort(list(m_lens))[::-1].copy()


# ------------------------------------------------------------------------------------------ the statistics
def euclidean_distance_matrix(m1, m2, dtype):
    m1, m2 = np.asarray(m1, dtype), np.asarray(m2, dtype)
    return np.sqrt(-2 * (m1 @ m2.T) + np.square(m1).sum(1, keepdims=True) + np.square(m2).sum(1))


def diagonal_ranks(m1, m2, dtype):
    """Entries strictly below the diagonal one, per row; a NaN entry is not below anything (numpy's `<`), and a row whose diagonal
    distance is not finite ranks last: N2, in no top-k."""
    with np.errstate(invalid="ignore"):
        d = euclidean_distance_matrix(m1, m2, dtype)
        diag = np.diag(d)
        below = (d < diag[:, None]).sum(1)
    return np.where(np.isfinite(diag), below, d.shape[1])


def r_precision(m1, m2, top_k, dtype):
    order = np.argsort(euclidean_distance_matrix(m1, m2, dtype), axis=1)
    hit = order[:, :top_k] == np.arange(len(order))[:, None]
    return np.cumsum(hit, 1) > 0


def matching_score(m1, m2, dtype):
    return np.linalg.norm(np.asarray(m1, dtype) - np.asarray(m2, dtype), axis=1)


def diversity(act, times, dtype):
    act = np.asarray(act, dtype)
    first = np.random.choice(act.shape[0], times, replace=False)
    second = np.random.choice(act.shape[0], times, replace=False)
    return np.linalg.norm(act[first] - act[second], axis=1).mean()


def multimodality(act, times, dtype):
    act = np.asarray(act, dtype)
    first = np.random.choice(act.shape[1], times, replace=False)
    second = np.random.choice(act.shape[1], times, replace=False)
    return np.linalg.norm(act[:, first] - act[:, second], axis=2).mean()


def statistics(act):
    act = np.asarray(act)
    return np.mean(act, axis=0), np.cov(act, rowvar=False)


def frechet(mu1, s1, mu2, s2):
    from scipy import linalg
    mu1, mu2 = np.asarray(mu1), np.asarray(mu2)                  # a float32 mean stays float32 through diff.dot(diff), as in the reference
    s1, s2 = np.asarray(s1, np.float64), np.asarray(s2, np.float64)
    root = linalg.sqrtm(s1 @ s2)
    assert np.isfinite(root).all()
    if np.iscomplexobj(root):
        assert np.allclose(np.diagonal(root).imag, 0, atol=1e-3)
        root = root.real
    return float((mu1 - mu2) @ (mu1 - mu2) + np.trace(s1) + np.trace(s2) - 2 * np.trace(root))


def fid(gen, real):
    return frechet(*statistics(gen), *statistics(real))
