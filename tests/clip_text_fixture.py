"""Shared by tests/golden/make_golden_clip_text.py, tests/test_clip_text_cpu.py and tests/test_gpu_clip_text.py: seeded weights of a
CLIP text tower in the OpenAI key layout (every value f16-representable, as the published checkpoints are), seeded token rows with the
end-of-text token at a chosen position, the same weights under Hugging Face names, and a float64 numpy statement of the tower.

Scales (what a trained tower looks like): LayerNorm gains 1 + 0.1 n, matrices n / sqrt(fan_in), embeddings 0.5 n (token) and 0.25 n
(position), and three residual channels (OUTLIERS) 20 x larger in both embeddings and fed +-3 by every out-proj / FFN bias, so they stay
10 - 30 x above the rest through 2 and through 12 layers."""
import numpy as np

from conftest import SEED
from mst_amd import synthetic as syn

VOCAB, WIDTH, HEADS, FFN, CONTEXT = 1024, 512, 8, 2048, 77
EOT, SOT = VOCAB - 1, VOCAB - 2
OUTLIERS = (5, 133, 301)
# case -> (layers, context the ids are built at (zero-padded to 77), end-of-text positions)
CASES = {"l2": (2, 77, (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 76)),
         "l12": (12, 77, (7, 21, 76)),
         "c22": (2, 22, (3, 11, 21))}


def _f16(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


def state_dict(layers, seed=SEED):
    """OpenAI-layout state dict, float32 numpy holding f16-representable values."""
    n = lambda name, shape: syn.normal(seed, "clip/" + name, shape).astype(np.float64)
    sd = {}
    tok, pos = 0.5 * n("tok", (VOCAB, WIDTH)), 0.25 * n("pos", (CONTEXT, WIDTH))
    for c in OUTLIERS:
        tok[:, c] *= 20.0
        pos[:, c] *= 20.0
    sd["token_embedding.weight"], sd["positional_embedding"] = tok, pos
    for i in range(layers):
        p = f"transformer.resblocks.{i}."
        for ln in ("ln_1", "ln_2"):
            sd[p + ln + ".weight"] = 1.0 + 0.1 * n(f"{i}/{ln}/g", (WIDTH,))
            sd[p + ln + ".bias"] = 0.05 * n(f"{i}/{ln}/b", (WIDTH,))
        sd[p + "attn.in_proj_weight"] = n(f"{i}/wqkv", (3 * WIDTH, WIDTH)) / np.sqrt(WIDTH)
        sd[p + "attn.in_proj_bias"] = 0.02 * n(f"{i}/bqkv", (3 * WIDTH,))
        sd[p + "attn.out_proj.weight"] = n(f"{i}/wo", (WIDTH, WIDTH)) / np.sqrt(WIDTH)
        sd[p + "mlp.c_fc.weight"] = n(f"{i}/w1", (FFN, WIDTH)) / np.sqrt(WIDTH)
        sd[p + "mlp.c_fc.bias"] = 0.02 * n(f"{i}/b1", (FFN,))
        sd[p + "mlp.c_proj.weight"] = n(f"{i}/w2", (WIDTH, FFN)) / np.sqrt(FFN)
        bo, b2 = 0.02 * n(f"{i}/bo", (WIDTH,)), 0.02 * n(f"{i}/b2", (WIDTH,))
        for k, c in enumerate(OUTLIERS):
            bo[c] = 3.0 * (-1.0) ** k
            b2[c] = 3.0 * (-1.0) ** k
        sd[p + "attn.out_proj.bias"], sd[p + "mlp.c_proj.bias"] = bo, b2
    sd["ln_final.weight"] = 1.0 + 0.1 * n("lnf/g", (WIDTH,))
    sd["ln_final.bias"] = 0.05 * n("lnf/b", (WIDTH,))
    sd["text_projection"] = n("proj", (WIDTH, WIDTH)) / np.sqrt(WIDTH)
    return {k: _f16(v) for k, v in sd.items()}


def to_hf(sd):
    """The same tensors under Hugging Face's CLIPTextModelWithProjection names."""
    out = {"text_model.embeddings.token_embedding.weight": sd["token_embedding.weight"],
           "text_model.embeddings.position_embedding.weight": sd["positional_embedding"],
           "text_model.final_layer_norm.weight": sd["ln_final.weight"], "text_model.final_layer_norm.bias": sd["ln_final.bias"],
           "text_projection.weight": np.ascontiguousarray(sd["text_projection"].T)}
    i = 0
    while f"transformer.resblocks.{i}.ln_1.weight" in sd:
        p, q = f"transformer.resblocks.{i}.", f"text_model.encoder.layers.{i}."
        w, b = sd[p + "attn.in_proj_weight"], sd[p + "attn.in_proj_bias"]
        for k, name in enumerate(("q_proj", "k_proj", "v_proj")):
            out[q + f"self_attn.{name}.weight"] = np.ascontiguousarray(w[k * WIDTH:(k + 1) * WIDTH])
            out[q + f"self_attn.{name}.bias"] = np.ascontiguousarray(b[k * WIDTH:(k + 1) * WIDTH])
        for a, c in (("attn.out_proj", "self_attn.out_proj"), ("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"), ("mlp.c_fc", "mlp.fc1"),
                     ("mlp.c_proj", "mlp.fc2")):
            out[q + c + ".weight"], out[q + c + ".bias"] = sd[p + a + ".weight"], sd[p + a + ".bias"]
        i += 1
    return out


def token_row(case, k, e, context=CONTEXT, tail="zeros", seed=SEED):
    """int64 [context]: start-of-text, e - 1 seeded ids below SOT, end-of-text at position e, then zeros -- or, tail="ids", seeded ids
    below the end-of-text id, which nothing may depend on."""
    u = syn.uniform01(seed, f"clip/ids/{case}/{k}", CONTEXT)
    row = np.zeros(context, dtype=np.int64)
    row[0] = SOT
    row[1:e] = (u[1:e] * SOT).astype(np.int64)
    row[e] = EOT
    if tail == "ids":
        v = syn.uniform01(seed, f"clip/tail/{case}/{k}", CONTEXT)
        row[e + 1:] = (v[e + 1:context] * EOT).astype(np.int64)
    return row


def case_ids(case, tail="zeros"):
    """int64 [prompts, 77] of a case: built at the case's context, zero-padded to 77."""
    _, ctx, ends = CASES[case]
    out = np.zeros((len(ends), CONTEXT), dtype=np.int64)
    for k, e in enumerate(ends):
        out[k, :ctx] = token_row(case, k, e, ctx, tail)
    return out


def _ln(x, g, b):
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    return (x - m) / np.sqrt(v + 1e-5) * g + b


def forward64(sd, ids):
    """The tower in float64 over the live rows of every prompt: [B, 512]."""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
    layers = 0
    while f"transformer.resblocks.{layers}.ln_1.weight" in w:
        layers += 1
    out = np.zeros((len(ids), WIDTH))
    for r, row in enumerate(np.asarray(ids)):
        e = int(np.argmax(row))
        x = w["token_embedding.weight"][row[:e + 1]] + w["positional_embedding"][:e + 1]
        causal = np.tril(np.ones((e + 1, e + 1), dtype=bool))
        for i in range(layers):
            p = f"transformer.resblocks.{i}."
            h = _ln(x, w[p + "ln_1.weight"], w[p + "ln_1.bias"])
            qkv = h @ w[p + "attn.in_proj_weight"].T + w[p + "attn.in_proj_bias"]
            q, k, v = (qkv[:, j * WIDTH:(j + 1) * WIDTH].reshape(e + 1, HEADS, 64).transpose(1, 0, 2) for j in range(3))
            s = np.where(causal, q @ k.transpose(0, 2, 1) / 8.0, -np.inf)
            pr = np.exp(s - s.max(-1, keepdims=True))
            pr /= pr.sum(-1, keepdims=True)
            o = (pr @ v).transpose(1, 0, 2).reshape(e + 1, WIDTH)
            x = x + o @ w[p + "attn.out_proj.weight"].T + w[p + "attn.out_proj.bias"]
            h = _ln(x, w[p + "ln_2.weight"], w[p + "ln_2.bias"])
            u = h @ w[p + "mlp.c_fc.weight"].T + w[p + "mlp.c_fc.bias"]
            x = x + (u / (1.0 + np.exp(-1.702 * u))) @ w[p + "mlp.c_proj.weight"].T + w[p + "mlp.c_proj.bias"]
        out[r] = _ln(x[e], w["ln_final.weight"], w["ln_final.bias"]) @ w["text_projection"]
    return out


def distance(got, ref):
    """Per prompt: max |got - ref| over max |ref|."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(got - ref).max(-1) / np.abs(ref).max(-1)


# ---- the toy vocabulary of the tokenizer golden (tests/golden/clip_toy_merges.txt) and its strings
TOY_MERGES = ["t h", "th e</w>", "i n", "e r", "o n", "a n", "w a", "l k", "wa lk", "walk s</w>", "p er", "o n</w>", "s on</w>",
              "per son</w>", "an d</w>", "r u", "ru n", "run s</w>", "j u", "ju m", "jum p", "jump s</w>", "in g</w>", "walk ing</w>",
              "' s</w>", "' t</w>", "d on", "don 't</w>", "! !", "!! !</w>", "o l", "ol d</w>", "a n</w>", "m an</w>", "g o", "c a", "ca f",
              "p r", "o u", "pr ou", "d l", "l y</w>"]
TOY_STRINGS = ["a person walks proudly", "A Person WALKS", "the man runs and jumps", "don't walk", "the man's walking", "it's 12 o'clock",
               "walks 3 times, then 42", "stop!!! now", "wow... ok?!", "  the   old\tman \n jumps  ", "café walking", "über runs",
               "a person is walking and running and jumping", "he'll they've i'm she'd we're", "walk-ing in", "<|startoftext|> the",
               "the the the", "", "x", " ".join(["the man walks and runs and jumps"] * 16)]       # the last: > 77 tokens, truncated
