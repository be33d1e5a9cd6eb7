"""Golden vectors of CLIP's text tower -> tests/golden/clip_text.npz, and of its tokenizer -> tests/golden/clip_toy_merges.txt +
tests/golden/clip_tokens.npz.

Runs only where `transformers` is installed, on the CPU, offline (TRANSFORMERS_OFFLINE=1: the model is built from a config, nothing is
fetched):

    python tests/golden/make_golden_clip_text.py

The oracle is Hugging Face's CLIPTextModelWithProjection (hidden_act="quick_gelu", eos_token_id=2 so that the pooled row is
argmax(input_ids), as in OpenAI CLIP), an implementation independent of this package, loaded with tests/clip_text_fixture.py's seeded
weights under Hugging Face names.  Every input is rebuilt by the tests from the seed; per case (clip_text_fixture.CASES) only these are
stored:

  <case>|f64   the float64 module's output [prompts, 512]
  <case>|d32   per prompt, max |fp32 module - f64| / max |f64|
  <case>|d16   per prompt, the same for the fp16 module: the arithmetic the reference runs in after clip.model.convert_weights

Tokenizer: the toy merges file (a header line and clip_text_fixture.TOY_MERGES, data only) and the ids of TOY_STRINGS at context 77,
the last one over-long and truncated.  The ids are hand-derivable from the vocabulary rule (256 byte symbols, the same with </w>, the
merges, the two specials); HAND below derives three of them by hand, and the script asserts them.  transformers' CLIPTokenizer is built
offline from the same toy vocabulary when it can be, and then the stored ids are asserted to equal its ids too (`tokens|source` says
which: "transformers" or "hand-checked rule only")."""
import json
import os
import sys
import tempfile

os.environ.setdefault("TRANSFORMERS_OFFLINE", "1")
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clip_text_fixture as cf  # noqa: E402
import mst_amd  # noqa: E402,F401
from mst_amd.model.clip_text import SimpleTokenizer, bytes_to_unicode  # noqa: E402

MERGES = os.path.join(HERE, "clip_toy_merges.txt")


def build(layers, dtype):
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    cfg = CLIPTextConfig(vocab_size=cf.VOCAB, hidden_size=cf.WIDTH, intermediate_size=cf.FFN, projection_dim=cf.WIDTH,
                         num_hidden_layers=layers, num_attention_heads=cf.HEADS, max_position_embeddings=cf.CONTEXT,
                         hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=2, bos_token_id=0, pad_token_id=1,
                         attn_implementation="sdpa")       # the eager path takes its softmax in fp32 whatever the module's dtype
    model = CLIPTextModelWithProjection(cfg).eval()
    sd = {k: torch.from_numpy(v) for k, v in cf.to_hf(cf.state_dict(layers)).items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    return model.to(dtype)


def towers():
    out = {}
    for case, (layers, _, ends) in cf.CASES.items():
        ids = torch.from_numpy(cf.case_ids(case))
        with torch.no_grad():
            y = {name: build(layers, dt)(input_ids=ids).text_embeds.double().numpy()
                 for name, dt in (("f64", torch.float64), ("f32", torch.float32), ("f16", torch.float16))}
            other = build(layers, torch.float64)(input_ids=torch.from_numpy(cf.case_ids(case, tail="ids"))).text_embeds.numpy()
        assert np.array_equal(other, y["f64"]), "tokens behind end-of-text changed the oracle's output"
        assert np.isfinite(y["f16"]).all()
        out[case + "|f64"] = y["f64"]
        out[case + "|d32"] = cf.distance(y["f32"], y["f64"])
        out[case + "|d16"] = cf.distance(y["f16"], y["f64"])
        mine = cf.distance(cf.forward64(cf.state_dict(layers), ids.numpy()), y["f64"])
        print(f"{case}: ends {ends} d32 {out[case + '|d32'].max():.2e} d16 {out[case + '|d16'].min():.2e}..{out[case + '|d16'].max():.2e} "
              f"numpy f64 statement {mine.max():.2e}")
    return out


def toy_vocab():
    sym = list(bytes_to_unicode().values())
    return sym + [s + "</w>" for s in sym] + ["".join(m.split()) for m in cf.TOY_MERGES] + ["<|startoftext|>", "<|endoftext|>"]


def hand():
    """Three strings by hand.  Ids: byte symbol c -> index of c in the byte table ('!' = 0, so a letter is ord - 33), c</w> -> 256 + that,
    merge k (0-based line of TOY_MERGES) -> 512 + k, start 512 + len(merges), end one more."""
    m = {"".join(x.split()): 512 + k for k, x in enumerate(cf.TOY_MERGES)}
    sot = 512 + len(cf.TOY_MERGES)
    eot = sot + 1
    c = lambda ch: ord(ch) - 33
    e = lambda ch: 256 + ord(ch) - 33
    return {
        # t h e</w>: (t, h) is merge 0 -> th e</w>; (th, e</w>) is merge 1 -> the</w>
        "the the the": [sot, m["the</w>"], m["the</w>"], m["the</w>"], eot],
        # one letter is its own end-of-word symbol
        "x": [sot, e("x"), eot],
        # lower-cased.  a -> a</w>.  p e r s o n</w>: (e, r) -> er, (p, er) -> per, (o, n</w>) -> on</w> ("o n" does not apply to n</w>),
        # (s, on</w>) -> son</w>, (per, son</w>) -> person</w>.  w a l k s</w>: (w, a) -> wa, (l, k) -> lk, (wa, lk) -> walk,
        # (walk, s</w>) -> walks</w>
        "A Person WALKS": [sot, e("a"), m["person</w>"], m["walks</w>"], eot],
    }


def tokens():
    with open(MERGES, "w") as fh:
        fh.write("#version: 0.2\n" + "\n".join(cf.TOY_MERGES) + "\n")
    tok = SimpleTokenizer(MERGES)
    vocab = toy_vocab()
    assert [tok.decoder[i] for i in range(len(vocab))] == vocab
    ids = tok.tokenize(cf.TOY_STRINGS, context_length=77, truncate=True).numpy()
    for s, want in hand().items():
        row = ids[cf.TOY_STRINGS.index(s)]
        assert row[:len(want)].tolist() == want and not row[len(want):].any(), (s, row[:12], want)
    assert ids[-1, 76] == len(vocab) - 1 and ids[-1].min() > 0, "the over-long string must be cut with end-of-text last"
    source = "hand-checked rule only"
    try:
        from transformers import CLIPTokenizer
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "vocab.json"), "w") as fh:
                json.dump({v: i for i, v in enumerate(vocab)}, fh)
            with open(os.path.join(d, "merges.txt"), "w") as fh:
                fh.write("#version: 0.2\n" + "\n".join(cf.TOY_MERGES) + "\n")
            hf = CLIPTokenizer(os.path.join(d, "vocab.json"), os.path.join(d, "merges.txt"))
            theirs = np.zeros_like(ids)
            for r, s in enumerate(cf.TOY_STRINGS):
                row = hf(s)["input_ids"]
                if len(row) > 77:
                    row = row[:77]
                    row[-1] = len(vocab) - 1
                theirs[r, :len(row)] = row
        bad = [cf.TOY_STRINGS[r] for r in range(len(ids)) if not np.array_equal(ids[r], theirs[r])]
        assert not bad, f"SimpleTokenizer and transformers' CLIPTokenizer disagree on {bad}"
        source = "transformers"
    except (ImportError, OSError) as e:
        print("transformers' CLIPTokenizer could not be built:", e)
    print("tokenizer golden source:", source)
    return ids, source


def main():
    if "--tokens-only" not in sys.argv:
        np.savez_compressed(os.path.join(HERE, "clip_text.npz"), **towers())
    ids, source = tokens()
    np.savez_compressed(os.path.join(HERE, "clip_tokens.npz"), ids=ids, source=np.array(source))


if __name__ == "__main__":
    main()
