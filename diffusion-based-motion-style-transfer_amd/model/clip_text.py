"""CLIP's text tower on the GPU (csrc/mst_clip.h) and CLIP's byte-level BPE tokenizer: the native way from `y['text']` to the
[B, 512] embedding `MDM.encode_text` needs.  Replaces `clip.load` / `clip.tokenize` / `clip_model.encode_text` of
model/mdm_forstyledataset.py's `encode_text` for the ViT-B/32 and ViT-B/16 text towers (width 512, 8 heads, FFN 2048, any layer
count, context <= 77).  Nothing is bundled: the checkpoint and the merges file are the user's own.

    enc = ClipTextEncoder.from_file("ViT-B-32.pt", device)          # torch.jit archive, torch.save dict or .safetensors
    enc.tokenizer = SimpleTokenizer("bpe_simple_vocab_16e6.txt.gz") # or a model directory's merges.txt
    emb = enc(["a person walks proudly"])                           # float32 [1, 512] on the device
    model.use_native_text_encoder("ViT-B-32.pt", "merges.txt")      # the same, hooked into encode_text

Only the rows up to a prompt's end-of-text token are computed (causality: nothing behind it can reach its embedding), packed over the
batch.  A prompt's embedding is the same bits alone, anywhere in any batch, whatever lies behind its end-of-text token, on any stream.
There is no fallback: without the HIP library every call raises."""
import ctypes as C
import gzip
import html
import os
import unicodedata

import numpy as np
import torch

from .. import _native

WIDTH, HEADS, FFN, MAX_CONTEXT = 512, 8, 2048, 77
F16_MAX = 65504.0
LAYER_FIELDS = ("ln1_g", "ln1_b", "wqkv", "bqkv", "wo", "bo", "ln2_g", "ln2_b", "w1", "b1", "w2", "b2")
PACKED = ("wqkv", "wo", "w1", "w2")


# ------------------------------------------------------------------------------------------------------------------ state dicts
def _openai_table(sd):
    n = 0
    while f"transformer.resblocks.{n}.ln_1.weight" in sd:
        n += 1
    t = {"tok_emb": sd["token_embedding.weight"], "pos_emb": sd["positional_embedding"], "lnf_g": sd["ln_final.weight"],
         "lnf_b": sd["ln_final.bias"], "proj": sd["text_projection"], "layers": []}
    for i in range(n):
        p = f"transformer.resblocks.{i}."
        t["layers"].append({
            "ln1_g": sd[p + "ln_1.weight"], "ln1_b": sd[p + "ln_1.bias"],
            "wqkv": sd[p + "attn.in_proj_weight"], "bqkv": sd[p + "attn.in_proj_bias"],
            "wo": sd[p + "attn.out_proj.weight"], "bo": sd[p + "attn.out_proj.bias"],
            "ln2_g": sd[p + "ln_2.weight"], "ln2_b": sd[p + "ln_2.bias"],
            "w1": sd[p + "mlp.c_fc.weight"], "b1": sd[p + "mlp.c_fc.bias"],
            "w2": sd[p + "mlp.c_proj.weight"], "b2": sd[p + "mlp.c_proj.bias"]})
    return t


def _hf_table(sd):
    n = 0
    while f"text_model.encoder.layers.{n}.layer_norm1.weight" in sd:
        n += 1
    t = {"tok_emb": sd["text_model.embeddings.token_embedding.weight"], "pos_emb": sd["text_model.embeddings.position_embedding.weight"],
         "lnf_g": sd["text_model.final_layer_norm.weight"], "lnf_b": sd["text_model.final_layer_norm.bias"],
         "proj": sd["text_projection.weight"].t(), "layers": []}
    for i in range(n):
        p = f"text_model.encoder.layers.{i}."
        a = p + "self_attn."
        t["layers"].append({
            "ln1_g": sd[p + "layer_norm1.weight"], "ln1_b": sd[p + "layer_norm1.bias"],
            "wqkv": torch.cat([sd[a + "q_proj.weight"], sd[a + "k_proj.weight"], sd[a + "v_proj.weight"]], 0),
            "bqkv": torch.cat([sd[a + "q_proj.bias"], sd[a + "k_proj.bias"], sd[a + "v_proj.bias"]], 0),
            "wo": sd[a + "out_proj.weight"], "bo": sd[a + "out_proj.bias"],
            "ln2_g": sd[p + "layer_norm2.weight"], "ln2_b": sd[p + "layer_norm2.bias"],
            "w1": sd[p + "mlp.fc1.weight"], "b1": sd[p + "mlp.fc1.bias"],
            "w2": sd[p + "mlp.fc2.weight"], "b2": sd[p + "mlp.fc2.bias"]})
    return t


def weight_table(sd):
    """One table from either key layout (OpenAI `transformer.resblocks.N...` / Hugging Face `text_model...`), on the CPU, every tensor
    contiguous float32 holding f16-representable magnitudes: {"tok_emb" [V, 512], "pos_emb" [C, 512], "lnf_g", "lnf_b", "proj" [512 in,
    512 out], "layers": [{ln1_g, ln1_b, wqkv [1536, 512] (rows q | k | v), bqkv, wo, bo, ln2_g, ln2_b, w1, b1, w2, b2}]}.  Raises
    ValueError naming what it refuses: an unknown layout, a tower that is not 512 / 8 / 2048, a context above 77, a tensor whose largest
    magnitude overflows f16."""
    sd = {k: (v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))) for k, v in sd.items()}
    if "token_embedding.weight" in sd:
        t = _openai_table(sd)
    elif "text_model.embeddings.token_embedding.weight" in sd:
        t = _hf_table(sd)
    else:
        raise ValueError("clip_text: neither 'token_embedding.weight' (OpenAI layout) nor 'text_model.embeddings.token_embedding.weight' "
                         "(Hugging Face layout) is in the state dict")
    if not t["layers"]:
        raise ValueError("clip_text: the state dict holds no transformer layer")
    width = int(t["tok_emb"].shape[1])
    if width != WIDTH:
        raise ValueError(f"clip_text: width {width}: only the {WIDTH}-wide text tower (ViT-B/32, ViT-B/16) is built")
    ffn = int(t["layers"][0]["w1"].shape[0])
    if ffn != FFN:
        raise ValueError(f"clip_text: ffn {ffn}: only the {FFN}-wide FFN is built")
    if int(t["pos_emb"].shape[0]) > MAX_CONTEXT:
        raise ValueError(f"clip_text: context {int(t['pos_emb'].shape[0])} above {MAX_CONTEXT}")
    want = {"wqkv": (3 * WIDTH, WIDTH), "bqkv": (3 * WIDTH,), "wo": (WIDTH, WIDTH), "bo": (WIDTH,), "w1": (FFN, WIDTH), "b1": (FFN,),
            "w2": (WIDTH, FFN), "b2": (WIDTH,), "ln1_g": (WIDTH,), "ln1_b": (WIDTH,), "ln2_g": (WIDTH,), "ln2_b": (WIDTH,)}

    def fit(name, v, shape=None):
        v = v.detach().to("cpu", torch.float32).contiguous()
        if shape is not None and tuple(v.shape) != shape:
            raise ValueError(f"clip_text: {name} has shape {tuple(v.shape)}, expected {shape}")
        if not bool(torch.isfinite(v).all()) or float(v.abs().max()) > F16_MAX:
            raise ValueError(f"clip_text: {name} does not fit f16 without overflow (largest magnitude {float(v.abs().max()):.6g})")
        return v

    out = {"tok_emb": fit("tok_emb", t["tok_emb"]), "pos_emb": fit("pos_emb", t["pos_emb"]), "lnf_g": fit("lnf_g", t["lnf_g"], (WIDTH,)),
           "lnf_b": fit("lnf_b", t["lnf_b"], (WIDTH,)), "proj": fit("proj", t["proj"], (WIDTH, WIDTH)), "layers": []}
    for i, layer in enumerate(t["layers"]):
        out["layers"].append({k: fit(f"layers.{i}.{k}", layer[k], want[k]) for k in LAYER_FIELDS})
    return out


# ------------------------------------------------------------------------------------------------------------------ tokenizer
def bytes_to_unicode():
    """Byte -> printable unicode character: the printable latin-1 bytes map to themselves, the others to 256, 257, ... in byte order."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, [chr(c) for c in cs]))


SOT, EOT = "<|startoftext|>", "<|endoftext|>"
_CONTRACTIONS = ("'s", "'t", "'re", "'ve", "'m", "'ll", "'d")


def _kind(ch):
    if ch.isspace():
        return "s"
    c = unicodedata.category(ch)[0]
    return "L" if c == "L" else "N" if c == "N" else "o"


def split_words(text):
    """CLIP's pattern <|startoftext|> | <|endoftext|> | 's 't 're 've 'm 'll 'd | letters+ | one digit | (non-space, non-letter,
    non-digit)+ as a scanner over unicodedata categories; alternatives in that order at every position, runs greedy."""
    out, i, n = [], 0, len(text)
    while i < n:
        ch = text[i]
        kind = _kind(ch)
        if kind == "s":
            i += 1
            continue
        hit = next((s for s in (SOT, EOT) + _CONTRACTIONS if text.startswith(s, i)), None)
        if hit is not None:
            out.append(hit)
            i += len(hit)
        elif kind == "N":
            out.append(ch)
            i += 1
        else:
            j = i + 1
            while j < n and _kind(text[j]) == kind:
                j += 1
            out.append(text[i:j])
            i = j
    return out


class SimpleTokenizer:
    """CLIP's byte-level BPE over the user's own merges file (bpe_simple_vocab_16e6.txt.gz of the `clip` package, or the merges.txt of
    a CLIP model directory; gzipped or plain).  Vocabulary: the 256 byte symbols, the same with '</w>', the merges in file order, then
    <|startoftext|> and <|endoftext|>.  No ftfy clean-up."""

    def __init__(self, bpe_path):
        with open(bpe_path, "rb") as fh:
            raw = fh.read()
        if raw[:2] == b"\x1f\x8b":
            raw = gzip.decompress(raw)
        lines = raw.decode("utf-8").split("\n")[1:49152 - 256 - 2 + 1]          # line 1 is a header; the published file has more lines than merges
        merges = [tuple(l.split()) for l in lines if len(l.split()) == 2]
        self.byte_encoder = bytes_to_unicode()
        vocab = list(self.byte_encoder.values())
        vocab = vocab + [v + "</w>" for v in vocab] + ["".join(m) for m in merges] + [SOT, EOT]
        self.encoder = {v: i for i, v in enumerate(vocab)}
        self.decoder = {i: v for v, i in self.encoder.items()}
        self.ranks = {m: i for i, m in enumerate(merges)}
        self.cache = {SOT: SOT, EOT: EOT}
        self.sot, self.eot = self.encoder[SOT], self.encoder[EOT]

    @property
    def vocab_size(self):
        return len(self.encoder)

    def bpe(self, token):
        if token in self.cache:
            return self.cache[token]
        word = tuple(token[:-1]) + (token[-1] + "</w>",)
        while len(word) > 1:
            pairs = {(word[k], word[k + 1]) for k in range(len(word) - 1)}
            best = min(pairs, key=lambda p: self.ranks.get(p, float("inf")))
            if best not in self.ranks:
                break
            a, b = best
            new, k = [], 0
            while k < len(word):
                if k < len(word) - 1 and word[k] == a and word[k + 1] == b:
                    new.append(a + b)
                    k += 2
                else:
                    new.append(word[k])
                    k += 1
            word = tuple(new)
        out = " ".join(word)
        self.cache[token] = out
        return out

    def encode(self, text):
        text = " ".join(html.unescape(html.unescape(text)).split()).lower()
        ids = []
        for w in split_words(text):
            sym = "".join(self.byte_encoder[b] for b in w.encode("utf-8"))
            ids.extend(self.encoder[s] for s in self.bpe(sym).split(" "))
        return ids

    def tokenize(self, texts, context_length=77, truncate=True):
        """int64 [len(texts), context_length]: start-of-text, the prompt, end-of-text, zeros.  A prompt that does not fit is cut and its
        last kept position becomes end-of-text (truncate=False: RuntimeError)."""
        if isinstance(texts, str):
            texts = [texts]
        out = torch.zeros(len(texts), context_length, dtype=torch.int64)
        for r, text in enumerate(texts):
            ids = [self.sot] + self.encode(text) + [self.eot]
            if len(ids) > context_length:
                if not truncate:
                    raise RuntimeError(f"Input {text} is too long for context length {context_length}")
                ids = ids[:context_length]
                ids[-1] = self.eot
            out[r, :len(ids)] = torch.tensor(ids, dtype=torch.int64)
        return out


# ------------------------------------------------------------------------------------------------------------------ encoder
class ClipTextEncoder:
    def __init__(self, table, device, tokenizer=None, dataset=None):
        """table: weight_table(...)'s result.  Uploads it (embeddings and projection as f16, vectors as float32) and packs the four
        matrices of every layer into MFMA fragment order, once."""
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ClipTextEncoder runs on the GPU only: there is no CPU path")
        self.tokenizer, self.dataset = tokenizer, dataset
        self.layers = len(table["layers"])
        self.vocab, self.context = int(table["tok_emb"].shape[0]), int(table["pos_emb"].shape[0])
        lib = _native.lib()
        dev = self.device
        self._keep, sources = [], []

        def up(v, dtype):
            t = v.to(dev, dtype).contiguous()
            self._keep.append(t)
            return t

        with torch.cuda.device(dev):
            st = _native.stream_ptr(dev)
            self._layer_array = (_native.MstClipLayer * self.layers)()
            for i, layer in enumerate(table["layers"]):
                for k in LAYER_FIELDS:
                    if k in PACKED:
                        src = layer[k].to(dev, torch.float16).contiguous()
                        dst = torch.empty_like(src)
                        self._keep.append(dst)
                        sources.append(src)
                        _native.check(lib.mst_clip_pack_weight(_native.ptr(src), 1, src.shape[0], src.shape[1], _native.ptr(dst), st))
                        setattr(self._layer_array[i], k, dst.data_ptr())
                    else:
                        setattr(self._layer_array[i], k, up(layer[k], torch.float32).data_ptr())
            self._w = _native.MstClipWeights(
                layers=self.layers, vocab=self.vocab, context=self.context, width=WIDTH, heads=HEADS, ffn=FFN,
                tok_emb=up(table["tok_emb"], torch.float16).data_ptr(), pos_emb=up(table["pos_emb"], torch.float16).data_ptr(),
                lnf_g=up(table["lnf_g"], torch.float32).data_ptr(), lnf_b=up(table["lnf_b"], torch.float32).data_ptr(),
                proj=up(table["proj"], torch.float16).data_ptr(), layer=self._layer_array)
            torch.cuda.current_stream(dev).synchronize()        # the row-major sources may go once they are packed

    @classmethod
    def from_state_dict(cls, sd, device, **kw):
        return cls(weight_table(sd), device, **kw)

    @classmethod
    def from_file(cls, path, device, **kw):
        """A torch.jit archive (the published ViT-B-32.pt), a torch.save dict (a state dict, or {'state_dict': ...}), or .safetensors
        when `safetensors` is importable."""
        path = os.fspath(path)
        if path.endswith(".safetensors"):
            try:
                from safetensors.torch import load_file
            except ImportError as e:
                raise RuntimeError("clip_text: reading .safetensors needs the `safetensors` package") from e
            sd = load_file(path)
        else:
            try:
                sd = torch.jit.load(path, map_location="cpu").state_dict()
            except RuntimeError:
                sd = torch.load(path, map_location="cpu")
                if hasattr(sd, "state_dict"):
                    sd = sd.state_dict()
                elif isinstance(sd, dict) and "state_dict" in sd and not torch.is_tensor(sd["state_dict"]):
                    sd = sd["state_dict"]
        return cls.from_state_dict(sd, device, **kw)

    def check_tokens(self, ids):
        """The host-side contract of encode_tokens: -> (int64 numpy [B, C], live rows per prompt); ValueError naming what is wrong."""
        a = ids.detach().cpu().numpy() if torch.is_tensor(ids) else np.asarray(ids)
        if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1 or a.dtype.kind not in "iu":
            raise ValueError(f"clip_text: token ids must be an integer [B, C] array, got {a.dtype} {a.shape}")
        return check_token_array(a.astype(np.int64), self.vocab, self.context)

    def encode_tokens(self, ids):
        """ids int64 [B, C <= context] on the host or the device, every row holding the end-of-text id (vocab - 1, the row's maximum)
        -> float32 [B, 512] on the device, on the current stream."""
        a, lens = self.check_tokens(ids)
        lib = _native.lib()
        dev = self.device
        B = a.shape[0]
        lens32 = np.ascontiguousarray(lens, dtype=np.int32)
        offs = np.zeros(B, dtype=np.int32)
        rows, nbytes = C.c_int32(), C.c_int64()
        i32p = C.POINTER(C.c_int32)
        _native.check(lib.mst_clip_plan(lens32.ctypes.data_as(i32p), B, self.context, offs.ctypes.data_as(i32p), C.byref(rows), C.byref(nbytes)))
        stride = int(lens32.max())
        host = np.concatenate([a[:, :stride].astype(np.int32).ravel(), lens32, offs])
        with torch.cuda.device(dev):
            buf = torch.from_numpy(host).to(dev)
            ids_d, lens_d, offs_d = buf[:B * stride], buf[B * stride:B * stride + B], buf[B * stride + B:]
            ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
            out = torch.empty(B, WIDTH, dtype=torch.float32, device=dev)
            _native.check(lib.mst_clip_encode(C.byref(self._w), _native.ptr(ids_d), B, stride, _native.ptr(lens_d), _native.ptr(offs_d),
                                              rows.value, _native.ptr(ws), nbytes.value, _native.ptr(out), _native.stream_ptr(dev)))
        return out

    def tokenize(self, texts):
        """encode_text's own rule: HumanML / KIT prompts are cut at 20 tokens + start / end and zero-padded to 77."""
        if self.tokenizer is None:
            raise RuntimeError("clip_text: no tokenizer set: ClipTextEncoder(..., tokenizer=SimpleTokenizer(bpe_path))")
        if self.dataset in ("humanml", "kit"):
            t = self.tokenizer.tokenize(texts, context_length=22, truncate=True)
            return torch.cat([t, torch.zeros(t.shape[0], 77 - 22, dtype=t.dtype)], dim=1)
        return self.tokenizer.tokenize(texts, context_length=77, truncate=True)

    def __call__(self, texts):
        ids = self.tokenize(texts)
        if self.tokenizer.vocab_size != self.vocab:
            raise ValueError(f"clip_text: the tokenizer has {self.tokenizer.vocab_size} entries, the token embedding {self.vocab} rows")
        return self.encode_tokens(ids)


def check_token_array(a, vocab, context):
    """ids int64 [B, C] -> (ids, live rows per prompt = first position of the row's maximum + 1).  ValueError: a context above the
    tower's, an id out of range, a row without the end-of-text id (the vocabulary's last, which CLIP pools at through argmax)."""
    if a.shape[1] > context:
        raise ValueError(f"clip_text: context {a.shape[1]} above the tower's {context}")
    if a.min() < 0 or a.max() >= vocab:
        bad = int(a.min()) if a.min() < 0 else int(a.max())
        raise ValueError(f"clip_text: token id {bad} out of range 0..{vocab - 1}")
    top = a.max(axis=1)
    if np.any(top != vocab - 1):
        r = int(np.nonzero(top != vocab - 1)[0][0])
        raise ValueError(f"clip_text: row {r} holds no end-of-text token (id {vocab - 1}): its largest id is {int(top[r])}")
    return a, a.argmax(axis=1).astype(np.int64) + 1
