"""Times the native CLIP text tower (mst_amd.model.clip_text, csrc/mst_clip.h) against the same 12-layer tower evaluated with torch ops
in fp16 on the device, as clip_model.encode_text runs it after clip.model.convert_weights: every one of the 77 positions, causal mask,
pooled at argmax.  Shapes: 32 and 64 prompts with a HumanML-like length mix (end-of-text uniform in 6 .. 21, context 22 zero-padded
to 77) and 64 prompts filling all 77 positions.  Both sides get their token ids on the device's host side the same way (a host int64
tensor in, an embedding on the device out), so the native side's validation and planning are inside its time.

Method: per shape, `--reps` interleaved repetitions (native, torch, native, torch, ...), each timing `--iters` calls between device
synchronises with the host clock; the medians are reported, with the spread (min .. max) beside them.  Needs a GPU; prints one JSON line
per shape.

    python tools/clip_text_bench.py [--reps 9] [--iters 20] [--layers 12]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mst_amd  # noqa: E402,F401
from mst_amd.model.clip_text import ClipTextEncoder  # noqa: E402

VOCAB, WIDTH, FFN, CTX = 49408, 512, 2048, 77


def weights(layers, dev):
    g = torch.Generator(device="cpu").manual_seed(1)
    n = lambda *s: torch.randn(*s, generator=g)
    sd = {"token_embedding.weight": 0.02 * n(VOCAB, WIDTH), "positional_embedding": 0.01 * n(CTX, WIDTH),
          "ln_final.weight": 1 + 0.1 * n(WIDTH), "ln_final.bias": 0.05 * n(WIDTH), "text_projection": n(WIDTH, WIDTH) / WIDTH ** 0.5}
    for i in range(layers):
        p = f"transformer.resblocks.{i}."
        for ln in ("ln_1", "ln_2"):
            sd[p + ln + ".weight"], sd[p + ln + ".bias"] = 1 + 0.1 * n(WIDTH), 0.05 * n(WIDTH)
        sd[p + "attn.in_proj_weight"], sd[p + "attn.in_proj_bias"] = n(3 * WIDTH, WIDTH) / WIDTH ** 0.5, 0.02 * n(3 * WIDTH)
        sd[p + "attn.out_proj.weight"], sd[p + "attn.out_proj.bias"] = n(WIDTH, WIDTH) / WIDTH ** 0.5, 0.02 * n(WIDTH)
        sd[p + "mlp.c_fc.weight"], sd[p + "mlp.c_fc.bias"] = n(FFN, WIDTH) / WIDTH ** 0.5, 0.02 * n(FFN)
        sd[p + "mlp.c_proj.weight"], sd[p + "mlp.c_proj.bias"] = n(WIDTH, FFN) / FFN ** 0.5, 0.02 * n(WIDTH)
    return {k: v.half() for k, v in sd.items()}


def torch_tower(sd, layers, dev):
    w = {k: v.to(dev) for k, v in sd.items()}

    def run(ids_host):
        ids = ids_host.to(dev)
        B, C = ids.shape
        x = w["token_embedding.weight"][ids] + w["positional_embedding"][:C]
        for i in range(layers):
            p = f"transformer.resblocks.{i}."
            h = F.layer_norm(x, (WIDTH,), w[p + "ln_1.weight"], w[p + "ln_1.bias"])
            q, k, v = (t.view(B, C, 8, 64).transpose(1, 2) for t in F.linear(h, w[p + "attn.in_proj_weight"], w[p + "attn.in_proj_bias"]).chunk(3, -1))
            o = F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(B, C, WIDTH)
            x = x + F.linear(o, w[p + "attn.out_proj.weight"], w[p + "attn.out_proj.bias"])
            h = F.layer_norm(x, (WIDTH,), w[p + "ln_2.weight"], w[p + "ln_2.bias"])
            u = F.linear(h, w[p + "mlp.c_fc.weight"], w[p + "mlp.c_fc.bias"])
            x = x + F.linear(u * torch.sigmoid(1.702 * u), w[p + "mlp.c_proj.weight"], w[p + "mlp.c_proj.bias"])
        x = F.layer_norm(x, (WIDTH,), w["ln_final.weight"], w["ln_final.bias"])
        return (x[torch.arange(B, device=dev), ids.argmax(-1)] @ w["text_projection"]).float()
    return run


def prompts(batch, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(batch, CTX, dtype=torch.int64)
    for b in range(batch):
        e = int(torch.randint(lo, hi + 1, (1,), generator=g))
        ids[b, 0] = VOCAB - 2
        ids[b, 1:e] = torch.randint(0, VOCAB - 2, (e - 1,), generator=g)
        ids[b, e] = VOCAB - 1
    return ids


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--layers", type=int, default=12)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_text_bench needs a GPU: a CPU run measures nothing")
    dev = torch.device("cuda")
    sd = weights(a.layers, dev)
    enc, ref = ClipTextEncoder.from_state_dict(sd, dev), torch_tower(sd, a.layers, dev)
    for name, batch, lo, hi in (("humanml_mix_32", 32, 6, 21), ("humanml_mix_64", 64, 6, 21), ("full_77_64", 64, 76, 76)):
        ids = prompts(batch, lo, hi, batch + hi)
        y, z = enc.encode_tokens(ids), ref(ids)
        err = float(((y - z).abs().amax(-1) / z.abs().amax(-1)).max())
        for _ in range(3):
            enc.encode_tokens(ids), ref(ids)
        tn, tt = [], []
        for _ in range(a.reps):
            tn.append(timed(lambda: enc.encode_tokens(ids), a.iters))
            tt.append(timed(lambda: ref(ids), a.iters))
        print(json.dumps({"shape": name, "prompts": batch, "live_rows": int((ids.argmax(-1) + 1).sum()), "layers": a.layers,
                          "native_ms": round(statistics.median(tn), 4), "native_ms_range": [round(min(tn), 4), round(max(tn), 4)],
                          "torch_fp16_ms": round(statistics.median(tt), 4), "torch_fp16_ms_range": [round(min(tt), 4), round(max(tt), 4)],
                          "torch_over_native": round(statistics.median(tt) / statistics.median(tn), 3),
                          "native_vs_torch_fp16_max_rel": err, "reps": a.reps, "iters": a.iters}), flush=True)


if __name__ == "__main__":
    main()
