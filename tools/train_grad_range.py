"""What dynamic range of cotangents the fine-tune objective hands to ONE native backward pass.

mst_train_backward / mst_train_model_backward / mst_motion_encoder_backward scale the whole launch by one power of two (max |g| into
[16, 32)); a clip whose gradient lies 2^-k below the launch's largest loses f16 precision from k = 18 on (DESIGN section 5,
tests/test_gpu_train_profile.py: R_SUPPORTED).  This runs the three fine-tune gradient cases of tests/test_gpu_boundary.py and records,
per backward pass, max |g| of every clip that enters a stack:

  torch   the model evaluated with torch ops (tests/torch_reference.py), a tensor hook on the output of every nn.TransformerEncoder call:
          the gradient entering the trainable stack (one call per chained step: the clips of the shared tape) and the frozen motion encoder;
  native  the arguments of DenoiserEngine.train_model_backward (d_out per clip) and motion_encoder_backward (d_mu per clip).

    python tools/train_grad_range.py            # one JSON line per case and path; the last line is the worst ratio (OBJECTIVE_RATIO)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import test_gpu_boundary as tb  # noqa: E402
from mst_amd.engine import DenoiserEngine  # noqa: E402
from torch_reference import use_native, use_torch_ops  # noqa: E402

CASES = ("xia|ft1", "xia|ft0", "hml|ft1")


def ratio(maxima):
    live = [m for m in maxima if m > 0]
    return max(live) / min(live) if live else 1.0


def run_case(case, path):
    model = tb.build("stylexia_posrot" if case.startswith("xia") else "humanml")["m"]
    seen = {}                                             # stack name -> per call, the per-clip max |g|
    handles, saved = [], {}
    if path == "torch":
        use_torch_ops(model)
        for name, mod in model.named_modules():
            if isinstance(mod, torch.nn.TransformerEncoder):
                def fwd_hook(m, args, out, name=name):
                    if out.requires_grad:                 # [S, B, 512]
                        out.register_hook(lambda g, name=name: seen.setdefault(name, []).append(g.abs().amax((0, 2)).tolist()))
                handles.append(mod.register_forward_hook(fwd_hook))
    else:
        for meth, arg in (("train_model_backward", 1), ("motion_encoder_backward", 1)):
            saved[meth] = getattr(DenoiserEngine, meth)

            def patched(self, *a, _orig=saved[meth], _name=meth, **k):
                g = a[1]
                seen.setdefault(_name, []).append(g.reshape(g.shape[0], -1).abs().amax(1).tolist())
                return _orig(self, *a, **k)
            setattr(DenoiserEngine, meth, patched)
    status = "ok"
    try:
        tb.test_finetune_gradients_all_96_tensors_and_input_gradient_vs_reference(case)
    except AssertionError as e:                           # the recording is done by then: backward runs before the comparisons
        status = "assertion: " + str(e)[:120]
    finally:
        for h in handles:
            h.remove()
        for meth, fn in saved.items():
            setattr(DenoiserEngine, meth, fn)
        use_native(model)
        model.zero_grad()
    # per call: what one launch sees; merged: every clip that entered the stack during the pass, whichever launch took it (an upper bound)
    merged = {n: [x for call in v for x in call] for n, v in seen.items()}
    out = {"case": case, "path": path, "status": status,
           "stacks": {n: {"calls": len(seen[n]), "clips": len(v), "max": max(v), "min_nonzero": min([x for x in v if x > 0] or [0.0]),
                          "ratio_per_call": max(ratio(c) for c in seen[n]), "ratio_merged": ratio(v)} for n, v in merged.items()}}
    print(json.dumps(out), flush=True)
    if path == "native":                                  # every call is one launch with a scale of its own
        return max([ratio(c) for v in seen.values() for c in v] or [1.0])
    return max([ratio(v) for v in merged.values()] or [1.0])


def main():
    worst = {"torch": 1.0, "native": 1.0}
    for path in ("torch", "native"):
        for case in CASES:
            try:
                worst[path] = max(worst[path], run_case(case, path))
            except Exception as e:                        # noqa: BLE001  (a path the objective cannot take is reported, not hidden)
                print(json.dumps({"case": case, "path": path, "status": f"{type(e).__name__}: {str(e)[:200]}"}), flush=True)
    print(json.dumps({"objective_ratio": worst, "log2": {k: round(float(torch.log2(torch.tensor(v))), 2) for k, v in worst.items()}}))


if __name__ == "__main__":
    main()
