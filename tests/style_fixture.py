"""Several styles in one engine, shared by the style GPU tests (test_gpu_style_bank.py, test_gpu_style_kernels.py): synthetic styles
(each its own seeded encoder stack over ONE shared prior), an engine that holds them in style slots, and the fp32 oracle of one style."""
import numpy as np
import torch

from mst_amd import synthetic as syn
from conftest import SEED

PRIOR = "motion_enc.mdm_model."
LP = "seqTransEncoder.layers."


def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


_W = {}


def style_weights(F, s):
    """Style s at F features: the stack of seed SEED + 1 + s, the prior of SEED (shared by every style)."""
    if (F, s) not in _W:
        prior = syn.denoiser_state(SEED, F, layer_prefix=LP, prior_prefix=PRIOR)
        w = syn.denoiser_state(SEED + 1 + s, F, layer_prefix=LP, prior_prefix=PRIOR)
        w.update({k: v for k, v in prior.items() if k.startswith(PRIOR)})
        _W[(F, s)] = w
    return _W[(F, s)]


def layer_list(w, nl=8):
    from mst_amd.engine import LAYER_TENSORS
    return [cu(w[f"{LP}{i}.{k}"]) for i in range(nl) for k in LAYER_TENSORS]


_PE = []


def pe():
    if not _PE:
        _PE.append(syn.positional_table(5000, 512))
    return _PE[0]


def make_engine(F, T, max_rows, slots):
    """An engine for clips of up to T frames: style 0 in slot 0 (the engine's own weights), style s in slot s.  MST_* switches read
    at creation (MST_SMALL_M, MST_TAIL_NTB, MST_STYLE_XCD) take the caller's environment."""
    from mst_amd.engine import DenoiserEngine
    eng = DenoiserEngine(F, T, max_rows, device=dev())
    eng.load_state_dict({k: torch.from_numpy(v) for k, v in style_weights(F, 0).items()}, prior_prefix=PRIOR,
                        pe=torch.from_numpy(pe()))
    if slots > 1:
        eng.style_slots(slots)
        for s in range(1, slots):
            eng.load_layers_slot(s, layer_list(style_weights(F, s)))
    torch.cuda.synchronize()
    return eng


def schedule():
    from mst_amd.engine import Schedule
    from oracle import schedule as osch
    tab, tmap = osch.make("cosine", 1000, "")
    return Schedule(tab, tmap, dev())


def oracle_forward(F, s, x, t, txt, scale=None):
    """Style s's denoiser on the CPU in fp32 (guided by `scale` per clip when given: ClassifierFreeSampleModel)."""
    from oracle import denoiser
    if scale is None:
        return denoiser.forward(style_weights(F, s), pe(), x, t, txt, prior=PRIOR)
    return denoiser.cfg_forward(style_weights(F, s), pe(), x, t, txt, scale, prior=PRIOR)
