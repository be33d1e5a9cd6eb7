"""The cases of tests/test_gpu_token_profile.py: shapes, the kernels each is meant to reach (named by tests/plan_mirror.py), their
inputs and their oracle results.  tests/test_token_profile_cpu.py runs the rounding model through the same cases on the CPU, so the
inputs and the oracle calls live here, once; every oracle result is computed once per process and handed out read-only."""
import functools

import numpy as np
import torch

import plan_mirror as pm
import token_profile as tp

SEED = 4711
FEATS = 263                 # the trunk sweep's width (HumanML)

# ------------------------------------------------------------------------------ the width sweep
# Both ends of every k_embed_in<KS>'s range of widths (KS = 3: 1 .. 96 features pad to 96): the NBW edges 128 / 129, 256 / 257,
# 384 / 385 and 512 are among them.
WIDTHS = [1, 96] + [f for ks in range(4, 17) for f in (32 * ks - 31, 32 * ks)]
# Two clips.  136 and 140 frame rows make three 64-frame tiles, the last one partial, with the clip boundary inside the third;
# T % 4 == 0 takes the staged epilogue (and the fused next-step embedding where one exists), T % 4 == 2 DEpiEmbedOut::finish.
WIDTH_FRAMES = [68, 70]
WIDTH_CLIPS = 2
PRECISE_WIDTHS = [96, 256, 257, 384, 385, 512]
LOOPS = (("ddpm", 1, 0.0), ("ddim", 2, 0.3))           # (sampler, DEpiEmbedOut<MODE>, eta)

# ------------------------------------------------------------------------------ the trunk sweep
# Large tiles forced (MST_SMALL_M=0), three clips: 3 (T + 1) is a multiple of no tile height and both clip boundaries fall inside tiles.
TAIL_NTB = [2, 3, 4]
TRUNK_FRAMES = [15, 100, 191, 196, 207, 223]
TRUNK_CLIPS = 3
# the small paths at their defaults: (clips, frames)
SMALL_SHAPES = [(3, 60), (5, 196), (8, 196), (2, 5)]


def width_cases():
    return [(F, T) for F in WIDTHS for T in WIDTH_FRAMES]


def precise_cases():
    return [(F, T) for F in PRECISE_WIDTHS for T in WIDTH_FRAMES]


def trunk_cases():
    return [(ntb, T) for ntb in TAIL_NTB for T in TRUNK_FRAMES]


def width_kernels(F, T, precise=False):
    """What one width case launches: {call: (pose embedding, output projection[, the loop's first step])}."""
    k = {"forward": (pm.embed_in_kernel(F, precise), pm.embed_out_kernel(F, T, False, precise)),
         "guided": (pm.embed_in_kernel(F, precise), pm.embed_out_kernel(F, T, True, precise))}
    if not precise:
        for name, mode, _ in LOOPS:
            fused = bool(pm.plan_embed_out(F, T, mode=mode)["ksn"])
            # a 2-step loop: the first step hands over to the second (frame rows or the whole embedding), the last step hands over nothing
            k[name] = (pm.embed_in_kernel(F), pm.embed_out_kernel(F, T, mode=mode, fused_next=fused), pm.embed_out_kernel(F, T, mode=mode))
            # under guidance every step hands over frame rows: two accumulator sets (NX 2) up to 384 features, the ring beyond
            k[name + " guided"] = (pm.embed_in_kernel(F), pm.embed_out_kernel(F, T, True, mode=mode))
    return k


def trunk_kernels(B, T, small_m=pm.SMALL_M, tail_ntb=0):
    """{call: (path, detail)} of one trunk case: forward runs B rows, guided forward 2 B."""
    out = {}
    for call, rows in (("forward", B), ("guided", 2 * B)):
        p = pm.plan_trunk(pm.knobs(small_m=small_m, tail_ntb=tail_ntb), rows, T)
        path = pm.PATHS[p["path"]]
        if path == "large":
            detail = f"nt16 {p['nt16']}, {pm.QKV_ATTN[p['qkv_attn']]}, tail_ntb {p['tail_ntb']}"
        elif path == "small-ring":
            detail = "hi + lo" if p["precise"] else "plain"
        else:
            detail = f"rows ntb {1 if path == 'small-rows-ln' else pm.rows_ntb(rows * (T + 1))}"
        out[call] = (path, detail, p)
    return out


# ------------------------------------------------------------------------------ inputs
def _syn():
    import mst_amd  # noqa: F401
    import mst_amd.synthetic as syn
    return syn


@functools.lru_cache(maxsize=None)
def weights(F):
    syn = _syn()
    return syn.denoiser_state(SEED, F), syn.positional_table(5000, 512)


T_OF_CLIP = [17, 803, 431, 0, 999, 250, 650, 77]        # original-process timesteps, per clip


def forward_inputs(F, T, B):
    syn = _syn()
    return dict(x=syn.normal(SEED, f"x/{F}/{T}/{B}", (B, F, 1, T)), txt=syn.normal(SEED, f"txt/{B}", (B, 512)),
                t=np.array(T_OF_CLIP[:B]), scale=np.linspace(1.5, 2.5, B).astype(np.float32))


def loop_inputs(F, T, B):
    """A 2-step loop over the last two indices of a 20-step respacing, with recorded noise and a mask that is not the root pattern
    (every third feature, frames 0 .. T / 2)."""
    syn = _syn()
    shape = (B, F, 1, T)
    mask = np.zeros(shape, np.float32)
    mask[:, ::3, :, : max(1, T // 2)] = 1
    return dict(shape=shape, mask=mask, motion=syn.normal(SEED, f"motion/{F}/{T}", shape), txt=syn.normal(SEED, f"txt/{B}", (B, 512)),
                nz=np.stack([syn.normal(SEED, f"nz{k}/{F}/{T}", shape) for k in range(3)]))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def oracle_forward(F, T, B, guided):
    """(reference, fp16 model) of one forward / guided forward."""
    from oracle import denoiser
    w, pe = weights(F)
    i = forward_inputs(F, T, B)
    if guided:
        return _frozen(*tp.rounding_model(denoiser.cfg_forward, w, pe, i["x"], i["t"], i["txt"], i["scale"]))
    return _frozen(*tp.rounding_model(denoiser.forward, w, pe, i["x"], i["t"], i["txt"]))


@functools.lru_cache(maxsize=None)
def oracle_loop(F, T, B, sampler, eta, guided=False):
    """(reference, fp16 model) x0-hat dumps [2, B, F, 1, T] of the 2-step loop; guided: over cfg_forward with forward_inputs' scales."""
    from oracle import denoiser, diffusion, schedule
    w, pe = weights(F)
    i = loop_inputs(F, T, B)
    tab, tmap = schedule.make("cosine", 1000, "ddim20")

    def loop(model_fn):
        return diffusion.sample_loop(model_fn, tab, tmap, i["shape"], lambda k: torch.from_numpy(i["nz"][k]), sampler, True, i["mask"],
                                     i["motion"], init_image=i["motion"], skip_timesteps=18, eta=eta, dump_all_xstart=True)
    if guided:
        return _frozen(*tp.rounding_model(denoiser.cfg_forward, w, pe, i["txt"], forward_inputs(F, T, B)["scale"], loop=loop))
    return _frozen(*tp.rounding_model(denoiser.forward, w, pe, i["txt"], loop=loop))
