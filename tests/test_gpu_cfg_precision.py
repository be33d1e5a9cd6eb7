"""Classifier-free guidance (BASELINE.json configs[2]) against the fp32 oracle, per clip, across the guidance scale.

The blend u + s (c - u) runs in fp32, but c and u come out of f16-operand GEMMs: their rounding is amplified by about s.  These
tests measure that on both launch paths (the large-tile kernels a batch takes, the small-tile kernels a launch of a few clips
takes), pin the reference-free identities of the blend, run guided inpainting loops clip by clip, and run the full-length
(1000-step, 263 x 196) plain and guided loops exactly as bench.py launches them, one clip of the last slice against the oracle.
The default path must hold 1e-3 relative L2 per clip for every scale up to engine.CFG_SCALE_MAX; above it the engine warns."""
import os
import time
import warnings

import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
from mst_amd import synthetic as syn
from conftest import SEED, rel_l2

pytestmark = pytest.mark.gpu

TOL = 1e-3
SHAPES = {"xia": (181, 76), "hml": (263, 196)}
SCALES = (1.0, 1.5, 2.5, 3.0, 4.0)
NSEED = 8
SMALL_CLIPS = 4          # clips per launch on the small-tile path: 8 rows x 197 tokens, under MST_SMALL_M's default of 1900
PATHS = {"large": "0", "small": "1900"}       # MST_SMALL_M at engine creation: 0 = never the small-tile kernels
SWEEP = {}               # (tag, path, scale) -> per-clip errors, for the table and the CFG_SCALE_MAX check


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    print(f"\n[time] {request.node.name}: {time.perf_counter() - t0:.1f} s")


_W, _ENG = {}, {}


def weights(tag):
    if tag not in _W:
        _W[tag] = syn.denoiser_state(SEED, SHAPES[tag][0])
    return _W[tag]


def engine(tag, rows, small_m=None, precise=False, fresh=False):
    """A cached engine (fresh: a new one); MST_SMALL_M / MST_PRECISE are read at creation, so the launch path is fixed here
    (None: the defaults)."""
    from mst_amd.engine import DenoiserEngine
    key = (tag, rows, small_m, precise)
    if fresh or key not in _ENG:
        F, T = SHAPES[tag]
        env = {"MST_SMALL_M": small_m, "MST_PRECISE": "1" if precise else "0"}
        old = {k: os.environ.get(k) for k in env}
        try:
            for k, v in env.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
            eng = DenoiserEngine(F, T, rows, device=_dev())
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        eng.load_state_dict({k: torch.from_numpy(v) for k, v in weights(tag).items()},
                            pe=torch.from_numpy(syn.positional_table(5000, 512)))
        if fresh:
            return eng
        _ENG[key] = eng
    return _ENG[key]


def cfg_warnings(fn):
    """The guidance-scale warnings `fn()` raises (any other warning is not this test's business)."""
    with warnings.catch_warnings(record=True) as got:
        warnings.simplefilter("always")
        fn()
    return [w for w in got if "CFG_SCALE_MAX" in str(w.message)]


def seeds(tag, n=NSEED, name="sweep"):
    """n clips, each its own x, text embedding and timestep; the timesteps spread over 0..999 (both ends included)."""
    F, T = SHAPES[tag]
    x = np.concatenate([syn.normal(SEED, f"cfgp/{name}/{tag}/x/{i}", (1, F, 1, T)) for i in range(n)])
    txt = np.stack([syn.normal(SEED, f"cfgp/{name}/{tag}/txt/{i}", (512,)) for i in range(n)])
    t = np.linspace(0, 999, n).round().astype(np.int64)
    return x, txt, t


def per_clip(out, ref, sel=None):
    """Relative L2 of every clip (over the entries `sel` picks, when given)."""
    out, ref = np.asarray(out), np.asarray(ref)
    if sel is None:
        return np.array([rel_l2(out[i], ref[i]) for i in range(out.shape[0])])
    return np.array([rel_l2(out[i][sel[i]], ref[i][sel[i]]) for i in range(out.shape[0])])


def guided(eng, x, t, txt, scale, clips):
    """The guided forward in launches of `clips` clips."""
    outs = []
    for lo in range(0, x.shape[0], clips):
        eng.set_text(cu(txt[lo:lo + clips]), cfg=True)
        outs.append(eng.forward(cu(x[lo:lo + clips]), cu(t[lo:lo + clips]), scale=cu(scale[lo:lo + clips]), cfg=True))
    return torch.cat(outs).cpu().numpy()


def plain(eng, x, t, txt, clips, uncond=False):
    """The unguided forward (conditional, or unconditional rows: keep = 0) in launches of `clips` clips."""
    outs = []
    for lo in range(0, x.shape[0], clips):
        n = min(clips, x.shape[0] - lo)
        eng.set_text(cu(txt[lo:lo + n]), keep=cu(np.zeros(n, np.float32)) if uncond else None)
        outs.append(eng.forward(cu(x[lo:lo + n]), cu(t[lo:lo + n])))
    return torch.cat(outs).cpu().numpy()


# ------------------------------------------------------------------------------ (a) the guided forward across the scale
@pytest.mark.parametrize("tag", ["xia", "hml"])
def test_guided_forward_scale_sweep(tag):
    """8 clips x 5 scales = 40 clips (80 rows): one launch on the large-tile path, launches of 4 clips on the small-tile path.
    Every clip against oracle.denoiser.cfg_forward; a table of worst / mean per scale."""
    from oracle import denoiser
    from mst_amd.engine import CFG_SCALE_MAX
    assert CFG_SCALE_MAX in SCALES
    x1, txt1, t1 = seeds(tag)
    n = len(SCALES)
    x, txt, t = np.repeat(x1, n, 0), np.repeat(txt1, n, 0), np.repeat(t1, n)
    scale = np.tile(np.array(SCALES, np.float32), NSEED)                  # clip k: seed k // 5 at scale SCALES[k % 5]
    torch.set_num_threads(16)
    ref = denoiser.cfg_forward(weights(tag), syn.positional_table(5000, 512), x, t, txt, scale).numpy()
    B = x.shape[0]
    lines = [f"guided forward {tag} {SHAPES[tag]}: relative L2 per clip vs fp32, {NSEED} clips per scale"]
    for path, clips in (("large", B), ("small", SMALL_CLIPS)):
        eng = engine(tag, 2 * clips, PATHS[path])
        out = guided(eng, x, t, txt, scale, clips)
        assert np.isfinite(out).all()
        e = per_clip(out, ref)
        for j, s in enumerate(SCALES):
            es = e[j::n]
            SWEEP[(tag, path, s)] = es
            lines.append(f"  {path:5s} tiles  scale {s:3.1f}  worst {es.max():.2e}  mean {es.mean():.2e}  (clip {int(es.argmax())})")
    print("\n" + "\n".join(lines))
    print("\nworst / mean relative L2 per clip, guided forward, every sweep so far (CFG_SCALE_MAX = %g)" % CFG_SCALE_MAX)
    print("scale | " + " | ".join(f"{tg} {path}" for tg in SHAPES for path in PATHS))
    for s in SCALES:
        cells = [SWEEP.get((tg, path, s)) for tg in SHAPES for path in PATHS]
        print(f"{s:5.1f} | " + " | ".join("-" if c is None else f"{c.max():.2e} / {c.mean():.2e}" for c in cells))
    for (tg, path, s), es in SWEEP.items():
        if tg == tag and s <= CFG_SCALE_MAX:
            assert es.max() < TOL, (tag, path, s, es)


# ------------------------------------------------------------------------------ (b) identities of the blend, reference-free
@pytest.mark.parametrize("tag", ["xia", "hml"])
@pytest.mark.parametrize("path", ["large", "small"])
def test_scale_one_is_cond_and_scale_zero_is_uncond(tag, path):
    """u + 1 (c - u) is c and u + 0 (c - u) is u up to one fp32 rounding, on the same launch path and batch size: catches swapped
    cond / uncond rows or a wrong blend whatever the operand rounding does."""
    x, txt, t = seeds(tag, name="ident")
    clips = NSEED if path == "large" else SMALL_CLIPS
    eng = engine(tag, 2 * clips, PATHS[path])
    c = plain(eng, x, t, txt, clips)
    u = plain(eng, x, t, txt, clips, uncond=True)
    assert per_clip(u, c).min() > 1e-4                  # the two halves differ: the identities below can tell them apart
    for s, want in ((1.0, c), (0.0, u)):
        g = guided(eng, x, t, txt, np.full(NSEED, s, np.float32), clips)
        e = per_clip(g, want)
        print(f"identity {tag} {path} scale {s}: worst {e.max():.1e}")
        assert e.max() < 1e-6, (s, e)


# ------------------------------------------------------------------------------ precise mode above the limit, and the warning
@pytest.mark.parametrize("tag", ["xia", "hml"])
def test_precise_mode_holds_above_the_limit(tag):
    """set_precise(True) splits every operand: the sweep's largest scale and one well above CFG_SCALE_MAX stay within 1e-3."""
    from oracle import denoiser
    from mst_amd.engine import CFG_SCALE_MAX
    x, txt, t = seeds(tag)
    big = 2.0 * CFG_SCALE_MAX
    eng = engine(tag, 2 * SMALL_CLIPS, precise=True)
    torch.set_num_threads(16)
    ref_c = denoiser.forward(weights(tag), syn.positional_table(5000, 512), x, t, txt).numpy()
    ref_u = denoiser.forward(weights(tag), syn.positional_table(5000, 512), x, t, txt, uncond=True).numpy()
    for s in (max(SCALES), big):
        assert not cfg_warnings(lambda: eng.check_guidance_scale(cu(np.full(NSEED, s, np.float32))))    # precise mode: silent
        e = per_clip(guided(eng, x, t, txt, np.full(NSEED, s, np.float32), SMALL_CLIPS), ref_u + s * (ref_c - ref_u))
        print(f"precise {tag} scale {s}: worst {e.max():.2e} mean {e.mean():.2e}")
        assert e.max() < TOL, (s, e)


def test_guidance_above_the_limit_warns_once_per_engine():
    from mst_amd.engine import CFG_SCALE_MAX, Schedule, SAMPLER_DDPM
    from oracle import schedule
    F, T = SHAPES["xia"]
    tab, tmap = schedule.make("cosine", 1000, "")
    sch = Schedule(tab, tmap, _dev())
    x, txt, t = seeds("xia", 2, "warn")
    mask, motion = cu(syn.root_horizontal_mask(2, F, T)), cu(x)
    over = CFG_SCALE_MAX + 0.5
    eng = engine("xia", 4, fresh=True)
    eng.set_text(cu(txt), cfg=True)
    run = lambda s: (lambda: eng.sample_loop(sch, cu(x).clone(), 1, 0, SAMPLER_DDPM, cfg=True, scale=cu(np.array(s, np.float32)),
                                             mask=mask, motion=motion, seed=3))
    assert not cfg_warnings(run([2.5, 1.0]))               # the reference's scripts' scale: silent
    assert not cfg_warnings(run([CFG_SCALE_MAX, 0.0]))
    got = cfg_warnings(run([1.5, over]))
    assert len(got) == 1 and "set_precise(True) / MST_PRECISE=1" in str(got[0].message), got
    assert not cfg_warnings(run([over, over]))             # once per engine
    # a fresh engine warns again; negative scales extrapolate the other way (1 - s counts); host arrays are checked too
    eng = engine("xia", 4, fresh=True)
    assert len(cfg_warnings(lambda: eng.check_guidance_scale(np.array([1.0, 1.0 - over])))) == 1


def test_guidance_warning_through_the_drop_in_boundary():
    """The scripts' path: ClassifierFreeSampleModel.forward and GaussianDiffusion's native loop check the scale too."""
    from test_gpu_boundary import build
    from mst_amd.engine import CFG_SCALE_MAX
    from mst_amd.model.cfg_sampler import ClassifierFreeSampleModel
    c = build()
    F, T = SHAPES["xia"]
    B = 3
    x = cu(syn.normal(SEED, "cfgp/boundary/x", (B, F, 1, T)))
    t = torch.full((B,), 5, device=_dev())
    y = {"text": ["a person walks proudly"] * B, "mask": torch.ones(B, 1, 1, T, device=_dev()),
         "inpainting_mask": cu(syn.root_horizontal_mask(B, F, T)), "inpainted_motion": x}
    model = ClassifierFreeSampleModel(c["m"])

    def fresh(fn):                                      # the model's engines forget an earlier warning: each case starts clean
        def go():
            for ent in c["m"].__dict__.get("_mst_engines", {}).values():
                ent["eng"]._cfg_warned, ent["eng"]._cfg_seen = False, None
            with torch.no_grad():
                fn()
        return go
    at = lambda s: {**y, "scale": torch.full((B,), s, device=_dev())}
    over = CFG_SCALE_MAX + 1.0
    loop = lambda s: c["full"].p_sample_loop(model, (B, F, 1, T), clip_denoised=False, skip_timesteps=997, init_image=x,
                                             model_kwargs={"y": at(s)})
    fresh(lambda: model(x, t, at(2.5)))()              # (builds the engine)
    assert not cfg_warnings(fresh(lambda: model(x, t, at(2.5))))
    assert len(cfg_warnings(fresh(lambda: model(x, t, at(over))))) == 1
    assert not cfg_warnings(fresh(lambda: loop(2.5)))
    assert len(cfg_warnings(fresh(lambda: loop(over)))) == 1


# ------------------------------------------------------------------------------ (c) guided inpainting loops, clip by clip
@pytest.mark.parametrize("tag", ["xia", "hml"])
def test_guided_inpainting_loops_per_clip(tag):
    """DDPM indices 9..0 of the full process, recorded noise, root_horizontal inpainting, scales 1.5 and 2.5 over 4 clips each;
    the batch of 8 on the large-tile path and in launches of 4 on the small-tile path, every clip against the oracle's loop."""
    from oracle import denoiser, diffusion, schedule
    from mst_amd.engine import Schedule, SAMPLER_DDPM
    F, T = SHAPES[tag]
    x, txt, _ = seeds(tag, name="loop")
    B = x.shape[0]
    shape = (B, F, 1, T)
    scale = np.repeat(np.array([1.5, 2.5], np.float32), B // 2)
    mask = syn.root_horizontal_mask(B, F, T)
    motion = syn.normal(SEED, f"cfgp/loop/{tag}/motion", shape)
    nz = np.stack([syn.normal(SEED, f"cfgp/loop/{tag}/noise/{k}", shape) for k in range(11)])
    tab, tmap = schedule.make("cosine", 1000, "")
    sch = Schedule(tab, tmap, _dev())
    w, pe = weights(tag), syn.positional_table(5000, 512)
    torch.set_num_threads(16)
    ref = diffusion.sample_loop(lambda xx, tt: denoiser.cfg_forward(w, pe, xx, tt, txt, scale), tab, tmap, shape,
                                lambda k: torch.from_numpy(nz[k]), "ddpm", True, mask, motion, init_image=motion,
                                skip_timesteps=990).numpy()
    free = mask == 0
    for path, clips in (("large", B), ("small", SMALL_CLIPS)):
        eng = engine(tag, 2 * clips, PATHS[path])
        outs = []
        for lo in range(0, B, clips):
            hi = lo + clips
            eng.set_text(cu(txt[lo:hi]), cfg=True)
            x9 = sch.q_sample(cu(motion[lo:hi]), cu(np.full(clips, 9)), cu(nz[0, lo:hi]), cu(mask[lo:hi]))
            outs.append(eng.sample_loop(sch, x9, 9, 0, SAMPLER_DDPM, cfg=True, scale=cu(scale[lo:hi]), mask=cu(mask[lo:hi]),
                                        motion=cu(motion[lo:hi]), noise=cu(nz[1:, lo:hi])))
        out = torch.cat(outs).cpu().numpy()
        assert np.array_equal(out[mask == 1], motion[mask == 1])          # masked entries bit for bit
        e, e_free = per_clip(out, ref), per_clip(out, ref, free)
        for s in (1.5, 2.5):
            k = scale == s
            print(f"guided loop {tag} {path} scale {s}: worst {e[k].max():.2e} mean {e[k].mean():.2e}   "
                  f"unmasked entries: worst {e_free[k].max():.2e} mean {e_free[k].mean():.2e}")
        assert e.max() < TOL and e_free.max() < TOL, (path, e, e_free)


# ------------------------------------------------------------------------------ (d) 1000 steps at the headline shape
@pytest.mark.parametrize("kind", ["plain", "guided"])
def test_full_length_headline_loop_one_clip_of_the_last_slice(kind):
    """bench.py's launch (configs[1] / configs[2]): 64 clips of (263, 1, 196), all 1000 DDPM indices, root_horizontal inpainting,
    in-kernel Philox noise, on an engine built as bench.py builds it.  Clip 63 (in the last slice) against the oracle fed the same
    Philox numbers, and the same clip alone on a small-tile engine with those numbers injected."""
    from oracle import denoiser, diffusion, schedule
    from mst_amd.engine import Schedule, SAMPLER_DDPM
    tag, B, seed, i = "hml", 64, 4242 if kind == "plain" else 4243, 63
    F, T = SHAPES[tag]
    cfg = kind == "guided"
    scale = np.linspace(1.5, 3.0, B).astype(np.float32) if cfg else None    # every clip its own scale: clip 63 is 3.0
    eng = engine(tag, 2 * B if cfg else B)                                   # bench.py: DenoiserEngine(F, T, rows), default switches
    assert eng.loop_slices(B, cfg) == (2 if cfg else 3)
    txt = syn.normal(SEED, f"cfgp/long/{kind}/txt", (B, 512))
    x0 = syn.normal(SEED, f"cfgp/long/{kind}/x", (B, F, 1, T))
    motion = syn.normal(SEED, f"cfgp/long/{kind}/motion", (B, F, 1, T))
    mask = syn.root_horizontal_mask(B, F, T)
    tab, tmap = schedule.make("cosine", 1000, "")
    sch = Schedule(tab, tmap, _dev())
    eng.set_text(cu(txt), cfg=cfg)
    big = eng.sample_loop(sch, cu(x0).clone(), 999, 0, SAMPLER_DDPM, cfg=cfg, scale=None if scale is None else cu(scale),
                          mask=cu(mask), motion=cu(motion), mask_noise=True, seed=seed)
    big = big[i:i + 1].cpu().numpy()
    # the clip's noise of every step, as the kernel draws it (the slice's clip offset in the counter included)
    nz = torch.empty((1000, 1, F, 1, T), dtype=torch.float32)
    for j in range(1000):
        nz[j] = eng.philox_normal(B, T, seed, j)[i].cpu()
    sl = slice(i, i + 1)
    w, pe = weights(tag), syn.positional_table(5000, 512)
    if cfg:
        s = float(scale[i])
        txt2 = np.concatenate([txt[sl], txt[sl]])
        keep = np.array([1.0, 0.0], np.float32)

        def model_fn(xx, tt):                               # cond and uncond of the clip in ONE oracle call per step
            o = denoiser.forward(w, pe, torch.cat([xx, xx]), torch.cat([tt, tt]), txt2, cond_keep=keep)
            return o[1:] + s * (o[:1] - o[1:])
    else:
        model_fn = lambda xx, tt: denoiser.forward(w, pe, xx, tt, txt[sl])
    torch.set_num_threads(16)
    t0 = time.perf_counter()
    ref = diffusion.sample_loop(model_fn, tab, tmap, (1, F, 1, T), lambda k: torch.from_numpy(x0[sl]) if k == 0 else nz[k - 1],
                                "ddpm", True, torch.from_numpy(mask[sl]), torch.from_numpy(motion[sl])).numpy()
    t_oracle = time.perf_counter() - t0
    one = engine(tag, 2, PATHS["small"])
    one.set_text(cu(txt[sl]), cfg=cfg)
    alone = one.sample_loop(sch, cu(x0[sl]).clone(), 999, 0, SAMPLER_DDPM, cfg=cfg, scale=None if scale is None else cu(scale[sl]),
                            mask=cu(mask[sl]), motion=cu(motion[sl]), mask_noise=True, noise=nz.to(_dev())).cpu().numpy()
    e_big, e_one = rel_l2(big, ref), rel_l2(alone, ref)
    print(f"1000-step {kind} loop (263,1,196), clip {i} of {B}{f', scale {scale[i]:.1f}' if cfg else ''}: "
          f"64-clip Philox launch {e_big:.2e}, the clip alone (small tiles, injected noise) {e_one:.2e}  (oracle {t_oracle:.0f} s)")
    for out in (big, alone):
        assert np.array_equal(out[:, :3], motion[sl, :3])
    assert e_big < TOL and e_one < TOL, (e_big, e_one)
