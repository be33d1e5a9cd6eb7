"""Overlapping windows on the GPU (csrc/mst_window.h, mst_amd/diffusion/windows.py, GaussianDiffusion.ddim_sample_loop_windows).

Kernels: k_window_unfold / k_window_stitch against tests/window_fixture.py under the suite's bar -- relative L2 against the float64
statement at most 4 x the float32 statement's own distance from it, floor 1e-6 (the figures are printed), and bit for bit the float32
statement (same operations, same order, no contraction) -- plus the exact properties:
singly covered elements keep their bits, covering windows agree bit for bit after a stitch, agreeing windows are left alone, the fold
is exactly 0.0 from a clip's length on, fold(unfold(x)) is x.  Every operand sits in front of a NaN-filled guard.
Overlaps: O in {1, 3, 4, W - 1} where 1 <= O <= W - 1; a one-frame window cannot overlap, so W == 1 runs at O == 0.

Loop: the seeded synthetic Xia model (181 features, ddim20, skip_timesteps=12: indices 7 .. 0) -- against ddim_sample_loop where every
clip fits one window, and against the same loop driven step by step from Python (one-step DenoiserEngine.sample_loop calls with
windows.stitch_ between them: the same kernels on the same operands in the same order), both bit for bit."""
import numpy as np
import pytest
import torch

import mst_amd  # noqa: F401
from mst_amd import synthetic as syn
from conftest import SEED
import window_fixture as wf

pytestmark = pytest.mark.gpu

GUARD = 4096


def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def guarded(values):
    """`values` on the GPU as a view of a buffer whose next GUARD elements are NaN -> (view, guard)."""
    v = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32))
    buf = torch.full((v.numel() + GUARD,), float("nan"), dtype=torch.float32, device=dev())
    buf[:v.numel()] = v.reshape(-1).to(dev())
    return buf[:v.numel()].view(v.shape), buf[v.numel():]


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------ kernels
def overlaps(W):
    return [0] if W == 1 else sorted({o for o in (1, 3, 4, W - 1) if 1 <= o <= W - 1})


def clip_lengths(W, O):
    """Mixed clips of one call: len < W, len == W, len == W + 1, and several windows with a shifted last one -- long enough that under
    O == W - 1 some frame is covered by W windows (len >= 2W - 1)."""
    S = W - O
    big = max(2 * W + 1, W + 2 * S + 1)
    if S > 1 and (big - W) % S == 0:
        big += 1                                  # the last window does not sit on the stride grid
    return ([max(1, W - 3)] if W > 1 else []) + [W, W + 1, big]


KERNEL_CASES = [(W, O, F) for W in (1, 5, 8, 64, 65, 196) for O in overlaps(W) for F in (1, 3, 263)]


@pytest.mark.parametrize("W,O,F", KERNEL_CASES, ids=[f"W{w}-O{o}-F{f}" for w, o, f in KERNEL_CASES])
def test_kernels_against_fixture(W, O, F):
    from mst_amd.diffusion.windows import WindowPlan, fold, stitch_, unfold
    lens = clip_lengths(W, O)
    L = max(lens) + 3                             # frames past every clip; L, W and the starts are no multiples of 4 in most cases
    plan = WindowPlan(lens, W, O, dev(), long_frames=L)
    win0, starts, clips = wf.plan(lens, W, O)
    assert np.array_equal(plan.clip_win0, win0) and np.array_equal(plan.win_start, starts) and np.array_equal(plan.win_clip, clips)
    assert plan.n_windows == len(starts) and plan.long_frames == L
    if O == W - 1 and W > 1:
        assert max(len(wf.covering(lens, win0, starts, W, len(lens) - 1, f)) for f in range(lens[-1])) == W
    rng = np.random.default_rng(SEED + 1000 * W + 10 * O + F)
    long_h = rng.standard_normal((len(lens), F, 1, L)).astype(np.float32)
    long_d, long_guard = guarded(long_h)

    # unfold: a gather, exact; zero padding past a clip
    win = unfold(long_d, plan)
    want = wf.unfold(long_h, lens, win0, starts, clips, W)
    assert same_bits(win.cpu(), torch.from_numpy(want))
    # fold(unfold(x)) == x below the length, exactly 0.0 from there on; the windows agree, so the stitch inside leaves them alone
    back = fold(win, plan).cpu().numpy()
    for c, n in enumerate(lens):
        assert np.array_equal(back[c, :, 0, :n].view(np.uint32), long_h[c, :, 0, :n].view(np.uint32)), c
        assert not back[c, :, 0, n:].any() and not np.signbit(back[c, :, 0, n:]).any(), c
    kept = win.clone()
    stitch_(kept, plan)
    assert same_bits(kept, win)                   # equal inputs stay bit-equal

    # independent windows; some keep their agreeing values (rule two beside rule three in one call): feature 0, or with a single
    # feature the windows of the len == W + 1 clip
    noisy_h = (want + rng.standard_normal(want.shape)).astype(np.float32)
    agree = np.zeros(want.shape[:2], bool)
    if F > 1:
        agree[:, 0] = True
    else:
        agree[clips == len(lens) - 2] = True
    noisy_h[agree] = want[agree]
    w_d, w_guard = guarded(noisy_h)
    l_d, l_guard = guarded(np.full((len(lens), F, 1, L), 7.0, np.float32))
    stitch_(w_d, plan, long_out=l_d)
    torch.cuda.synchronize()
    got_w, got_l = w_d.cpu().numpy(), l_d.cpu().numpy()
    for g in (long_guard, w_guard, l_guard):
        assert bool(torch.isnan(g).all())
    assert np.isfinite(got_w).all() and np.isfinite(got_l).all()
    s32, l32 = wf.stitch(noisy_h, lens, win0, starts, clips, W, L, np.float32)
    s64, l64 = wf.stitch(noisy_h, lens, win0, starts, clips, W, L, np.float64)
    for name, got, f32, f64 in (("windows", got_w, s32, s64), ("long", got_l, l32, l64)):
        ref_dev, e = wf.rel(f32, f64), wf.rel(got, f64)
        print(f"windows: W{W} O{O} F{F} {name} ref {ref_dev:.3e} got {e:.3e} bar {wf.bar(ref_dev):.3e} "
              f"(bitwise the float32 statement: {np.array_equal(got.view(np.uint32), f32.view(np.uint32))})")
        assert e <= wf.bar(ref_dev), name
        # stricter than the bar, from the arithmetic: the kernel forms the same products and sums in the same order with contraction
        # off, and fp32 division is correctly rounded on both sides, so it IS the float32 statement
        assert np.array_equal(got.view(np.uint32), f32.view(np.uint32)), name
    assert np.array_equal(got_w[agree].view(np.uint32), noisy_h[agree].view(np.uint32))        # agreeing windows: untouched
    assert W == 1 or not np.array_equal(got_w, noisy_h)                                        # ... and the others were averaged
    cover = np.zeros((len(starts), W), np.int32)
    for c, n in enumerate(lens):
        assert not got_l[c, :, 0, n:].any() and not np.signbit(got_l[c, :, 0, n:]).any(), c    # exactly 0.0 from len on
        for k in range(win0[c], win0[c + 1]):
            for j in range(win0[c], win0[c + 1]):
                lo, hi = max(starts[k], starts[j]), min(starts[k], starts[j]) + W
                if lo < min(hi, n):
                    cover[k, lo - starts[k]:min(hi, n) - starts[k]] += 1
            if k + 1 < win0[c + 1]:               # neighbours agree on what they share (every covering set is a run of neighbours)
                d = starts[k + 1] - starts[k]
                if d < W:
                    assert torch.equal(w_d[k, :, 0, d:], w_d[k + 1, :, 0, :W - d]), (c, k)
            i = np.arange(W)
            live = starts[k] + i < n
            assert np.array_equal(got_l[c][:, 0, starts[k] + i[live]].view(np.uint32), got_w[k][:, 0, i[live]].view(np.uint32))
    single = cover <= 1                           # covered by this window alone (or padding past the clip): bits kept
    pick = np.broadcast_to(single[:, None, :], got_w[:, :, 0, :].shape)
    assert pick.any() and np.array_equal(got_w.view(np.uint32)[:, :, 0, :][pick], noisy_h.view(np.uint32)[:, :, 0, :][pick])


def test_windows_refuse_bad_operands():
    from mst_amd.diffusion.windows import WindowPlan, stitch_, unfold
    plan = WindowPlan([9, 40], 16, 4, dev())
    assert plan.long_frames == 40 and plan.n_windows == 1 + 3 and list(plan.win_start) == [0, 0, 12, 24]
    assert list(plan.win_lengths) == [9, 16, 16, 16]
    with pytest.raises(ValueError, match="shape"):
        unfold(torch.zeros(2, 3, 1, 39, device=dev()), plan)
    with pytest.raises(ValueError, match="shape"):
        stitch_(torch.zeros(3, 3, 1, 16, device=dev()), plan)
    with pytest.raises(ValueError, match="float32"):
        unfold(torch.zeros(2, 3, 1, 40, device=dev(), dtype=torch.float64), plan)
    with pytest.raises(RuntimeError, match="long_frames 5000 outside"):
        WindowPlan([5000], 16, 4, dev())


# ------------------------------------------------------------------------------------------ loop
F_XIA, SKIP = 181, 12
PROMPTS = ["a person walks proudly", "an old man jumps", "a person walks proudly", "an old man jumps"]


@pytest.fixture(scope="module")
def xia():
    import loop_fixture as lf
    model, d = lf.build_model(dev())
    return model, d


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def long_inputs(tag, lens, L):
    """(noise, init image, kwargs) of C long clips, zero from each clip's length on (as the demo pads), with the root-trajectory
    inpainting pair of the sampler tests."""
    C = len(lens)
    live = np.zeros((C, 1, 1, L), np.float32)
    for c, n in enumerate(lens):
        live[c, ..., :n] = 1
    noise = syn.normal(SEED, f"win/{tag}/noise", (C, F_XIA, 1, L)) * live
    motion = syn.normal(SEED, f"win/{tag}/motion", (C, F_XIA, 1, L)) * live
    mask = syn.root_horizontal_mask(C, F_XIA, L) * live
    y = {"text": PROMPTS[:C], "mask": cu(live > 0), "lengths": torch.tensor(lens, device=dev()),
         "inpainting_mask": cu(mask.astype(np.float32)), "inpainted_motion": cu(motion.astype(np.float32))}
    return cu(noise.astype(np.float32)), cu(motion.astype(np.float32)), {"y": y}


def stepwise(d, model, plan, noise, init, kw, extra_y=None, dump=False):
    """The windowed loop driven from Python: q_sample on the long tensors, unfold, then per index ONE one-step sample_loop call on the
    windows and one stitch_.  -> (long, windows, [folded x0-hat per step])."""
    from mst_amd.diffusion.gaussian_diffusion import _unwrap
    from mst_amd.diffusion.windows import fold, stitch_, unfold
    from mst_amd.engine import SAMPLER_DDIM
    denoiser, cfg, _ = _unwrap(model)
    y = dict(kw["y"])
    idx = list(range(d.num_timesteps - SKIP))[::-1]
    t = torch.full((noise.shape[0],), idx[0], device=dev(), dtype=torch.long)
    x = unfold(d.q_sample(init, t, noise, model_kwargs=kw).contiguous(), plan)
    mask, motion = unfold(y["inpainting_mask"], plan), unfold(y["inpainted_motion"], plan)
    wc = plan.win_clip_tensor()
    yw = {"text": [y["text"][int(c)] for c in plan.win_clip]}
    for k in ("scale", "style"):
        if k in y:
            yw[k] = y[k][wc.to(y[k].device)]
    eng = denoiser.mst_engine(plan.n_windows * (2 if cfg is not None else 1), plan.window)
    denoiser.mst_prepare(eng, yw, cfg is not None)
    sch = d._schedule(dev())
    dumps = []
    for i in idx:
        res = eng.sample_loop(sch, x, i, i, SAMPLER_DDIM, eta=0.0, cfg=cfg is not None, scale=yw.get("scale") if cfg is not None else None,
                              mask=mask, motion=motion, mask_noise=True, clip_denoised=False, noise=None, seed=0, dump_xstart=dump)
        if dump:
            dumps.append(fold(res[1][0], plan))
        stitch_(x, plan)
    return fold(x, plan), x, dumps


def test_loop_single_windows_equal_plain_loop(xia):
    """(a) every clip fits one window: the windowed loop is ddim_sample_loop on the same init, noise and kwargs, bit for bit."""
    model, d = xia
    W = 16
    lens = [9, 16, 13]
    noise, init, kw = long_inputs("a", lens, W)
    got = d.ddim_sample_loop_windows(model, None, window=W, overlap=4, lengths=lens, noise=noise, clip_denoised=False, model_kwargs=kw,
                                     skip_timesteps=SKIP, init_image=init)
    ref = d.ddim_sample_loop(model, (len(lens), F_XIA, 1, W), noise=noise, clip_denoised=False, model_kwargs=kw, skip_timesteps=SKIP,
                             init_image=init)
    assert got.shape == ref.shape
    for c, n in enumerate(lens):
        assert torch.equal(got[c, :, :, :n], ref[c, :, :, :n]), c
        assert not got[c, :, :, n:].any(), c
    assert set(kw["y"]) == {"text", "mask", "lengths", "inpainting_mask", "inpainted_motion"}          # model_kwargs are not mutated
    assert kw["y"]["inpainted_motion"].shape[-1] == W


@pytest.mark.parametrize("W,O", [(16, 4), (16, 5), (17, 4), (17, 5)], ids=lambda v: str(v))
def test_loop_equals_stepwise(xia, W, O):
    """(b)-(e) lens 9, 16, 17 and 40 in one batch: the native loop is the step-by-step loop bit for bit -- the long sample, the windows,
    the folded x0-hat of every step; neighbours agree on shared frames; inpainted rows are the content's bits."""
    from mst_amd.diffusion.windows import WindowPlan
    model, d = xia
    lens = [9, 16, 17, 40]
    L = 40
    noise, init, kw = long_inputs(f"b{W}{O}", lens, L)
    plan = WindowPlan(lens, W, O, dev(), long_frames=L)
    assert plan.n_windows > len(lens)
    want_long, want_win, want_dump = stepwise(d, model, plan, noise, init, kw, dump=True)
    got_long, got_win = d.ddim_sample_loop_windows(model, (len(lens), F_XIA, 1, L), plan=plan, noise=noise, clip_denoised=False,
                                                   model_kwargs=kw, skip_timesteps=SKIP, init_image=init, return_windows=True)
    assert torch.equal(got_win, want_win) and torch.equal(got_long, want_long)
    assert bool(torch.isfinite(got_long).all())
    # (c) neighbours agree on the frames they share
    shared = 0
    for c in range(len(lens)):
        for k in range(plan.clip_win0[c], plan.clip_win0[c + 1] - 1):
            dlt = int(plan.win_start[k + 1] - plan.win_start[k])
            assert 0 < dlt < W
            assert torch.equal(got_win[k, :, 0, dlt:], got_win[k + 1, :, 0, :W - dlt]), (c, k)
            shared += W - dlt
    assert shared > 0
    # (d) inpainted rows: the content's bits, and zeros from the length on
    motion, mask = kw["y"]["inpainted_motion"], kw["y"]["inpainting_mask"]
    for c, n in enumerate(lens):
        rows = mask[c, :, 0, 0] > 0
        assert int(rows.sum()) >= 1
        assert torch.equal(got_long[c, rows, 0, :n], motion[c, rows, 0, :n]), c
        assert not got_long[c, :, :, n:].any(), c
    assert not torch.equal(got_long[:, 5:], init[:, 5:])                    # the free rows did move
    # (e) the x0-hat dump, folded per step
    dump = d.ddim_sample_loop_windows(model, (len(lens), F_XIA, 1, L), plan=plan, noise=noise, clip_denoised=False, model_kwargs=kw,
                                      skip_timesteps=SKIP, init_image=init, dump_all_xstart=True)
    assert len(dump) == len(want_dump) == d.num_timesteps - SKIP
    for j, (a, b) in enumerate(zip(dump, want_dump)):
        assert a.shape == (len(lens), F_XIA, 1, L) and torch.equal(a, b), j
    # ... also when the dump is cut into chunks of one step (the bound on the dump's size)
    old = d.noise_chunk_bytes
    try:
        d.noise_chunk_bytes = 1
        chunked, win2 = d.ddim_sample_loop_windows(model, (len(lens), F_XIA, 1, L), plan=plan, noise=noise, clip_denoised=False,
                                                   model_kwargs=kw, skip_timesteps=SKIP, init_image=init, dump_all_xstart=True,
                                                   return_windows=True)
    finally:
        d.noise_chunk_bytes = old
    assert all(torch.equal(a, b) for a, b in zip(chunked, want_dump)) and torch.equal(win2, want_win)


def test_loop_under_cfg(xia):
    """(f) ClassifierFreeSampleModel, two clips: the per-clip scale is gathered per window; equal to the step-by-step loop."""
    from mst_amd.diffusion.windows import WindowPlan
    from mst_amd.model.cfg_sampler import ClassifierFreeSampleModel
    model, d = xia
    lens, L, W, O = [17, 40], 40, 17, 5
    noise, init, kw = long_inputs("cfg", lens, L)
    kw["y"]["scale"] = torch.tensor([2.5, 1.5], device=dev())
    cfg_model = ClassifierFreeSampleModel(model)
    plan = WindowPlan(lens, W, O, dev(), long_frames=L)
    want_long, want_win, _ = stepwise(d, cfg_model, plan, noise, init, kw)
    got_long, got_win = d.ddim_sample_loop_windows(cfg_model, (2, F_XIA, 1, L), plan=plan, noise=noise, clip_denoised=False, model_kwargs=kw,
                                                   skip_timesteps=SKIP, init_image=init, return_windows=True)
    assert torch.equal(got_win, want_win) and torch.equal(got_long, want_long)
    plain = d.ddim_sample_loop_windows(model, (2, F_XIA, 1, L), plan=plan, noise=noise, clip_denoised=False, model_kwargs=kw,
                                       skip_timesteps=SKIP, init_image=init)
    assert not torch.equal(plain, got_long)                                 # the guidance did act


def test_loop_with_a_style_bank():
    """(f) a StyleBank of two styles, two clips of different styles: the style index is gathered per window; equal to the step-by-step
    loop, and each clip equals the same clip sampled with its style in both slots."""
    import style_fixture as sf
    from mst_amd.diffusion.windows import WindowPlan
    from mst_amd.model.mdm_forstyledataset import StyleDiffusion
    from mst_amd.model.style_bank import StyleBank
    from mst_amd.utils import model_util
    import loop_fixture as lf
    members = []
    for s in range(2):
        m = StyleDiffusion("", F_XIA, 1, 1, True, "rot6d", True, True, latent_dim=512, ff_size=1024, num_layers=8, num_heads=4,
                           dropout=0.1, activation="gelu", data_rep="hml_vec", cond_mode="text", cond_mask_prob=0.1,
                           arch="trans_enc", dataset="stylexia_posrot")
        missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in sf.style_weights(F_XIA, s).items()}, strict=False)
        assert not unexpected
        m.motion_enc.mdm_model.set_text_encoder(
            lambda texts: torch.stack([torch.from_numpy(syn.normal(SEED, "text/" + t, (512,))) for t in texts]))
        members.append(m.to(dev()).eval())
    bank = StyleBank(members)
    _, d, _ = model_util.creat_serval_diffusion(lf.diffusion_args(), StyleDiffusion, "ddim20")
    lens, L, W, O = [20, 45], 45, 20, 5                                     # (the style-aware kernels take clips of 17 .. 207 frames)
    noise, init, kw = long_inputs("bank", lens, L)
    plan = WindowPlan(lens, W, O, dev(), long_frames=L)
    res = {}
    for key, styles in (("mixed", [0, 1]), (0, [0, 0]), (1, [1, 1])):
        kw["y"]["style"] = torch.tensor(styles)
        res[key] = d.ddim_sample_loop_windows(bank, (2, F_XIA, 1, L), plan=plan, noise=noise, clip_denoised=False, model_kwargs=kw,
                                              skip_timesteps=SKIP, init_image=init)
    assert torch.equal(res["mixed"][0], res[0][0]) and torch.equal(res["mixed"][1], res[1][1])
    assert not torch.equal(res[0][1], res[1][1])                            # the styles do differ
    kw["y"]["style"] = torch.tensor([0, 1])
    want_long, _, _ = stepwise(d, bank, plan, noise, init, kw)
    assert torch.equal(res["mixed"], want_long)


def test_loop_refusals(xia):
    """(g) each refusal, by message."""
    from mst_amd import _native as N
    from mst_amd.diffusion.windows import WindowPlan
    from mst_amd.engine import SAMPLER_DDPM
    import ctypes as C
    model, d = xia
    lens, L, W, O = [9, 40], 40, 16, 4
    noise, init, kw = long_inputs("g", lens, L)
    plan = WindowPlan(lens, W, O, dev(), long_frames=L)
    call = lambda m=model, **k: d.ddim_sample_loop_windows(m, (2, F_XIA, 1, L), **{**dict(
        plan=plan, noise=noise, clip_denoised=False, model_kwargs=kw, skip_timesteps=SKIP, init_image=init), **k})
    with pytest.raises(ValueError, match="eta 0.5 must be 0"):
        call(eta=0.5)
    with pytest.raises(ValueError, match="cond_fn is not supported"):
        call(cond_fn=lambda x, t, **k: torch.zeros_like(x))
    with pytest.raises(ValueError, match="denoised_fn is not supported"):
        call(denoised_fn=lambda x: x)
    with pytest.raises(ValueError, match="not the native denoiser"):
        call(m=lambda x, t, **k: x)
    model.train()
    try:
        with pytest.raises(ValueError, match="training mode"):
            call()
    finally:
        model.eval()
    with pytest.raises(ValueError, match="window 224 is above the engine's limit of 223"):
        call(plan=None, window=224, overlap=8)
    with pytest.raises(ValueError, match="the plan is for 2 clips of 40 frames"):
        d.ddim_sample_loop_windows(model, (2, F_XIA, 1, 39), plan=plan, noise=noise[..., :39], model_kwargs=kw)
    # the library's own refusals (mst_sample_loop_windows)
    eng = model.mst_engine(plan.n_windows, W)
    sch = d._schedule(dev())
    x = torch.zeros(plan.n_windows, F_XIA, 1, W, device=dev())

    def native(batch=plan.n_windows, frames=W, sampler=1, eta=0.0):
        a = N.MstLoopArgs()
        a.batch, a.frames, a.sampler, a.eta, a.noise_mode, a.t_start, a.t_end = batch, frames, sampler, eta, 1, 3, 0
        a.x_dev = x.data_ptr()
        rc = N.lib().mst_sample_loop_windows(eng.handle, sch.handle, C.byref(a), plan.handle, N.stream_ptr(dev()))
        return rc, N.lib().mst_last_error().decode()
    for kwargs, what in ((dict(sampler=SAMPLER_DDPM), "sampler 0 is not MST_SAMPLER_DDIM"), (dict(sampler=3), "sampler 3 is not MST_SAMPLER_DDIM"),
                         (dict(eta=0.25), "eta 0.25 must be 0"), (dict(batch=plan.n_windows - 1), "is not the plan's window count 4"),
                         (dict(frames=W - 1), "frames 15 is not the plan's window 16")):
        rc, msg = native(**kwargs)
        assert rc != 0 and msg.startswith("mst_sample_loop_windows:") and what in msg, msg
    torch.cuda.synchronize()
    assert not x.any()                                                      # nothing ran


def test_plain_loop_unchanged_around_a_windowed_one(xia):
    """(h) the windowed loop leaves no state behind: a plain ddim_sample_loop before and after it gives the same bits."""
    model, d = xia
    T = 16
    noise, init, kw = long_inputs("h", [16, 16], T)
    plain = lambda: d.ddim_sample_loop(model, (2, F_XIA, 1, T), noise=noise, clip_denoised=False, model_kwargs=kw, skip_timesteps=SKIP,
                                       init_image=init)
    before = plain()
    lens, L = [9, 40], 40
    n2, i2, kw2 = long_inputs("h2", lens, L)
    out = d.ddim_sample_loop_windows(model, (2, F_XIA, 1, L), window=16, overlap=4, lengths=lens, noise=n2, clip_denoised=False,
                                     model_kwargs=kw2, skip_timesteps=SKIP, init_image=i2)
    assert bool(torch.isfinite(out).all())
    after = plain()
    assert torch.equal(before, after)
