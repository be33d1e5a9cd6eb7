"""The glue and elementwise kernels at the shapes where their loops change path, against float64 (tests/glue_fixture.py).

  masked_l2      k_masked_l2_fwd: 1024 threads, an 8-way unrolled main loop while i + 7 * 1024 < F * T and a tail behind it; the mask sum
                 strides T by 1024.  k_masked_l2_bwd: grid capped at 64 blocks.  Totals around every boundary, T = 1 and T > 1024.
  text_cosine    k_text_cosine: rows strided by 16 waves, columns by 64 lanes, the row terms summed from a 1024-entry LDS array.
  step backward  k_step_backward through FusedStepFn: sampler x blend x clip x which gradients arrive, t = 0 and the last index.
  grid stride    the stand-alone kernels cap their grid at 2048 x 256 threads: per_clip = 2048 * 256 + 777 runs the loop's second pass.
  recover_joints k_recover_from_ric: sequential scans, 256-thread strides, 5 * T * 4 bytes of dynamic LDS (the host refuses above the
                 device's limit).

Bars.  For every case the reference's own fp32 formula (torch ops on the CPU; oracle.postprocess / oracle.diffusion where they restate
it) is evaluated on the same inputs and its distance from the float64 closed form measured: relative L2, absolute for the scalar
text-cosine loss.  The kernel's bar is 4 x that distance (two fp32 evaluations differ in summation order) and not below 1e-6, the bar
tests/test_gpu_fused_ops.py already holds.  Bit-exact assertions (masked frames, saturated elements, blend rows) stay exact.
Every case prints `glue: <case> ref <fp32 reference deviation> got <kernel deviation> bar <bar>`; DESIGN.md section 5 has the table.

Operands of masked_l2 sit in front of a NaN-filled guard region of one unrolled sweep (8 * 1024 floats): a loop that runs one slab
too far reads NaN instead of a neighbour's values (or unmapped memory).

Worst figures measured on an MI355X, kernel / fp32 reference / bar (the table is in DESIGN.md section 5):
  masked_l2 loss 1.1e-7 / 8.9e-8 / 1e-6, d_b 5.1e-8 / 5.1e-8 / 1e-6;  text_cosine loss 6.7e-8 / 7.6e-8 / 1e-6 (absolute),
  d_m 9.4e-8 / 1.6e-7 / 1e-6, the parallel row 1.3e-7 / 2.4e-7 / 1e-6 (absolute);  step backward 2.9e-8 / 3.3e-8 / 1e-6;
  grid-stride second pass: DDIM step 1.2e-7 / 1.4e-7 / 1e-6, the others below 5e-8;
  recover_joints T <= 2: 5.1e-8 / 5.7e-8 / 1e-6, T = 257 (J = 21): 2.2e-5 / 2.1e-5 / 8.5e-5, T = 1024 (J = 21): 4.1e-5 / 4.0e-5 / 1.6e-4,
  T = 4096 (the LDS limit): 1.5e-3 / 1.5e-3 / 6.1e-3."""
import numpy as np
import pytest
import torch

import glue_fixture as gf
import mst_amd  # noqa: F401
import mst_amd.synthetic as syn
from mst_amd import _native as N
from mst_amd.engine import SAMPLER_DDIM, SAMPLER_DDPM, Schedule

pytestmark = pytest.mark.gpu
SEED = 60613
GUARD = 8 * 1024
GRID_PASS = 2048 * 256


def dev():
    return torch.device("cuda:0")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def report(case, ref, got, bar):
    print(f"glue: {case} ref {ref:.3e} got {got:.3e} bar {bar:.3e}")


def guarded(values):
    """`values` on the GPU as a view of a buffer whose next GUARD floats are NaN."""
    v = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32))
    buf = torch.full((v.numel() + GUARD,), float("nan"), dtype=torch.float32, device=dev())
    buf[:v.numel()] = v.reshape(-1).to(dev())
    return buf[:v.numel()].view(v.shape)


# ------------------------------------------------------------------------------------------ masked_l2
L2_CASES = [  # (F, T, n, per_sample) -- F * T is the total the forward kernel's two loops split
    (7, 1, 6, False), (7, 1, 1, True),                      # 7: T = 1, the tail alone, most threads idle
    (33, 31, 6, True),                                      # 1023: one short of a thread slab
    (32, 32, 6, False),                                     # 1024: exactly one slab
    (25, 41, 6, True),                                      # 1025
    (56, 128, 6, False), (7, 1024, 1, True),                # 7 * 1024: the unrolled loop's bound itself (i + 7 * 1024 < total is false)
    (67, 107, 6, True), (67, 107, 70, False),               # 7 * 1024 + 1: thread 0 alone takes the unrolled sweep
    (64, 128, 6, True),                                     # 8 * 1024: one full sweep, no tail
    (3, 2731, 6, False), (3, 2731, 6, True),                # 8 * 1024 + 1: a sweep and a one-element tail; T > 1024 for the mask sum
    (3, 1500, 6, True), (3, 1500, 1, False),                # T = 1500 with F = 3
    (181, 76, 6, True), (181, 76, 70, False),               # the Xia clip
    (263, 196, 6, False), (263, 196, 70, True),             # the HumanML clip: the backward grid's 64-block cap, 806 elements a thread
]


def l2_id(c):
    F, T, n, per = c
    return f"total{F * T}_F{F}xT{T}_n{n}_{'per_sample' if per else 'broadcast'}"


@pytest.mark.parametrize("case", L2_CASES, ids=l2_id)
def test_masked_l2_forward_and_backward(case):
    from mst_amd.diffusion.fused_ops import MaskedL2Fn
    F, T, n, per = case
    tag = l2_id(case)
    na = n if per else 1
    a_h = syn.normal(SEED, f"l2/a/{tag}", (na, F, 1, T))
    b_h = syn.normal(SEED, f"l2/b/{tag}", (n, F, 1, T))
    m_h = (syn.uniform(SEED, f"l2/m/{tag}", (na, 1, 1, T), 0.0, 1.0) > 0.35).astype(np.float64 if per else np.float32)
    m_h[..., 0] = 1.0                                       # no sample without a kept frame (the reference divides by the count)
    if per and n > 1:
        m_h[1] = 0.0
        m_h[1, ..., T // 2] = 1.0                           # one sample whose mask keeps a single frame
    g_h = syn.normal(SEED, f"l2/g/{tag}", (n,))
    want, want_db = gf.masked_l2(a_h, b_h, m_h), gf.masked_l2_grad_b(a_h, b_h, m_h, g_h)
    # the reference's formula in fp32 on the CPU, and its autograd
    at, bt, mt = (torch.from_numpy(np.ascontiguousarray(v)) for v in (a_h, b_h, m_h))
    bt.requires_grad_(True)
    ref = gf.masked_l2_torch(at.expand(n, -1, -1, -1), bt, mt.expand(n, -1, -1, -1))
    (ref * torch.from_numpy(g_h)).sum().backward()
    bar_l, bar_g = gf.bar(gf.rel(ref, want)), gf.bar(gf.rel(bt.grad, want_db))
    # the node: a float64 mask for the per-sample form (the training loader attaches one), stride-0 views for the broadcast form
    a = guarded(a_h).requires_grad_(per)
    b = guarded(b_h).requires_grad_(True)
    m = cu(m_h)
    got = MaskedL2Fn.apply(a if per else a.expand(n, -1, -1, -1), b, m if per else m.expand(n, -1, -1, -1))
    (got * cu(g_h)).sum().backward()
    e_l, e_g = gf.rel(got, want), gf.rel(b.grad, want_db)
    report(f"masked_l2 {tag} loss", gf.rel(ref, want), e_l, bar_l)
    report(f"masked_l2 {tag} d_b", gf.rel(bt.grad, want_db), e_g, bar_g)
    assert tuple(got.shape) == (n,) and bool(torch.isfinite(got).all()) and bool(torch.isfinite(b.grad).all())
    assert e_l <= bar_l
    assert e_g <= bar_g
    keep = torch.from_numpy(np.broadcast_to(m_h, (n, 1, 1, T)) != 0).to(dev()).expand(n, F, 1, T)
    assert float(b.grad[~keep].abs().max() if bool((~keep).any()) else 0.0) == 0.0          # masked frames: exactly zero
    if per:
        assert torch.equal(a.grad, -b.grad)
        if n > 1:
            assert int((b.grad[1] != 0).sum()) <= F and float(b.grad[1, :, :, T // 2].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------ text_cosine
COS_CASES = [(B, 512) for B in (1, 15, 16, 17, 63, 64, 65, 1024)] + [(17, D) for D in (1, 63, 64, 65, 768)]


@pytest.mark.parametrize("B,D", COS_CASES, ids=[f"B{B}_D{D}" for B, D in COS_CASES])
def test_text_cosine_forward_and_backward(B, D):
    from mst_amd.diffusion.fused_ops import TextCosineFn
    tag = f"B{B}_D{D}"
    f_h = syn.normal(SEED, f"cos/f/{tag}", (B, D))
    m_h = syn.normal(SEED, f"cos/m/{tag}", (B, D))
    # row norms spread over 1e-3 .. 1e3 (the term is scale-invariant), independently for the two operands
    f_h = (f_h * 10.0 ** syn.uniform(SEED, f"cos/sf/{tag}", (B, 1), -3.0, 3.0)).astype(np.float32)
    m_h = (m_h * 10.0 ** syn.uniform(SEED, f"cos/sm/{tag}", (B, 1), -3.0, 3.0)).astype(np.float32)
    if B >= 2 and D >= 2:                                   # one nearly parallel pair: 1 - c cancels to ~1e-8
        m_h[1] = (f_h[1].astype(np.float64) * 3.0 * (1.0 + 1e-4 * syn.normal(SEED, f"cos/par/{tag}", (D,)))).astype(np.float32)
    want, want_g = gf.text_cosine(f_h, m_h), gf.text_cosine_grad_m(f_h, m_h, 10.0)
    mt = torch.from_numpy(m_h).requires_grad_(True)
    ref = gf.text_cosine_torch(torch.from_numpy(f_h), mt)
    (ref * 10.0).backward()
    # gradient rows scale as 1 / |m_b| (six decades here): compared as d_m |m_b|, so that every row weighs alike and the cancelling
    # row is judged absolutely, on the scale of the others.  D = 1: c = +-1 and the gradient is identically zero -- absolute distance.
    w = np.linalg.norm(m_h.astype(np.float64), axis=1, keepdims=True)

    def gdist(g):
        g = gf.f64(g) * w
        return float(np.abs(g - want_g * w).max()) if D == 1 else gf.rel(g, want_g * w)
    ref_l, ref_g = abs(float(ref.detach()) - want), gdist(mt.grad)
    mu = cu(m_h).requires_grad_(True)
    got = TextCosineFn.apply(cu(f_h), mu)
    (got * 10.0).backward()
    e_l, e_g = abs(float(got.detach()) - want), gdist(mu.grad)
    report(f"text_cosine {tag} loss(abs)", ref_l, e_l, gf.bar(ref_l))
    report(f"text_cosine {tag} d_m", ref_g, e_g, gf.bar(ref_g))
    assert e_l <= gf.bar(ref_l)
    assert bool(torch.isfinite(mu.grad).all()) and e_g <= gf.bar(ref_g)
    if B >= 2 and D >= 2:                                   # the cancelling row on its own: 1 - c of ~1e-8 against an absolute bar
        f1, m1 = f_h[1:2], m_h[1:2]
        want1 = gf.text_cosine(f1, m1)
        assert want1 < 1e-6
        ref1 = abs(float(gf.text_cosine_torch(torch.from_numpy(f1), torch.from_numpy(m1))) - want1)
        e1 = abs(float(TextCosineFn.apply(cu(f1), cu(m1))) - want1)
        report(f"text_cosine {tag} parallel row(abs)", ref1, e1, gf.bar(ref1))
        assert e1 <= gf.bar(ref1)


def test_text_cosine_refuses_more_rows_than_its_row_array():
    from mst_amd.diffusion.fused_ops import TextCosineFn
    with pytest.raises(RuntimeError, match=r"mst_text_cosine: bad arguments \(batch 1\.\.1024\)"):
        TextCosineFn.apply(torch.ones(1025, 8, device=dev()), torch.ones(1025, 8, device=dev()))


# ------------------------------------------------------------------------------------------ the with-grad step's backward
_SCH = {}


def sched(respacing):
    if respacing not in _SCH:
        from oracle import schedule
        tab, tmap = schedule.make("cosine", 1000, respacing)
        _SCH[respacing] = (tab, Schedule(tab, tmap, dev()))
    return _SCH[respacing]


SAMPLERS = [("ddpm", False, 0.0), ("ddim_eta0", True, 0.0), ("ddim_eta0.5", True, 0.5)]


@pytest.mark.parametrize("respacing", ["ddim20", ""], ids=["ddim20", "steps1000"])
@pytest.mark.parametrize("F,T", [(150, 61), (24, 1)], ids=["150x61", "24x1"])
@pytest.mark.parametrize("name,ddim,eta", SAMPLERS, ids=[s[0] for s in SAMPLERS])
def test_step_backward_every_combination(name, ddim, eta, F, T, respacing):
    """{blend, no blend} x {clip, no clip} x {both gradients, g_sample only, g_pred only} at t = 0 and the last index."""
    from mst_amd.diffusion.fused_ops import FusedStepFn
    tab, sch = sched(respacing)
    B, last = 2, len(tab["betas"]) - 1
    shape = (B, F, 1, T)
    h = {k: syn.normal(SEED, f"sb/{k}/{F}", shape) for k in ("out", "x", "noise", "motion", "ws", "wp")}
    mask_h = syn.root_horizontal_mask(B, F, T)
    t_h = np.array([0, last])
    d = {k: cu(v) for k, v in h.items()}
    worst = (0.0, 0.0, "")
    for blend in (True, False):
        for clip in (True, False):
            for which in ("both", "g_sample", "g_pred"):
                case = f"step_backward {name} {respacing or 'steps1000'} {F}x{T} {'blend' if blend else 'noblend'} {'clip' if clip else 'noclip'} {which}"
                ws = h["ws"] if which != "g_pred" else None
                wp = h["wp"] if which != "g_sample" else None
                # fp32 torch autograd of the reference's step
                o = torch.from_numpy(h["out"]).requires_grad_(True)
                s_ref, p_ref = gf.step_torch(tab, torch.from_numpy(t_h), ddim, eta, o, torch.from_numpy(h["x"]), torch.from_numpy(h["noise"]),
                                             torch.from_numpy(mask_h) if blend else None, torch.from_numpy(h["motion"]) if blend else None, clip)
                loss = 0.0
                if ws is not None:
                    loss = loss + (s_ref * torch.from_numpy(ws)).sum()
                if wp is not None:
                    loss = loss + (p_ref * torch.from_numpy(wp)).sum()
                loss.backward()
                # the node
                o2 = d["out"].clone().requires_grad_(True)
                s2, p2 = FusedStepFn.apply(o2, d["x"], cu(t_h), d["noise"], cu(mask_h) if blend else None, d["motion"] if blend else None,
                                           sch, SAMPLER_DDIM if ddim else SAMPLER_DDPM, eta, True, clip)
                loss2 = 0.0
                if ws is not None:
                    loss2 = loss2 + (s2 * d["ws"]).sum()
                if wp is not None:
                    loss2 = loss2 + (p2 * d["wp"]).sum()
                loss2.backward()
                assert torch.equal(p2.detach().cpu(), p_ref.detach())                       # blend and clamp are exact
                want = gf.step_d_out(tab, t_h, ddim, eta, ws, wp, mask_h if blend else None, p_ref.detach() if clip else None)
                dev_ref, e = gf.rel(o.grad, want), gf.rel(o2.grad, want)
                bar = gf.bar(dev_ref)
                report(case, dev_ref, e, bar)
                assert e <= bar, case
                if e > worst[0]:
                    worst = (e, dev_ref, case)
                if blend:
                    assert float(o2.grad[:, :3].abs().max()) == 0.0, case                  # inpainted rows take no gradient
                if clip:
                    sat = p2.detach().abs() >= 1.0
                    assert bool(sat.any()) and float(o2.grad[sat].abs().max()) == 0.0, case  # saturated elements take none
                    assert float(o2.grad[~sat].abs().max()) > 0.0
    report(f"step_backward {name} {respacing or 'steps1000'} {F}x{T} WORST ({worst[2]})", worst[1], worst[0], gf.bar(worst[1]))


# ------------------------------------------------------------------------------------------ the grid-stride loop
def test_grid_stride_second_pass():
    """per_clip = 2048 * 256 + 777: the step kernels' grid is capped at 2048 blocks of 256 threads, so elements from 2048 * 256 on are
    written by the loop's second pass.  That slice is asserted on its own."""
    from mst_amd.diffusion.fused_ops import FusedStepFn
    from oracle import diffusion
    tab, sch = sched("ddim20")
    P = GRID_PASS + 777
    shape = (2, P, 1, 1)
    h = {k: syn.normal(SEED, f"gs/{k}", shape) for k in ("out", "x", "noise", "motion", "ws", "wp")}
    mask_h = (syn.uniform(SEED, "gs/mask", shape, 0.0, 1.0) > 0.7).astype(np.float32)
    t_h = np.array([7, 19])
    d = {k: cu(v) for k, v in h.items()}
    tt, th = cu(t_h), torch.from_numpy(t_h)
    T64 = lambda k: torch.from_numpy(h[k]).double()
    m64 = torch.from_numpy(mask_h).double()
    tail = (slice(None), slice(GRID_PASS, None))

    def check(case, got, ref, want):
        for part, sl in (("all", (slice(None),)), ("second pass", tail)):
            dev_ref, e = gf.rel(ref[sl], want[sl]), gf.rel(got[sl], want[sl])
            report(f"grid_stride {case} {part}", dev_ref, e, gf.bar(dev_ref))
            assert bool(torch.isfinite(got[sl]).all()) and e <= gf.bar(dev_ref), (case, part)
    # q_sample
    ex = lambda name: torch.from_numpy(tab[name])[th].view(-1, 1, 1, 1)
    want = ex("sqrt_alphas_cumprod") * T64("motion") + ex("sqrt_one_minus_alphas_cumprod") * (T64("noise") * (1 - m64))
    check("q_sample", sch.q_sample(d["motion"], tt, d["noise"], cu(mask_h)).cpu(),
          diffusion.q_sample(tab, h["motion"], th, h["noise"], mask_h), want)
    # the steps
    for name, ddim, eta in (("ddpm", False, 0.0), ("ddim_eta0.5", True, 0.5)):
        s64, p64 = gf.step_torch(tab, th, ddim, eta, T64("out"), T64("x"), T64("noise"), m64, T64("motion"), False, dtype=torch.float64)
        o = (diffusion.ddim_sample(tab, h["out"], h["x"], th, h["noise"], eta=eta, inpainting=True, inpainting_mask=mask_h,
                                   inpainted_motion=h["motion"]) if ddim else
             diffusion.p_sample(tab, h["out"], h["x"], th, h["noise"], inpainting=True, inpainting_mask=mask_h, inpainted_motion=h["motion"]))
        s, p = sch.step(d["out"], d["x"], tt, d["noise"], SAMPLER_DDIM if ddim else SAMPLER_DDPM, eta, mask=cu(mask_h), motion=d["motion"],
                        mask_noise=True)
        check(f"step {name} sample", s.cpu(), o["sample"], s64)
        assert torch.equal(p.cpu(), o["pred_xstart"])
        keep = torch.from_numpy(mask_h[tail] != 0)
        assert torch.equal(p.cpu()[tail][keep], torch.from_numpy(h["motion"])[tail][keep])      # the blend, bit-exact, in the second pass
        # mst_step_backward on the same shape
        o1 = torch.from_numpy(h["out"]).requires_grad_(True)
        s_ref, p_ref = gf.step_torch(tab, th, ddim, eta, o1, torch.from_numpy(h["x"]), torch.from_numpy(h["noise"]), torch.from_numpy(mask_h),
                                     torch.from_numpy(h["motion"]), False)
        ((s_ref * torch.from_numpy(h["ws"])).sum() + (p_ref * torch.from_numpy(h["wp"])).sum()).backward()
        o2 = d["out"].clone().requires_grad_(True)
        s2, p2 = FusedStepFn.apply(o2, d["x"], tt, d["noise"], cu(mask_h), d["motion"], sch, SAMPLER_DDIM if ddim else SAMPLER_DDPM, eta, True, False)
        ((s2 * d["ws"]).sum() + (p2 * d["wp"]).sum()).backward()
        check(f"step_backward {name}", o2.grad.cpu(), o1.grad, torch.from_numpy(gf.step_d_out(tab, t_h, ddim, eta, h["ws"], h["wp"], mask_h)))
        assert float(o2.grad.cpu()[tail][keep].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ recover_joints
def _recover_case(T, J, F, tag):
    from mst_amd.utils.motion_process import recover_joints
    from oracle import postprocess
    B = 2
    sample = syn.normal(SEED, f"rj/{tag}/sample", (B, F, 1, T))
    mean = (syn.normal(SEED, f"rj/{tag}/mean", (F,)) * 0.3).astype(np.float32)
    std = syn.uniform(SEED, f"rj/{tag}/std", (F,), 0.2, 1.5).astype(np.float32)
    want = gf.recover_joints(sample, mean, std, J)
    ref = postprocess.recover_joints(sample, mean, std, J)
    got = recover_joints(cu(sample), mean, std, J)
    assert tuple(got.shape) == (B, 1, T, J, 3) == want.shape
    dev_ref, e = gf.rel(ref, want), gf.rel(got, want)
    report(f"recover_joints {tag}", dev_ref, e, gf.bar(dev_ref))
    assert bool(torch.isfinite(got).all()) and e <= gf.bar(dev_ref)
    assert torch.equal(got[:, 0, 0, 0, [0, 2]].cpu(), torch.zeros(B, 2))                     # the root starts at the origin, exactly


@pytest.mark.parametrize("J,F", [(22, 263), (21, 251)], ids=["J22", "J21"])
@pytest.mark.parametrize("T", [1, 2, 255, 256, 257, 1024])
def test_recover_joints_frame_counts(T, J, F):
    _recover_case(T, J, F, f"T{T}_J{J}")


def test_recover_joints_lds_limit():
    """The kernel asks for 5 * T * 4 bytes of dynamic LDS: the largest T that can launch follows from the device's shared memory per
    block (and the wrapper's own cap of 4096).  The host refuses anything above it; the limit itself runs."""
    from mst_amd.utils.motion_process import recover_joints
    limit = int(N.lib().mst_recover_max_frames())
    props = torch.cuda.get_device_properties(dev())
    per_block = getattr(props, "shared_memory_per_block", None)
    print(f"glue: recover_joints limit {limit} frames, shared memory per block {per_block}")
    assert 1024 <= limit <= 4096
    if per_block is not None:
        assert limit == min(4096, int(per_block) // (5 * 4))
    J, F = 22, 67
    x = torch.zeros(1, F, 1, limit + 1, device=dev())
    with pytest.raises(RuntimeError, match=rf"mst_recover_from_ric: frames {limit + 1} > {limit}"):
        recover_joints(x, np.zeros(F, np.float32), np.ones(F, np.float32), J)
    _recover_case(limit, J, F, f"T{limit}_limit")
