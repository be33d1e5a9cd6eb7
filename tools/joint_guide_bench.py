"""Joint-space guidance: what it costs.  HumanML shape, 64 x (263, 1, 196), 22 joints, dense weights, same box, interleaved:

  likelihood   (a) kernel  -- engine.joint_guide: logp and d logp / d x0 in one launch (csrc/mst_jguide.h)
               (b) torch   -- the same likelihood in torch ops under autograd on the device (tests/joint_guide_fixture.py: two cumsums,
                              index puts, qrot, and their backward), the form a hand-written cond_fn would take
  DDIM step    (c) no-grad -- ddim_sample on the native denoiser (one step of the sampling path)
               (d) with-grad, unguided -- ddim_sample_with_grad: the native training node's forward, the step node
               (e) with-grad, JointGuide -- (d) plus the kernel, the input-gradient-only backward and the guided step kernel

Each is warmed up, then timed `--reps` times in alternation over `--iters` calls per window with device events around a synchronised
window; medians.  (a) and (b) are compared on their outputs first (relative L2 of the gradients).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=196)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--step-iters", type=int, default=10)
    args = ap.parse_args()
    import numpy as np
    import torch
    import mst_amd  # noqa: F401
    import joint_guide_fixture as jf
    from mst_amd import engine
    from mst_amd import synthetic as syn
    from mst_amd.diffusion import gaussian_diffusion as gd
    from mst_amd.diffusion.guidance import JointGuide
    from mst_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    from mst_amd.model.mdm_forstyledataset import StyleDiffusion

    if not torch.cuda.is_available():
        raise SystemExit("joint_guide_bench needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    B, F, T, J = args.batch, 263, args.frames, 22
    case = jf.make_case(J, F, T, B, "dense")
    cu = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
    ops = {k: cu(case[k]) for k in ("x0", "mean", "std", "target", "weight", "scale")}
    lengths = torch.full((B,), T, device=dev, dtype=torch.int32)

    def timed(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    def kernel():
        return engine.joint_guide(ops["x0"], ops["mean"], ops["std"], J, ops["target"], ops["weight"], ops["scale"], lengths=lengths)

    def torch_ops():
        x0 = ops["x0"].detach().requires_grad_()
        logp, _ = jf.log_prob(x0, ops["mean"], ops["std"], J, ops["target"], ops["weight"], ops["scale"], lengths)
        return logp, torch.autograd.grad(logp.sum(), x0)[0]

    (lk, gk), (lt, gt) = kernel(), torch_ops()
    gap = float((gk - gt).norm() / gt.norm())
    for fn in (kernel, torch_ops):
        timed(fn, 5)
    ms = {"kernel": [], "torch": []}
    for _ in range(args.reps):
        ms["kernel"].append(timed(kernel, args.iters))
        ms["torch"].append(timed(torch_ops, args.iters))

    # ---- one DDIM step
    m = StyleDiffusion("", F, 1, 1, True, "rot6d", True, True, latent_dim=512, ff_size=1024, num_layers=8, num_heads=4, dropout=0.1,
                       activation="gelu", data_rep="hml_vec", cond_mode="text", cond_mask_prob=0.0, arch="trans_enc", dataset="humanml")
    sd = {k: torch.from_numpy(syn.tensor_for(3, k, tuple(v.shape)).copy()) for k, v in m.state_dict().items()
          if not k.endswith(".pe") and "clip_model" not in k}
    m.load_state_dict(sd, strict=False)
    m = m.to(dev).eval()
    d = SpacedDiffusion(use_timesteps=space_timesteps(1000, "ddim20"), betas=gd.get_named_beta_schedule("cosine", 1000),
                        model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE)
    guide = JointGuide(case["target"], case["weight"], case["mean"], case["std"], J, scale=case["scale"])
    x = cu(syn.normal(1, "jgb/x", (B, F, 1, T)))
    t = torch.full((B,), 10, device=dev, dtype=torch.long)
    kw = {"y": {"text_embed": cu(syn.normal(1, "jgb/txt", (B, 512))), "lengths": lengths}}

    def no_grad():
        with torch.no_grad():
            return d.ddim_sample(m, x, t, model_kwargs=kw)

    def with_grad():
        return d.ddim_sample_with_grad(m, x, t, model_kwargs=kw)

    def guided():
        return d.ddim_sample_with_grad(m, x, t, cond_fn=guide, model_kwargs=kw)

    steps = {"no_grad": no_grad, "with_grad": with_grad, "guided": guided}
    for fn in steps.values():
        timed(fn, 3)
    sm = {k: [] for k in steps}
    for _ in range(args.reps):
        for k, fn in steps.items():
            sm[k].append(timed(fn, args.step_iters))
    assert all(p.grad is None for p in m.parameters())
    med = lambda v: statistics.median(v)
    r = lambda v: round(v, 4)
    print(json.dumps({
        "shape": [B, F, 1, T], "joints": J, "reps": args.reps, "iters": args.iters, "step_iters": args.step_iters,
        "kernel_ms": r(med(ms["kernel"])), "kernel_all_ms": [r(v) for v in ms["kernel"]],
        "torch_ops_ms": r(med(ms["torch"])), "torch_ops_all_ms": [r(v) for v in ms["torch"]],
        "torch_over_kernel": round(med(ms["torch"]) / med(ms["kernel"]), 1), "grad_rel_l2_kernel_vs_torch": float(f"{gap:.3e}"),
        "logp_rel": float(f"{float(((lk - lt.detach()).abs() / lt.detach().abs()).max()):.3e}"),
        "ddim_step_no_grad_ms": r(med(sm["no_grad"])), "ddim_step_with_grad_ms": r(med(sm["with_grad"])),
        "ddim_step_guided_ms": r(med(sm["guided"])), "step_all_ms": {k: [r(v) for v in vs] for k, vs in sm.items()},
        "guided_over_with_grad": round(med(sm["guided"]) / med(sm["with_grad"]), 3),
        "guided_over_no_grad": round(med(sm["guided"]) / med(sm["no_grad"]), 3)}))


if __name__ == "__main__":
    main()
