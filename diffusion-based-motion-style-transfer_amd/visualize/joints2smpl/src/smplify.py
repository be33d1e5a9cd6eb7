"""SMPLify-3D on the GPU: `guess_init_3d` and `SMPLify3D` of the reference's visualize/joints2smpl/src/smplify.py with its interface
and its schedule, over one native evaluation of the objective and its gradient (csrc/mst_smplify.h, `mst_smplify_objective`).

The reference's closure runs a full smplx forward pass (6890 vertices), the loss functions of customloss.py and an autograd backward
pass.  Here the closure is ONE call: parameters in, the loss on the device and the parameters' `.grad` out.  customloss.py is not
mirrored function by function -- the objective is fused from the parameters to the loss.  The optimisers are torch.optim's LBFGS
(strong-Wolfe) and Adam, as plumbing; their schedule is the reference's: stage 1 (camera translation and global orientation) is 10
`step(closure)` calls of LBFGS(max_iter=num_iters) or 20 Adam steps, stage 2 (body pose, betas when seq_ind == 0, orientation, camera)
is num_iters such calls or num_iters Adam steps; joint weight 600, preserve weight 5 under L-BFGS, 0 under Adam and in the final loss.

The Rodrigues form of the objective is smplx's batch_rodrigues AS RECALLED, `RODRIGUES_FORM_UNVERIFIED` below: smplx is not installed
where this was written, so the form could not be checked against it.  It is stated in one place in the kernel (fit_rodrigues) and in
one place in the tests (tests/smplify_fixture.py).  The final vertices come from the existing SMPL forward pass fed the kernel's own
rotation matrices, so they are the vertices of the same form.

Not covered: use_collision=True (mesh_intersection), fitting several clips in one optimiser (L-BFGS's line search couples a clip's
frames, so that would change results)."""
import ctypes as C

import torch

from .... import _native as N
from ....model.smpl import NUM_BETAS, NUM_JOINTS, NUM_VERTEX_IDS, SMPL, SMPLBody, _up256
from . import config
from .prior import MaxMixturePrior

RODRIGUES_FORM_UNVERIFIED = "a = |theta + 1e-8|, d = theta / a, K = skew(d), R = I + sin(a) K + (1 - cos(a)) K K"
STAGES = {"camera": 0, "body": 1, 0: 0, 1: 1}
# body_fitting_loss_3d's defaults and what smplify.py:226-272 passes; `depth` is camera_fitting_loss_3d's 100, doubled because the
# reference's broadcast adds the depth term once per selected joint (four times) before the sum
BODY_WEIGHTS = {"sigma": 100.0, "joint": 600.0, "prior": 4.78 * 1.5, "angle": 15.2, "shape": 5.0, "keep": 5.0, "depth": 0.0}
CAMERA_WEIGHTS = {"sigma": 100.0, "joint": 0.0, "prior": 0.0, "angle": 0.0, "shape": 0.0, "keep": 0.0, "depth": 2 * 100.0}
GRADS = ("body_pose", "betas", "global_orient", "camera_translation")
_CATEGORIES = {"orig": 24, "AMASS": 22}


def _torso(joints_category):
    table = {"orig": config.JOINT_MAP, "AMASS": config.AMASS_JOINT_MAP}[joints_category]
    return [config.JOINT_MAP[j] for j in config.TORSO_JOINTS], [table[j] for j in config.TORSO_JOINTS]


@torch.no_grad()
def guess_init_3d(model_joints, j3d, joints_category="orig"):
    """The camera translation that brings the model's four torso joints onto the targets' (smplify.py:19-40): [N, 3]."""
    if joints_category not in _CATEGORIES:
        raise ValueError(f"guess_init_3d: joints_category {joints_category!r} is neither 'orig' nor 'AMASS'")
    gt, cat = _torso(joints_category)
    return (j3d[:, cat] - model_joints[:, gt]).sum(dim=1) / 4.0


class SMPLify3D:
    """Implementation of SMPLify, use 3D joints.  `smplxmodel`: the package's `model.smpl.SMPL` or an `SMPLBody`; `pose_prior`: a
    `MaxMixturePrior` (the user's gmm_08.pkl)."""

    def __init__(self, smplxmodel, step_size=1e-2, batch_size=1, num_iters=100, use_collision=False, use_lbfgs=True,
                 joints_category="orig", device=torch.device("cuda:0"), *, pose_prior):
        if use_collision:
            raise NotImplementedError("SMPLify3D: use_collision=True needs mesh_intersection's BVH and penetration loss, which are not covered")
        if isinstance(smplxmodel, SMPLBody):
            smplxmodel = SMPL(smplxmodel)
        if not isinstance(smplxmodel, SMPL):
            raise TypeError("SMPLify3D: smplxmodel is the package's model.smpl.SMPL or an SMPLBody; no body model is bundled and smplx is not used")
        if not isinstance(pose_prior, MaxMixturePrior):
            raise TypeError("SMPLify3D: pose_prior= is a MaxMixturePrior (from_pkl / from_arrays); no prior file is bundled")
        if joints_category not in _CATEGORIES:
            raise ValueError(f"SMPLify3D: joints_category {joints_category!r} is neither 'orig' nor 'AMASS'")
        if int(num_iters) < 1 or int(batch_size) < 1:
            raise ValueError(f"SMPLify3D: num_iters {num_iters} and batch_size {batch_size} are at least 1")
        self.batch_size, self.device, self.step_size, self.num_iters = int(batch_size), torch.device(device), float(step_size), int(num_iters)
        self.use_lbfgs, self.use_collision, self.pose_prior = bool(use_lbfgs), False, pose_prior
        self.smpl, self.body, self.joints_category = smplxmodel, smplxmodel.body, joints_category
        self.model_faces = torch.as_tensor(smplxmodel.faces).reshape(-1)
        self.num_joints = _CATEGORIES[joints_category]
        self.smpl_index = self.corr_index = range(self.num_joints)
        self.native_seconds = None               # set by __call__(time_native=True): host seconds spent inside the native entry

    # ------------------------------------------------------------------ one native evaluation
    def objective(self, stage, body_pose, global_orient, betas, camera_translation, j3d, *, conf_3d=1.0, preserve_pose=None,
                  camera_estimate=None, weights=None, want=GRADS, out=None, rotations=False, joints=False, total=True):
        """-> (loss, per_frame [N], grads).  stage 'camera' or 'body'.  body_pose [N, 69], global_orient [N, 3], betas [N, 10],
        camera_translation [N, 3] or [N, 1, 3], j3d [N, nj, 3] (nj = 22 for 'AMASS', 24 for 'orig'), conf_3d a scalar or [nj],
        preserve_pose [N, 69] (body), camera_estimate [N, 3] or [N, 1, 3] (camera): contiguous float32 tensors on one CUDA device.
        `weights`: overrides of BODY_WEIGHTS / CAMERA_WEIGHTS.  `want`: the gradients to compute, by parameter name; the camera stage
        has those of global_orient and camera_translation only.  `out`: name -> a buffer to write that gradient into.  grads: name
        -> tensor in the parameter's shape, plus 'rotations' [N, 24, 3, 3] and 'joints' [N, 24, 3] (the posed joints, no camera
        translation) when asked for.  total=False skips the second launch; loss is then None.  One launch (two with the total) on
        the current stream; nothing synchronises."""
        what = "SMPLify3D.objective"
        if stage not in STAGES:
            raise ValueError(f"{what}: stage {stage!r} is neither 'camera' nor 'body'")
        st = STAGES[stage]
        for name, t in (("body_pose", body_pose), ("global_orient", global_orient), ("betas", betas), ("camera_translation", camera_translation),
                        ("j3d", j3d)):
            if not torch.is_tensor(t):
                raise TypeError(f"{what}: {name} is a tensor")
        if not body_pose.is_cuda:
            raise RuntimeError(f"{what} runs on the GPU only (no CPU fallback); move the parameters to cuda")
        dev, n, nj = body_pose.device, body_pose.shape[0], self.num_joints

        def checked(name, t, shape):
            if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n * shape[0] * (shape[1] if len(shape) > 1 else 1):
                raise ValueError(f"{what}: {name} of shape {tuple(t.shape)}, {t.dtype} on {t.device}; expected contiguous float32 [{n}, {', '.join(map(str, shape))}] on {dev}")
            return t.detach()
        if n < 1:
            raise ValueError(f"{what}: {n} frames")
        pose, orient = checked("body_pose", body_pose, (69,)), checked("global_orient", global_orient, (3,))
        bet, cam = checked("betas", betas, (NUM_BETAS,)), checked("camera_translation", camera_translation, (3,))
        tgt = checked("j3d", j3d, (nj, 3))
        want = tuple(want)
        for w_ in want:
            if w_ not in GRADS:
                raise ValueError(f"{what}: no gradient named {w_!r}; the parameters are {GRADS}")
        w = dict(BODY_WEIGHTS if st else CAMERA_WEIGHTS)
        for k, v in (weights or {}).items():
            if k not in w:
                raise ValueError(f"{what}: no weight named {k!r}; the weights are {sorted(w)}")
            w[k] = float(v)
        conf = pres = est = packed = None
        if st:
            if torch.is_tensor(conf_3d) and conf_3d.numel() > 1:
                if conf_3d.numel() != nj:
                    raise ValueError(f"{what}: conf_3d of {conf_3d.numel()} values, expected a scalar or one per target joint ({nj})")
                conf = conf_3d.detach().to(device=dev, dtype=torch.float32).reshape(nj).contiguous()
            else:
                conf = torch.full((nj,), float(conf_3d), dtype=torch.float32, device=dev)
            if preserve_pose is None:
                if w["keep"] != 0.0:
                    raise ValueError(f"{what}: the body stage keeps the pose near preserve_pose (weight {w['keep']}); pass it, or weights={{'keep': 0}}")
                preserve_pose = pose
            pres = checked("preserve_pose", preserve_pose, (69,))
            packed = self.pose_prior.packed(dev)
        else:
            if camera_estimate is None:
                raise ValueError(f"{what}: the camera stage needs camera_estimate")
            est = checked("camera_estimate", camera_estimate, (3,))
            if "body_pose" in want or "betas" in want:
                want = tuple(x for x in want if x in ("global_orient", "camera_translation"))
        shapes = {"body_pose": pose.shape, "betas": bet.shape, "global_orient": orient.shape, "camera_translation": cam.shape}
        grads = {}
        for name in want:
            buf = (out or {}).get(name)
            if buf is None:
                buf = torch.empty(shapes[name], dtype=torch.float32, device=dev)
            else:
                checked(f"out[{name!r}]", buf, (shapes[name].numel() // n,))
            grads[name] = buf
        lib, body = N.lib(), self.body._state(dev)
        per = torch.empty(n, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev) if total else None
        nbytes = int(lib.mst_smplify_workspace_bytes(n))
        if nbytes < 0:
            N.check(1)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rot = torch.empty(n, NUM_JOINTS, 3, 3, dtype=torch.float32, device=dev) if rotations else None
        par = (C.c_int32 * NUM_JOINTS)(*[int(a) for a in self.body.parents])
        wt = N.MstSmplifyWeights(*[w[k] for k in ("sigma", "joint", "prior", "angle", "shape", "keep", "depth")])
        with torch.cuda.device(dev):
            N.check(lib.mst_smplify_objective(st, nj, n, N.ptr(pose), N.ptr(orient), N.ptr(bet), N.ptr(cam), N.ptr(tgt), N.ptr(conf), N.ptr(pres),
                                              N.ptr(est), N.ptr(body["J0"]), N.ptr(body["Jdirs"]), par, N.ptr(packed), C.byref(wt), N.ptr(ws),
                                              N.ptr(per), N.ptr(loss), N.ptr(grads.get("body_pose")), N.ptr(grads.get("global_orient")),
                                              N.ptr(grads.get("betas")), N.ptr(grads.get("camera_translation")), N.ptr(rot),
                                              N.stream_ptr(dev)))
        if rotations:
            grads["rotations"] = rot
        if joints:
            grads["joints"] = ws[:n * NUM_JOINTS * 12].view(torch.float32).view(n, NUM_JOINTS, 3)
        return loss, per, grads

    # ------------------------------------------------------------------ the fit
    def _forward(self, rot, betas):
        """The existing SMPL forward pass on rotation matrices -> (vertices [N, V, 3], joints [N, 45, 3]): smplx's joint list."""
        n, V = rot.shape[0], self.body.num_vertices
        every = list(range(NUM_JOINTS + NUM_VERTEX_IDS))
        x = rot.reshape(n, NUM_JOINTS, 9).contiguous()
        joints, _, ws = self.body.run(x, (0, 9, 1, NUM_JOINTS * 9), None, n, 1, n, NUM_JOINTS, "rotmat", True, None, betas, 0.0, -1, "all",
                                      joint_map=every, root=-1)
        verts = ws[ws.numel() - _up256(n * V * 12):][:n * V * 12].view(torch.float32).view(n, V, 3).clone()
        return verts, joints[0].permute(2, 0, 1).contiguous()

    def __call__(self, init_pose, init_betas, init_cam_t, j3d, conf_3d=1.0, seq_ind=0, time_native=False):
        """Perform body fitting: init_pose [N, 72], init_betas [N, 10], init_cam_t (unused, as in the reference: the start is
        guess_init_3d's), j3d [N, >= nj, 3] -> (vertices [N, V, 3], joints [N, 45, 3], pose [N, 72], betas [N, 10], camera_translation
        [N, 1, 3], final_loss)."""
        what = "SMPLify3D"
        if not (torch.is_tensor(init_pose) and torch.is_tensor(init_betas) and torch.is_tensor(j3d)):
            raise TypeError(f"{what}: init_pose, init_betas and j3d are tensors")
        if not j3d.is_cuda:
            raise RuntimeError(f"{what} runs on the GPU only (no CPU fallback); move the joints to cuda")
        dev, nj = j3d.device, self.num_joints
        n = j3d.shape[0]
        if j3d.dim() != 3 or j3d.shape[1] < nj or j3d.shape[2] != 3:
            raise ValueError(f"{what}: j3d of shape {tuple(j3d.shape)}, expected [N, >= {nj}, 3] for joints_category {self.joints_category!r}")
        if tuple(init_pose.shape) != (n, 72) or tuple(init_betas.shape) != (n, NUM_BETAS):
            raise ValueError(f"{what}: init_pose {tuple(init_pose.shape)} and init_betas {tuple(init_betas.shape)}, expected [{n}, 72] and [{n}, {NUM_BETAS}]")
        f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous().clone()
        body_pose, global_orient, betas = f32(init_pose[:, 3:]), f32(init_pose[:, :3]), f32(init_betas)
        target = f32(j3d[:, :nj])
        preserve_pose = body_pose.clone()
        spent = [0.0]

        def evaluate(*a, **k):
            if not time_native:
                return self.objective(*a, **k)
            import time
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            r = self.objective(*a, **k)
            torch.cuda.synchronize(dev)
            spent[0] += time.perf_counter() - t0
            return r
        zero_cam = torch.zeros(n, 3, dtype=torch.float32, device=dev)
        _, _, g = evaluate("camera", body_pose, global_orient, betas, zero_cam, target, camera_estimate=zero_cam, want=(), joints=True, total=False)
        init_cam_t = guess_init_3d(g["joints"], target, self.joints_category).unsqueeze(1).contiguous()
        camera_translation = init_cam_t.clone()
        params = {"body_pose": body_pose, "betas": betas, "global_orient": global_orient, "camera_translation": camera_translation}

        def run(stage, names, steps, **kw):
            """`steps` optimiser steps over the parameters `names`; the closure is one native evaluation that fills their .grad."""
            opt_params = [params[k] for k in names]
            for p in opt_params:
                p.grad = torch.zeros_like(p)
            bufs = {k: params[k].grad for k in names}

            def closure():
                loss, _, _ = evaluate(stage, body_pose, global_orient, betas, camera_translation, target, want=names, out=bufs, **kw)
                return loss
            if self.use_lbfgs:
                opt = torch.optim.LBFGS(opt_params, max_iter=self.num_iters, lr=self.step_size, line_search_fn="strong_wolfe")
                for _ in range(steps):
                    opt.step(closure)
            else:
                opt = torch.optim.Adam(opt_params, lr=self.step_size, betas=(0.9, 0.999))
                for _ in range(steps):
                    closure()
                    opt.step()
            for p in opt_params:
                p.grad = None
        # step 1: camera translation and body orientation
        run("camera", ("global_orient", "camera_translation"), 10 if self.use_lbfgs else 20, camera_estimate=init_cam_t)
        # step 2: the body; the shape stays fixed inside a sequence
        names = ("body_pose", "betas", "global_orient", "camera_translation") if seq_ind == 0 else ("body_pose", "global_orient", "camera_translation")
        run("body", names, self.num_iters, conf_3d=conf_3d, preserve_pose=preserve_pose, weights={"keep": 5.0 if self.use_lbfgs else 0.0})
        final_loss, _, g = evaluate("body", body_pose, global_orient, betas, camera_translation, target, conf_3d=conf_3d,
                                    preserve_pose=preserve_pose, weights={"keep": 0.0}, want=(), rotations=True)
        vertices, joints = self._forward(g["rotations"], betas)
        self.native_seconds = spent[0] if time_native else None
        pose = torch.cat([global_orient, body_pose], dim=-1)
        return vertices, joints, pose, betas, camera_translation, final_loss
