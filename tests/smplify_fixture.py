"""What the SMPLify tests share: a torch restatement of the reference's fitting objective (visualize/joints2smpl/src/customloss.py,
prior.py) over tests/smpl_fixture.py's `lbs` and smplx's Rodrigues form, run under autograd in float64 (the oracle) or float32 (the
arithmetic the reference runs); a seeded synthetic mixture prior; seeded poses, targets and confidences; the inputs of the end-to-end fit.

tests/golden/make_golden_smplify.py asserts that the float64 restatement equals the reference's own functions to 1e-12, so this file
is the reference's objective and not an opinion about it.  The Rodrigues form is smplx.lbs.batch_rodrigues AS RECALLED (smplx is not
installed where this was written): |theta + 1e-8|, K = skew(theta / angle), I + sin K + (1 - cos) K K."""
import numpy as np
import torch

import smpl_fixture as sf

NG, ND = 8, 69
ANGLE_IDX = [52, 55, 9, 12]
ANGLE_SIGN = [1.0, -1.0, -1.0, -1.0]
SEL = [2, 1, 17, 16]                                       # RHip, LHip, RShoulder, LShoulder: JOINT_MAP and AMASS_JOINT_MAP alike
# body_fitting_loss_3d as smplify.py:226-233 calls it; camera_fitting_loss_3d's depth weight
SIGMA, W_JOINT, W_PRIOR, W_ANGLE, W_SHAPE, W_KEEP, W_DEPTH = 100.0, 600.0, 4.78 * 1.5, 15.2, 5.0, 5.0, 100.0
GROUPS = ("g_pose", "g_betas", "g_orient", "g_cam")
# the parity points: frames (the edges of the 16-frame tiles), target joints
PARITY = [(1, 22), (4, 24), (16, 22), (17, 24), (33, 22)]


def rodrigues(theta):
    """[..., 3] -> [..., 3, 3]: smplx's batch_rodrigues, as recalled."""
    angle = torch.norm(theta + 1e-8, dim=-1, keepdim=True)
    d = theta / angle
    cos, sin = torch.cos(angle)[..., None], torch.sin(angle)[..., None]
    rx, ry, rz = d[..., 0], d[..., 1], d[..., 2]
    z = torch.zeros_like(rx)
    K = torch.stack([z, -rz, ry, rz, z, -rx, -ry, rx, z], -1).reshape(theta.shape[:-1] + (3, 3))
    return torch.eye(3, dtype=theta.dtype) + sin * K + (1 - cos) * torch.matmul(K, K)


def smpl_forward(body, global_orient, body_pose, betas, dtype):
    """-> (vertices [N, V, 3], joints [N, 45, 3]): what smplx's SMPL returns for axis-angle input, in `dtype`."""
    n = body_pose.shape[0]
    theta = torch.cat([global_orient.reshape(n, 1, 3), body_pose.reshape(n, 23, 3)], 1).to(dtype)
    verts, joints = sf.lbs(body, rodrigues(theta), betas.to(dtype), dtype)
    return verts, joints[:, :sf.NJ + sf.NIDS]


# ------------------------------------------------------------------------------------------ the prior
def synthetic_gmm(seed=17):
    """The dict form of gmm_08.pkl: 8 Gaussians of dimension 69, covariances A A^T + c I (condition number about 25), float64."""
    g = np.random.default_rng([seed, NG, ND])
    means = g.standard_normal((NG, ND)) * 0.25
    covars = []
    for m in range(NG):
        A = g.standard_normal((ND, ND)) * (0.35 / np.sqrt(ND))
        covars.append(A @ A.T + (0.02 + 0.005 * m) * np.eye(ND))
    w = g.uniform(0.5, 1.5, NG)
    return {"means": means, "covars": np.stack(covars), "weights": w / w.sum()}


def prior_buffers(gmm):
    """prior.py:130-159 at dtype float32: float32 means and precisions, nll_weights from the float64 determinants."""
    means = gmm["means"].astype(np.float32)
    covs = gmm["covars"].astype(np.float32)
    precisions = np.stack([np.linalg.inv(c) for c in covs]).astype(np.float32)
    sqrdets = np.array([np.sqrt(np.linalg.det(c)) for c in gmm["covars"]])
    const = (2 * np.pi) ** (69 / 2.)
    nll = np.asarray(gmm["weights"] / (const * (sqrdets / sqrdets.min())))
    return {"means": means, "precisions": precisions, "nll_weights": torch.tensor(nll, dtype=torch.float32).unsqueeze(0).numpy(),
            "weights": torch.tensor(gmm["weights"], dtype=torch.float32).unsqueeze(0).numpy()}


def prior_values(buf, pose):
    """merged_log_likelihood before its min: [N, 8] in pose's dtype."""
    t = lambda a: torch.as_tensor(np.asarray(a)).to(pose.dtype)
    d = pose.unsqueeze(1) - t(buf["means"])
    y = torch.einsum("mij,bmj->bmi", t(buf["precisions"]), d)
    return 0.5 * (y * d).sum(-1) - torch.log(t(buf["nll_weights"]))


# ------------------------------------------------------------------------------------------ the two objectives, per frame
def gmof(x, sigma):
    return (sigma ** 2 * x ** 2) / (sigma ** 2 + x ** 2)


def body_per_frame(body, buf, nj, pose, orient, betas, cam, target, conf, preserve, keep=W_KEEP):
    dtype = pose.dtype
    _, joints = smpl_forward(body, orient, pose, betas, dtype)
    err = gmof((joints[:, :nj] + cam.unsqueeze(1)) - target, SIGMA)
    joint = ((W_JOINT ** 2) * ((conf ** 2) * err.sum(-1))).sum(-1)
    prior = (W_PRIOR ** 2) * prior_values(buf, pose).min(1)[0]
    angle = (W_ANGLE ** 2) * (torch.exp(pose[:, ANGLE_IDX] * torch.tensor(ANGLE_SIGN, dtype=dtype)) ** 2).sum(-1)
    shape = (W_SHAPE ** 2) * (betas ** 2).sum(-1)
    kept = (keep ** 2) * ((pose - preserve) ** 2).sum(-1)
    return joint + prior + angle + shape + kept


def camera_per_frame(body, pose, orient, betas, cam, target, cam_est):
    """camera_fitting_loss_3d: its depth term is broadcast over the four selected joints before the sum, hence the 4."""
    _, joints = smpl_forward(body, orient, pose, betas, pose.dtype)
    err = (target[:, SEL] - (joints[:, SEL] + cam.unsqueeze(1))) ** 2
    return err.sum((1, 2)) + 4 * (W_DEPTH ** 2) * ((cam - cam_est) ** 2).sum(-1)


# ------------------------------------------------------------------------------------------ seeded cases
_BODY = {}


def body83():
    if 83 not in _BODY:
        _BODY[83] = sf.synthetic_body(83)
    return _BODY[83]


GMM = synthetic_gmm()
PRIOR = prior_buffers(GMM)


def make_case(N, nj, seed=1, zero_frame=True):
    """float32 tensors of one parity point.  Frame n sits near mixture mean (3 n + seed) mod 8; frame 1 (N >= 4) is the all-zero pose."""
    g = np.random.default_rng([seed, N, nj])
    comp = (3 * np.arange(N) + seed) % NG
    pose = PRIOR["means"][comp].astype(np.float64) + 0.08 * g.standard_normal((N, ND))
    orient = 0.5 * g.standard_normal((N, 3))
    if zero_frame and N >= 4:
        pose[1], orient[1] = 0.0, 0.0
    betas = 0.5 * g.standard_normal((N, 10))
    cam = 0.3 * g.standard_normal((N, 3))
    t64 = lambda a: torch.as_tensor(a, dtype=torch.float64)
    _, j = smpl_forward(body83(), t64(orient + 0.1 * g.standard_normal((N, 3))), t64(pose + 0.15 * g.standard_normal((N, ND))), t64(betas),
                        torch.float64)
    target = j[:, :nj].numpy() + cam[:, None] + 0.02 * g.standard_normal((N, nj, 3))
    conf = g.uniform(0.5, 1.5, nj)
    conf[3] = 0.0
    c = {"pose": pose, "orient": orient, "betas": betas, "cam": cam, "target": target, "conf": conf,
         "preserve": pose + 0.05 * g.standard_normal((N, ND)), "cam_est": cam + 0.05 * g.standard_normal((N, 3))}
    c = {k: torch.as_tensor(v, dtype=torch.float32) for k, v in c.items()}
    c["N"], c["nj"] = N, nj
    return c


def evaluate(c, stage, dtype, conf=None, keep=W_KEEP, body=None, buf=None):
    """stage 'body' / 'camera' -> {'loss', 'per_frame', the four gradient groups (camera: g_orient, g_cam), 'values' [N, 8]} as float64
    numpy arrays, every step in `dtype`.  conf: None for the case's vector, or a scalar."""
    body, buf = body or body83(), buf or PRIOR
    leaf = {k: c[k].to(dtype).clone().requires_grad_(True) for k in ("pose", "orient", "betas", "cam")}
    if stage == "body":
        cf = c["conf"].to(dtype) if conf is None else torch.tensor(float(conf), dtype=dtype)
        per = body_per_frame(body, buf, c["nj"], leaf["pose"], leaf["orient"], leaf["betas"], leaf["cam"], c["target"].to(dtype), cf,
                             c["preserve"].to(dtype), keep)
    else:
        per = camera_per_frame(body, leaf["pose"], leaf["orient"], leaf["betas"], leaf["cam"], c["target"].to(dtype), c["cam_est"].to(dtype))
    loss = per.sum()
    loss.backward()
    out = {"loss": loss.detach().double().numpy(), "per_frame": per.detach().double().numpy(),
           "g_orient": leaf["orient"].grad.double().numpy(), "g_cam": leaf["cam"].grad.double().numpy()}
    if stage == "body":
        out["g_pose"], out["g_betas"] = leaf["pose"].grad.double().numpy(), leaf["betas"].grad.double().numpy()
        out["values"] = prior_values(buf, c["pose"].to(dtype)).double().numpy()
    return out


def check_case(c):
    """The conditions a parity point must meet, in float64: at least three components selected over a batch of three frames or more, and in
    every frame the best and the second-best component more than 1e-3 apart (relative), so that a flipped selection is an error."""
    v = prior_values(PRIOR, c["pose"].double()).numpy()
    order = np.sort(v, 1)
    gap = (order[:, 1] - order[:, 0]) / np.abs(order[:, 0])
    assert gap.min() > 1e-3, f"best and second-best component {gap.min():.3e} apart"
    picked = len(set(v.argmin(1).tolist()))
    if c["N"] >= 3:
        assert picked >= 3, f"only {picked} components selected over {c['N']} frames"
    return v.argmin(1)


# ------------------------------------------------------------------------------------------ the end-to-end fit
FIT_FRAMES, FIT_ITERS = 4, 30


def fit_inputs(nj, seed=5):
    """-> (init_pose [4, 72], init_betas [4, 10], j3d [4, nj, 3]) float32: targets are the 83-vertex body's joints at a known pose
    near a mixture mean, plus an offset; the start is the mixture's mean pose and zero betas."""
    g = np.random.default_rng([seed, nj])
    n = FIT_FRAMES
    pose = PRIOR["means"][[1, 1, 4, 4]].astype(np.float64) + 0.05 * g.standard_normal((n, ND))
    orient = 0.3 * g.standard_normal((n, 3))
    betas = np.tile(0.3 * g.standard_normal((1, 10)), (n, 1))
    t64 = lambda a: torch.as_tensor(a, dtype=torch.float64)
    _, j = smpl_forward(body83(), t64(orient), t64(pose), t64(betas), torch.float64)
    j3d = j[:, :nj].numpy() + np.array([0.2, 0.9, -0.1])
    mean = (PRIOR["weights"].astype(np.float64) @ PRIOR["means"].astype(np.float64)).reshape(1, ND)
    init_pose = np.concatenate([np.zeros((n, 3)), np.tile(mean, (n, 1))], 1)
    f32 = lambda a: torch.as_tensor(a, dtype=torch.float32)
    return f32(init_pose), torch.zeros(n, 10), f32(j3d)


def joint_error(joints, cam, j3d, nj):
    """mean over frames and joints of |joint + cam - target|."""
    d = (np.asarray(joints, np.float64)[:, :nj] + np.asarray(cam, np.float64).reshape(-1, 1, 3)) - np.asarray(j3d, np.float64)
    return float(np.linalg.norm(d, axis=-1).mean())
