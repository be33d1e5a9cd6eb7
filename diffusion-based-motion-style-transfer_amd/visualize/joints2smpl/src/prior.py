"""`MaxMixturePrior`: the Gaussian-mixture pose prior of the reference's visualize/joints2smpl/src/prior.py:99-195, as buffers.  The
file (`gmm_08.pkl`) is the user's own, as the SMPL body is; nothing is bundled.

The buffers are built exactly as prior.py:130-170 builds them at dtype float32: `means`, `covs` and `precisions` =
inv(cov.astype(float32)).astype(float32); `nll_weights` = weights / ((2 pi)^(69/2) sqrt(det cov) / min sqrt(det cov)) from the FLOAT64
determinants, rounded to float32; `weights`.  Built and validated on the host, no GPU needed.  The likelihood itself is evaluated
inside the fused objective (csrc/mst_smplify.h): `packed(device)` hands it the operand image, made once per device from the symmetric
part 1/2 (P + P^T) formed in double -- the gradient autograd gives the reference, whose float32 P is not symmetric."""
import pickle

import numpy as np
import torch

from .... import _native as N

NUM_GAUSSIANS = 8
POSE_DIM = 69


class MaxMixturePrior:
    def __init__(self, means, covars, weights, epsilon=1e-16):
        what = "MaxMixturePrior"
        means, covars, weights = np.asarray(means, np.float64), np.asarray(covars, np.float64), np.asarray(weights, np.float64).reshape(-1)
        if means.shape != (NUM_GAUSSIANS, POSE_DIM):
            raise ValueError(f"{what}: means of shape {means.shape}, expected [{NUM_GAUSSIANS}, {POSE_DIM}] (only gmm_08 over the 69 body-pose values is built)")
        if covars.shape != (NUM_GAUSSIANS, POSE_DIM, POSE_DIM):
            raise ValueError(f"{what}: covars of shape {covars.shape}, expected [{NUM_GAUSSIANS}, {POSE_DIM}, {POSE_DIM}]")
        if weights.shape != (NUM_GAUSSIANS,):
            raise ValueError(f"{what}: {weights.shape[0]} weights, expected {NUM_GAUSSIANS}")
        for name, a in (("means", means), ("covars", covars), ("weights", weights)):
            if not np.isfinite(a).all():
                raise ValueError(f"{what}: {name} is not finite")
        if not (weights > 0).all():
            raise ValueError(f"{what}: every mixture weight must be positive (min {weights.min():.3e}); the likelihood takes its logarithm")
        dets = np.array([np.linalg.det(c) for c in covars])
        if not (np.isfinite(dets).all() and (dets > 0).all()):
            raise ValueError(f"{what}: a covariance has determinant {dets.min():.3e}; every covariance must be positive definite")
        self.num_gaussians, self.epsilon, self.random_var_dim = NUM_GAUSSIANS, epsilon, POSE_DIM
        covs32 = covars.astype(np.float32)
        self.means = torch.tensor(means.astype(np.float32))
        self.covs = torch.tensor(covs32)
        precisions = np.stack([np.linalg.inv(c) for c in covs32]).astype(np.float32)
        if not np.isfinite(precisions).all():
            raise ValueError(f"{what}: a float32 covariance has no finite inverse")
        self.precisions = torch.tensor(precisions)
        sqrdets = np.sqrt(dets)
        const = (2 * np.pi) ** (69 / 2.)
        self.nll_weights = torch.tensor(np.asarray(weights / (const * (sqrdets / sqrdets.min()))), dtype=torch.float32).unsqueeze(0)
        if not (self.nll_weights > 0).all():
            raise ValueError(f"{what}: a component's constant underflows float32 (determinants {dets.min():.3e} .. {dets.max():.3e})")
        self.weights = torch.tensor(weights, dtype=torch.float32).unsqueeze(0)
        self.pi_term = torch.log(torch.tensor(2 * np.pi, dtype=torch.float32))
        self.cov_dets = torch.tensor(np.array([np.log(np.linalg.det(c) + epsilon) for c in covs32]), dtype=torch.float32)
        self._packed = {}

    @classmethod
    def from_arrays(cls, *, means, covars, weights, epsilon=1e-16):
        return cls(means, covars, weights, epsilon)

    @classmethod
    def from_pkl(cls, path, epsilon=1e-16):
        """The dict form {'means', 'covars', 'weights'} of gmm_08.pkl, read with encoding='latin1' as the reference reads it.  The
        sklearn-object form is not read.  Unpickling runs code: only open files you trust."""
        with open(path, "rb") as fh:
            gmm = pickle.load(fh, encoding="latin1")
        if not isinstance(gmm, dict):
            raise ValueError(f"MaxMixturePrior.from_pkl: {path} holds a {type(gmm).__name__}, expected the dict form with 'means', 'covars', 'weights'")
        missing = [k for k in ("means", "covars", "weights") if k not in gmm]
        if missing:
            raise KeyError(f"MaxMixturePrior.from_pkl: {path} lacks {missing} (keys: {sorted(gmm)[:20]})")
        return cls(gmm["means"], gmm["covars"], gmm["weights"], epsilon)

    def to(self, device):
        return self

    def get_mean(self):
        """The mean of the mixture, [1, 69]."""
        return torch.matmul(self.weights, self.means)

    def symmetric_precisions(self):
        """1/2 (P + P^T) of the float32 precisions, formed in double, rounded to float32."""
        p = self.precisions.numpy().astype(np.float64)
        return (0.5 * (p + p.transpose(0, 2, 1))).astype(np.float32)

    def packed(self, device):
        """The kernel's operand image on `device`, made on first use there."""
        device = torch.device(device)
        if device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("MaxMixturePrior runs on the GPU only (no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._packed:
            lib = N.lib()
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
            prec, means = up(self.symmetric_precisions()), up(self.means.numpy())
            neglog = up(-np.log(self.nll_weights.numpy().reshape(-1)))
            out = torch.empty(int(lib.mst_smplify_packed_prior_bytes()) // 4, dtype=torch.float32, device=device)
            with torch.cuda.device(device):
                N.check(lib.mst_smplify_pack_prior(N.ptr(prec), N.ptr(means), N.ptr(neglog), N.ptr(out), N.stream_ptr(device)))
                torch.cuda.current_stream(device).synchronize()            # the three sources are dropped below
            self._packed[device] = out
        return self._packed[device]
