"""The statistics of data_loaders/humanml/utils/metrics.py on the GPU (csrc/mst_eval.h): distance matrix and R-precision ranks,
matching score, diversity, multimodality, activation statistics, and the Frechet distance over them.

Every function takes numpy arrays (uploaded to the current GPU, results returned as numpy) or GPU tensors (array results stay on the
device).  Scalars come back as Python / numpy numbers either way.  The random index draws of diversity and multimodality stay on the host
and are the reference's own `np.random.choice` calls in its order, so a seeded run picks the same pairs.

Stated differences from the reference:
  * a distance whose radicand -2 a.b + |a|^2 + |b|^2 rounds below zero is 0 here, NaN there.  Only a negative radicand is clamped: a
    NaN or infinite embedding row gives non-finite distances here as there, never 0;
  * `calculate_R_precision` counts, per row, the entries strictly below the diagonal one (top-k is rank < k) where the reference
    argsorts: the two differ only where a row holds an exact tie with its diagonal entry, which argsort resolves by position;
  * a row whose diagonal distance is not finite gets rank N here and so is a hit at no k.  The reference's argsort puts NaN last, so
    an all-NaN row is ranked there by position (row 0 of a batch would hit at top-1); a NaN entry elsewhere in a row is "not below"
    the diagonal in both;
  * `calculate_activation_statistics` returns the mean in float64 (summed in double on the device); the reference's `np.mean` of
    float32 rows is float32.  The covariance is float64 in both.
The 512 x 512 matrix square root of the Frechet distance runs in float64 on the host (scipy.linalg.sqrtm)."""
import numpy as np
import torch

from .. import _native as N


def _up(x, what):
    """-> (fp32 contiguous GPU tensor, was_tensor)."""
    was = torch.is_tensor(x)
    t = x.detach() if was else torch.as_tensor(np.ascontiguousarray(x))
    if not t.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError(f"{what}: the statistics run in the HIP library only (no CPU fallback): no GPU here")
        t = t.to("cuda")
    return t.to(torch.float32).contiguous(), was


def _back(t, was):
    return t if was else t.cpu().numpy()


def _dist_rank(e1, e2, what, want_rank):
    a, was = _up(e1, what)
    b, _ = _up(e2, what)
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise ValueError(f"{what}: embeddings of shapes {tuple(a.shape)} and {tuple(b.shape)}: [N1, D] and [N2, D]")
    b = b.to(a.device)
    dist = torch.empty(a.shape[0], b.shape[0], dtype=torch.float32, device=a.device)
    rank = torch.empty(a.shape[0], dtype=torch.int32, device=a.device) if want_rank else None
    with torch.cuda.device(a.device):
        N.check(N.lib().mst_eval_dist_rank(N.ptr(a), N.ptr(b), a.shape[0], b.shape[0], a.shape[1], N.ptr(dist), N.ptr(rank),
                                           N.stream_ptr(a.device)))
    return dist, rank, was


def euclidean_distance_matrix(matrix1, matrix2):
    """[N1, D], [N2, D] -> [N1, N2] float32: sqrt(-2 a.b + |a|^2 + |b|^2), the reference's expansion; a radicand below zero is 0, a
    non-finite row stays non-finite."""
    dist, _, was = _dist_rank(matrix1, matrix2, "euclidean_distance_matrix", False)
    return _back(dist, was)


def diagonal_ranks(embedding1, embedding2):
    """Per row i of the distance matrix, the number of entries strictly smaller than entry (i, i): int32 [N]."""
    _, rank, was = _dist_rank(embedding1, embedding2, "diagonal_ranks", True)
    return _back(rank, was)


def calculate_top_k(mat, top_k):
    """mat [N, N]: row i lists candidates by rising distance.  -> bool [N, top_k]: column k says whether i is among row i's first k + 1."""
    if torch.is_tensor(mat):
        own = torch.arange(mat.shape[0], device=mat.device)[:, None]
        return torch.cumsum((mat[:, :top_k] == own).to(torch.int32), 1) > 0
    mat = np.asarray(mat)
    return np.cumsum(mat[:, :top_k] == np.arange(mat.shape[0])[:, None], axis=1) > 0


def calculate_R_precision(embedding1, embedding2, top_k, sum_all=False):
    _, rank, was = _dist_rank(embedding1, embedding2, "calculate_R_precision", True)
    hits = rank[:, None] < torch.arange(1, top_k + 1, device=rank.device, dtype=torch.int32)[None]
    if sum_all:
        hits = hits.sum(0)
    return _back(hits, was)


def _pair_norms(a, b, ia, ib, what):
    ia = np.ascontiguousarray(ia, dtype=np.int32).reshape(-1)
    ib = np.ascontiguousarray(ib, dtype=np.int32).reshape(-1)
    if ia.shape != ib.shape or ia.size < 1:
        raise ValueError(f"{what}: {ia.size} and {ib.size} indices")
    if ia.min() < 0 or ia.max() >= a.shape[0] or ib.min() < 0 or ib.max() >= b.shape[0]:
        raise ValueError(f"{what}: an index outside its matrix")
    out = torch.empty(ia.size, dtype=torch.float32, device=a.device)
    da, db = torch.from_numpy(ia).to(a.device), torch.from_numpy(ib).to(a.device)
    with torch.cuda.device(a.device):
        N.check(N.lib().mst_eval_pair_norms(N.ptr(a), N.ptr(b), N.ptr(da), N.ptr(db), ia.size, a.shape[0], b.shape[0], a.shape[1], N.ptr(out),
                                            N.stream_ptr(a.device)))
    return out


def calculate_matching_score(embedding1, embedding2, sum_all=False):
    what = "calculate_matching_score"
    a, was = _up(embedding1, what)
    b, _ = _up(embedding2, what)
    assert a.dim() == 2 and a.shape == b.shape
    rows = np.arange(a.shape[0])
    dist = _pair_norms(a, b.to(a.device), rows, rows, what)
    if sum_all:
        return dist.cpu().numpy().sum(axis=0)
    return _back(dist, was)


def calculate_activation_statistics(activations):
    """[N, D] -> (mu [D], cov [D, D]) in float64: np.cov(activations, rowvar=False), the mean subtracted before the products."""
    what = "calculate_activation_statistics"
    a, was = _up(activations, what)
    if a.dim() != 2 or a.shape[0] < 2:
        raise ValueError(f"{what}: activations of shape {tuple(a.shape)}: [N >= 2, D]")
    n, d = a.shape
    mu = torch.empty(d, dtype=torch.float64, device=a.device)
    cov = torch.empty(d, d, dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        N.check(N.lib().mst_eval_cov(N.ptr(a), n, d, N.ptr(mu), N.ptr(cov), N.stream_ptr(a.device)))
    return _back(mu, was), _back(cov, was)


def calculate_diversity(activation, diversity_times):
    what = "calculate_diversity"
    a, _ = _up(activation, what)
    assert a.dim() == 2
    assert a.shape[0] > diversity_times
    num_samples = a.shape[0]
    first = np.random.choice(num_samples, diversity_times, replace=False)
    second = np.random.choice(num_samples, diversity_times, replace=False)
    return _pair_norms(a, a, first, second, what).cpu().numpy().mean()


def calculate_multimodality(activation, multimodality_times):
    what = "calculate_multimodality"
    a, _ = _up(activation, what)
    assert a.dim() == 3
    assert a.shape[1] > multimodality_times
    sents, per_sent = a.shape[:2]
    first = np.random.choice(per_sent, multimodality_times, replace=False)
    second = np.random.choice(per_sent, multimodality_times, replace=False)
    base = (np.arange(sents) * per_sent)[:, None]
    flat = a.reshape(sents * per_sent, a.shape[2])
    dist = _pair_norms(flat, flat, base + first[None], base + second[None], what)
    return dist.cpu().numpy().reshape(sents, multimodality_times).mean()


def _host64(x):
    return (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).astype(np.float64)


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """|mu1 - mu2|^2 + tr(sigma1 + sigma2 - 2 sqrt(sigma1 sigma2)) in float64 on the host; mu / sigma as numpy or GPU tensors.  As the
    reference does: a square root that is not finite is taken again with eps on both diagonals; a complex root whose diagonal has an
    imaginary part above 1e-3 is an error, a smaller one is dropped."""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(_host64(mu1)), np.atleast_1d(_host64(mu2))
    sigma1, sigma2 = np.atleast_2d(_host64(sigma1)), np.atleast_2d(_host64(sigma2))
    if mu1.shape != mu2.shape or sigma1.shape != sigma2.shape:
        raise ValueError(f"calculate_frechet_distance: means {mu1.shape} / {mu2.shape}, covariances {sigma1.shape} / {sigma2.shape}")
    root = linalg.sqrtm(sigma1 @ sigma2)
    if not np.isfinite(root).all():
        print(f"fid calculation produces singular product; adding {eps} to diagonal of cov estimates")
        ridge = eps * np.eye(sigma1.shape[0])
        root = linalg.sqrtm((sigma1 + ridge) @ (sigma2 + ridge))
    if np.iscomplexobj(root):
        if not np.allclose(np.diagonal(root).imag, 0, atol=1e-3):
            raise ValueError(f"Imaginary component {np.abs(root.imag).max()}")
        root = root.real
    gap = mu1 - mu2
    return gap @ gap + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(root)


def fid_from_embeddings(gen, real):
    """Frechet distance between two sets of embeddings [N, D]."""
    mu_g, cov_g = calculate_activation_statistics(gen)
    mu_r, cov_r = calculate_activation_statistics(real)
    return float(calculate_frechet_distance(mu_g, cov_g, mu_r, cov_r))
