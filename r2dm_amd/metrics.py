"""BEV metrics of the reference's ``evaluate.py`` (metrics/bev.py) as HIP kernels: the bird's-eye-view occupancy
histograms, their Jensen-Shannon distance (JSD) and the RBF-kernel maximum mean discrepancy (MMD).

Same names and signatures as the reference module; inputs are ROCm tensors and nothing falls back to the CPU.

- Histogram counts are bit-identical to ``torch.histogramdd`` on the CPU (same fp32 bin edges, same binning rules,
  the depth in the CPU's fp32 operation order).
- JSD sums the counts exactly (int64 on the GPU) and normalises them in fp64 on the host.
- MMD sums ``1 - k = -expm1(-gamma d^2)`` in fp64 with ``d^2 = sum_k (p_k - q_k)^2`` taken directly, never as
  ``|p|^2 + |q|^2 - 2 p.q``, and never forms the N x N matrix; the result is deterministic.

And the distribution metrics of feature sets (metrics/distribution.py), which evaluate.py applies to the PointNet features (FPD):

- ``feature_moments``: mean and unbiased covariance in fp64 on the GPU, two passes, deterministic.
- ``compute_frechet_distance``: those moments, then the matrix square root on the host in fp64 (scipy), as the reference.
- ``compute_squared_mmd``: the polynomial-kernel estimator over random subsets drawn on the host as the reference draws them;
  per subset the GPU gathers the rows and sums the three kernel matrices in fp64 without writing them.

And, beyond the reference, the k-NN manifold metrics on the same features (``evaluate.py --prdc_k``):

- ``feature_knn``: per row the k-th smallest / smallest squared distance to another set and the number of that set's balls it falls in,
  fp64 with the Gram term on the fp64 matrix pipe, no N x M matrix, deterministic.
- ``knn_radii``, ``manifold_metrics``: improved precision / recall and density / coverage from four such passes.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib

# evaluate.py:20-22 (from LiDARGen): the image mask applied to generated samples before the histogram
MIN_DEPTH = 0.5
MAX_DEPTH = 63.0

_LAYOUT_SAMPLES, _LAYOUT_CLOUDS = 0, 1


def bin_edges(field_size: float = 160.0, bins: int = 100) -> torch.Tensor:
    """The fp32 bin edges torch.histogramdd uses for ``range=[-field_size/2, field_size/2]`` (a linspace), on the CPU."""
    bound = field_size / 2
    return torch.linspace(-bound, bound, bins + 1, dtype=torch.float32)


def bev_histograms(samples_or_clouds: torch.Tensor, field_size: float = 160.0, bins: int = 100, min_depth: float = 3.0,
                   max_depth: float = 70.0, image_min_depth: float = MIN_DEPTH, image_max_depth: float = MAX_DEPTH,
                   return_sum: bool = False):
    """Batched ``point_cloud_to_histogram`` as evaluate.py applies it.

    ``samples_or_clouds`` is either a batch of samples ``(B,5,H,W)`` [depth, x, y, z, reflectance] (what
    ``LiDARUtility.postprocess`` and sample_and_save.py write), whose xyz is first masked by
    ``image_min_depth < depth < image_max_depth`` (evaluate.py:22-41,150-151), or a batch of point clouds ``(B,N,3)``.
    Returns int32 counts ``(B,bins,bins)`` indexed [x bin, y bin]; with ``return_sum`` also their exact int64 sum over
    the batch ``(bins,bins)``."""
    x = samples_or_clouds
    _lib.require_gpu(x, "samples_or_clouds")
    if x.ndim == 4 and x.shape[1] == 5:
        layout, B, n = _LAYOUT_SAMPLES, x.shape[0], x.shape[2] * x.shape[3]
    elif x.ndim == 3 and x.shape[2] == 3:
        layout, B, n = _LAYOUT_CLOUDS, x.shape[0], x.shape[1]
    else:
        raise ValueError(f"expected (B,5,H,W) samples or (B,N,3) point clouds, got {tuple(x.shape)}")
    if bins % 2:
        raise ValueError("bins must be even (metrics/bev.py)")
    x = _lib.f32c(x)
    edges = bin_edges(field_size, bins).to(x.device)
    hist = torch.empty(B, bins, bins, dtype=torch.int32, device=x.device)
    total = torch.empty(bins, bins, dtype=torch.int64, device=x.device) if return_sum else None
    if B and n:
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().r2dm_bev_histogram(_lib.ptr(x), layout, _lib.ptr(edges), _lib.ptr(hist), _lib.ptr(total), B, n,
                                                     bins, float(min_depth), float(max_depth), float(image_min_depth),
                                                     float(image_max_depth), _lib.stream_ptr(x.device)))
    else:
        hist.zero_()
        if total is not None:
            total.zero_()
    return (hist, total) if return_sum else hist


def point_cloud_to_histogram(point_cloud: torch.Tensor, field_size: float = 160.0, bins: int = 100, min_depth: float = 3.0,
                             max_depth: float = 70.0) -> torch.Tensor:
    """metrics/bev.py: the (bins,bins) fp32 histogram of one ``(N,3)`` point cloud (on the cloud's device)."""
    assert point_cloud.ndim == 2, "must be (N, 3)"
    return bev_histograms(point_cloud[None], field_size, bins, min_depth, max_depth)[0].float()


def _as_counts(hist: torch.Tensor, what: str) -> torch.Tensor:
    _lib.require_gpu(hist, what)
    h = hist.detach().flatten(1)
    if h.dtype != torch.int32:
        h = h.to(torch.float32)
    return h.contiguous()


def histogram_sum(hist: torch.Tensor) -> torch.Tensor:
    """Exact int64 sum over the batch of ``(N, ...)`` histograms of counts (int32, or fp32 holding integers)."""
    h = _as_counts(hist, "hist")
    if h.dtype == torch.float32 and bool(((h < 0) | (h != h.trunc())).any()):
        raise ValueError("histogram_sum takes counts: non-negative integers")
    out = torch.empty(h.shape[1], dtype=torch.int64, device=h.device)
    with torch.cuda.device(h.device):
        _lib.check(_lib.lib().r2dm_bev_hist_sum(_lib.ptr(h), int(h.dtype == torch.int32), _lib.ptr(out), h.shape[0], h.shape[1],
                                                _lib.stream_ptr(h.device)))
    return out


@torch.no_grad()
def compute_jsd_2d(hist1: torch.Tensor, hist2: torch.Tensor) -> float:
    """BEV-based Jensen-Shannon distance between the summed histograms of two sets (metrics/bev.py)."""
    from scipy.spatial.distance import jensenshannon

    s1 = histogram_sum(hist1).cpu().numpy().astype(np.float64)
    s2 = histogram_sum(hist2).cpu().numpy().astype(np.float64)
    return float(jensenshannon(s1 / s1.sum(), s2 / s2.sum()))


@torch.no_grad()
def mmd_terms(hist1: torch.Tensor, hist2: torch.Tensor, sigma: float = 0.5):
    """(mean 1-k(p,q), mean 1-k(p,p), mean 1-k(q,q)) over all pairs of the row-normalised histograms, in fp64."""
    p, q = _as_counts(hist1, "hist1").float(), _as_counts(hist2, "hist2").float()
    if p.device != q.device:
        raise ValueError(f"hist1 on {p.device}, hist2 on {q.device}")
    if p.shape[1] != q.shape[1]:
        raise ValueError(f"histograms of {p.shape[1]} and {q.shape[1]} bins")
    L = _lib.lib()
    scratch = torch.empty(L.r2dm_bev_mmd_scratch_bytes(p.shape[0], q.shape[0]) + 256, dtype=torch.uint8, device=p.device)
    base = (-scratch.data_ptr()) % 256  # 256-byte aligned start
    out = torch.empty(3, dtype=torch.float64, device=p.device)
    with torch.cuda.device(p.device):
        _lib.check(L.r2dm_bev_mmd(_lib.ptr(p), _lib.ptr(q), p.shape[0], q.shape[0], p.shape[1], float(sigma),
                                  scratch.data_ptr() + base, scratch.numel() - base, _lib.ptr(out), _lib.stream_ptr(p.device)))
    pq, pp, qq = out.tolist()
    return pq, pp, qq


@torch.no_grad()
def compute_mmd_2d(hist1: torch.Tensor, hist2: torch.Tensor) -> float:
    """BEV-based maximum mean discrepancy (metrics/bev.py): mean k_pp + mean k_qq - 2 mean k_pq, biased, sigma 0.5."""
    pq, pp, qq = mmd_terms(hist1, hist2)
    return 2.0 * pq - pp - qq


# ---- distribution metrics of feature sets (metrics/distribution.py) ----------------------------------------------------------
def _as_feats(feats, what: str) -> torch.Tensor:
    """(N,D) fp32 features on the GPU; a numpy array (the reference's cache pickle) is uploaded."""
    if isinstance(feats, np.ndarray):
        feats = torch.from_numpy(np.ascontiguousarray(feats)).cuda()
    _lib.require_gpu(feats, what)
    if feats.ndim != 2:
        raise ValueError(f"{what}: expected (N,D) features, got {tuple(feats.shape)}")
    return _lib.f32c(feats)


@torch.no_grad()
def feature_moments(feats):
    """Mean ``(D,)`` and unbiased covariance ``(D,D)`` (``np.cov(rowvar=False)``) of ``(N,D)`` features, fp64, on the GPU."""
    f = _as_feats(feats, "feats")
    n, d = f.shape
    if n < 2 or d < 1:
        raise ValueError(f"feature_moments needs at least 2 rows and 1 column, got {tuple(f.shape)}")
    mean = torch.empty(d, dtype=torch.float64, device=f.device)
    cov = torch.empty(d, d, dtype=torch.float64, device=f.device)
    with torch.cuda.device(f.device):
        _lib.check(_lib.lib().r2dm_feature_moments(_lib.ptr(f), n, d, _lib.ptr(mean), _lib.ptr(cov), _lib.stream_ptr(f.device)))
    return mean, cov


def compute_frechet_distance(feats1, feats2) -> float:
    """Frechet distance between the Gaussians fitted to two feature sets (metrics/distribution.py):
    ``|mu1 - mu2|^2 + tr(S1 + S2 - 2 sqrtm(S1 S2))``, the moments on the GPU, the rest on the host in fp64."""
    import scipy.linalg

    mu1, s1 = (t.cpu().numpy() for t in feature_moments(feats1))
    mu2, s2 = (t.cpu().numpy() for t in feature_moments(feats2))
    if mu1.shape != mu2.shape:
        raise ValueError(f"features of {mu1.shape[0]} and {mu2.shape[0]} dimensions")
    m = np.square(mu1 - mu2).sum()
    s, _ = scipy.linalg.sqrtm(np.dot(s1, s2), disp=False)
    return float(np.real(m + np.trace(s1 + s2 - s * 2)))


def draw_mmd_subsets(n1: int, n2: int, num_subsets: int = 100, max_subset_size: int = 1000, rng=None):
    """The subsets of compute_squared_mmd in the reference's order of draws: per subset first ``choice(n2, m)`` (rows of
    feats2), then ``choice(n1, m)`` (rows of feats1), without replacement, from ``rng`` (anything with numpy's ``choice``;
    None = numpy's global state).  Returns int64 arrays ``(idx1, idx2)`` of shape ``(num_subsets, m)``."""
    choice = np.random.choice if rng is None else rng.choice
    m = min(min(n1, n2), max_subset_size)
    idx1, idx2 = np.empty((num_subsets, m), np.int64), np.empty((num_subsets, m), np.int64)
    for s in range(num_subsets):
        idx2[s] = choice(n2, m, replace=False)
        idx1[s] = choice(n1, m, replace=False)
    return idx1, idx2


@torch.no_grad()
def squared_mmd_from_indices(feats1, feats2, idx1, idx2) -> float:
    """compute_squared_mmd over explicit subsets: ``idx1`` / ``idx2`` (num_subsets, m) rows of feats1 / feats2."""
    f1, f2 = _as_feats(feats1, "feats1"), _as_feats(feats2, "feats2")
    if f1.device != f2.device:
        raise ValueError(f"feats1 on {f1.device}, feats2 on {f2.device}")
    if f1.shape[1] != f2.shape[1]:
        raise ValueError(f"features of {f1.shape[1]} and {f2.shape[1]} dimensions")
    idx1, idx2 = np.ascontiguousarray(idx1, dtype=np.int64), np.ascontiguousarray(idx2, dtype=np.int64)
    if idx1.ndim != 2 or idx1.shape != idx2.shape or idx1.shape[0] < 1 or idx1.shape[1] < 2:
        raise ValueError(f"subset indices of shapes {idx1.shape} and {idx2.shape}: expected two (num_subsets, m >= 2) arrays")
    for idx, f, what in ((idx1, f1, "idx1"), (idx2, f2, "idx2")):
        if idx.min() < 0 or idx.max() >= f.shape[0]:
            raise ValueError(f"{what} holds a row outside [0, {f.shape[0]})")
    S, m = idx1.shape
    d = f1.shape[1]
    L = _lib.lib()
    sums = torch.empty(S, 3, dtype=torch.float64, device=f1.device)
    with torch.cuda.device(f1.device):
        for k in range(0, S, 4096):  # (a launch takes up to 65535 subsets)
            nb = min(4096, S - k)
            ix = torch.from_numpy(idx2[k:k + nb]).to(f1.device)  # x: rows of feats2, y: rows of feats1 (the reference's naming)
            iy = torch.from_numpy(idx1[k:k + nb]).to(f1.device)
            scratch = torch.empty(L.r2dm_poly_mmd_scratch_bytes(nb, m) + 256, dtype=torch.uint8, device=f1.device)
            base = (-scratch.data_ptr()) % 256
            _lib.check(L.r2dm_poly_mmd(_lib.ptr(f2), _lib.ptr(f1), _lib.ptr(ix), _lib.ptr(iy), nb, m, d, scratch.data_ptr() + base,
                                       scratch.numel() - base, sums[k:k + nb].data_ptr(), _lib.stream_ptr(f1.device)))
    xy, xx, yy = sums.cpu().numpy().T
    t = ((xx + yy) / (m - 1) - xy * 2 / m).sum()
    return float(t / S / m)


def compute_squared_mmd(feats1, feats2, num_subsets: int = 100, max_subset_size: int = 1000, rng=None) -> float:
    """Squared MMD with the polynomial kernel ``(x.y / D + 1)^3`` over random subsets (metrics/distribution.py)."""
    n1, n2 = len(feats1), len(feats2)
    idx1, idx2 = draw_mmd_subsets(n1, n2, num_subsets, max_subset_size, rng)
    return squared_mmd_from_indices(feats1, feats2, idx1, idx2)


# ---- k-NN manifold metrics of feature sets: improved precision / recall, density / coverage ----------------------------------
_KNN_OUTPUTS = ("kth2", "min2", "argmin", "count")


@torch.no_grad()
def feature_knn(x, y=None, k: int = 0, y_radius2=None, want=_KNN_OUTPUTS, return_launch: bool = False):
    """Per row ``i`` of ``x`` (m,D) over the rows ``j`` of ``y`` (n,D), with ``D2(i,j) = max(0, |x_i|^2 + |y_j|^2 - 2 x_i.y_j)`` in fp64
    (the Gram term on the fp64 matrix pipe, no m x n matrix):

    - ``kth2`` (m,) fp64: the k-th smallest ``D2`` (needs ``k >= 1``);
    - ``min2`` (m,) fp64 and ``argmin`` (m,) int32: the smallest ``D2`` and its row of ``y``, the lowest on an equal value;
    - ``count`` (m,) int32: the number of ``j`` with ``D2 <= y_radius2[j]`` (needs ``y_radius2`` (n,) fp64).

    ``y=None`` means the same set: ``j == i`` is left out by index, so ``k`` is the k-th nearest *other* sample and a duplicate row is a
    neighbour at distance 0.  Returns a dict of the outputs named in ``want`` that can be computed; with ``return_launch`` also
    ``"launch"``: (row tiles, column splits).  Raises ``R2DMError`` on a refusal or when a row of ``x`` or ``y`` holds a non-finite value."""
    same = y is None
    fx = _as_feats(x, "x")
    fy = fx if same else _as_feats(y, "y")
    if fx.device != fy.device:
        raise ValueError(f"x on {fx.device}, y on {fy.device}")
    if fx.shape[1] != fy.shape[1]:
        raise ValueError(f"features of {fx.shape[1]} and {fy.shape[1]} dimensions")
    unknown = set(want) - set(_KNN_OUTPUTS)
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}: expected some of {_KNN_OUTPUTS}")
    (m, d), n, dev = fx.shape, fy.shape[0], fx.device
    r2 = None
    if y_radius2 is not None:
        if isinstance(y_radius2, np.ndarray):
            y_radius2 = torch.from_numpy(np.ascontiguousarray(y_radius2))
        r2 = y_radius2.detach().to(device=dev, dtype=torch.float64).contiguous()
        if r2.shape != (n,):
            raise ValueError(f"y_radius2 of shape {tuple(r2.shape)}: expected ({n},)")
    out = {}
    if "kth2" in want and k >= 1:
        out["kth2"] = torch.empty(m, dtype=torch.float64, device=dev)
    if "min2" in want:
        out["min2"] = torch.empty(m, dtype=torch.float64, device=dev)
    if "argmin" in want:
        out["argmin"] = torch.empty(m, dtype=torch.int32, device=dev)
    if "count" in want and r2 is not None:
        out["count"] = torch.empty(m, dtype=torch.int32, device=dev)
    L = _lib.lib()
    nbytes = L.r2dm_feature_knn_scratch_bytes(m, n, d, int(k))
    scratch = torch.empty(max(nbytes, 8) // 8 + 1, dtype=torch.float64, device=dev)
    status = torch.empty(1, dtype=torch.int64, device=dev)
    chosen = (ctypes.c_int32 * 2)()
    with torch.cuda.device(dev):
        _lib.check(L.r2dm_feature_knn(_lib.ptr(fx), m, _lib.ptr(fy), n, d, int(same), int(k), _lib.ptr(r2), _lib.ptr(out.get("kth2")),
                                      _lib.ptr(out.get("min2")), _lib.ptr(out.get("argmin")), _lib.ptr(out.get("count")), scratch.data_ptr(),
                                      scratch.numel() * 8, _lib.ptr(status), chosen, _lib.stream_ptr(dev)))
    bad = int(status.item())
    if bad:
        raise _lib.R2DMError(f"feature_knn: {bad} row(s) of the features hold a non-finite value")
    if return_launch:
        out["launch"] = (int(chosen[0]), int(chosen[1]))
    return out


def knn_radii(feats, k: int) -> torch.Tensor:
    """(N,) fp64: per row the squared distance to its k-th nearest *other* row (the ``nearest_k`` of the ``prdc`` package)."""
    if k < 1:
        raise ValueError(f"knn_radii needs k >= 1, got {k}")
    return feature_knn(feats, None, k, want=("kth2",))["kth2"]


def manifold_metrics(real, fake, k: int = 5, per_sample: bool = False) -> dict:
    """Improved precision and recall (Kynkaanniemi et al. 2019) and density and coverage (Naeem et al. 2020) of generated features ``fake``
    (M,D) against ``real`` (N,D).  With ``r_i^2`` / ``s_j^2`` the squared distance of real i / fake j to its k-th nearest *other* sample of its
    own set, and every comparison ``<=`` on squared distances (``prdc`` compares ``<``; the two differ on exact ties only):

    - precision = mean_j [exists i: D2(R_i, F_j) <= r_i^2],   recall = mean_i [exists j: D2(R_i, F_j) <= s_j^2],
    - density = 1 / (k M) sum_j #{i: D2(R_i, F_j) <= r_i^2},  coverage = mean_i [min_j D2(R_i, F_j) <= r_i^2].

    Four passes of ``feature_knn``.  ``per_sample`` adds ``fake_in_real`` (M,) bool, ``fake_count`` (M,) int32, ``real_in_fake`` (N,) bool,
    ``real_covered`` (N,) bool, ``real_radius2`` (N,) and ``fake_radius2`` (M,) fp64."""
    r, f = _as_feats(real, "real"), _as_feats(fake, "fake")
    r2, s2 = knn_radii(r, k), knn_radii(f, k)
    fake_count = feature_knn(f, r, 0, r2, want=("count",))["count"]
    rf = feature_knn(r, f, 0, s2, want=("count", "min2"))
    fake_in_real, real_in_fake, real_covered = fake_count > 0, rf["count"] > 0, rf["min2"] <= r2
    hits = torch.stack([fake_in_real.sum(), real_in_fake.sum(), fake_count.sum(dtype=torch.int64), real_covered.sum()]).tolist()  # exact counts, one read
    (n, _), m = r.shape, f.shape[0]
    out = {"precision": hits[0] / m, "recall": hits[1] / n, "density": hits[2] / (k * m), "coverage": hits[3] / n}
    if per_sample:
        out.update(fake_in_real=fake_in_real, fake_count=fake_count, real_in_fake=real_in_fake, real_covered=real_covered, real_radius2=r2,
                   fake_radius2=s2)
    return out
