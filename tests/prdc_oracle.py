"""numpy fp64 oracle of the k-NN manifold metrics (improved precision / recall, density / coverage) and the cases the tests share.

Distances are taken in DIFFERENCE form, ``sum_d (a_d - b_d)^2`` over the values widened to fp64 -- independent of the Gram form
``|a|^2 + |b|^2 - 2 a.b`` the library computes.  Radii: the k-th smallest distance to another sample of the same set, self left out by
index.  Every comparison is ``<=`` on squared distances.

Tolerance for values, derived and not measured: ``tol_i = 2^-36 (|x_i|^2 + max_j |y_j|^2)``.  Unit roundoff is 2^-53 and a sum has at
most 2^14 terms, so the worst case is 2^-39 of ``(|x|^2 + |y|^2) / 2``; 2^-36 leaves 8 x headroom.  A decision ``D2 <= radius`` is
non-firm when ``|D2 - radius| <= 2 tol``, with ``tol`` the larger of the tolerance of the distance and that of the radius (each is a
distance of its own pass); ``nonfirm`` counts those, and the minima whose runner-up is that close (where argmin could differ).  The
non-lattice cases below have none (tests/test_prdc_cpu.py), so the GPU test compares every decision.
"""
import numpy as np

TOL_SCALE = 2.0 ** -36


def widen(x):
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    return x.astype(np.float64)


def d2(x, y):
    """(m,n) fp64 squared distances in difference form, row-chunked."""
    x, y = widen(x), widen(y)
    out = np.empty((len(x), len(y)))
    step = max(1, (1 << 24) // max(1, y.size))
    for a in range(0, len(x), step):
        diff = x[a:a + step, None, :] - y[None, :, :]
        out[a:a + step] = np.square(diff).sum(-1)
    return out


def norms2(x):
    return np.square(widen(x)).sum(-1)


def tol(x, y):
    """(m,) the value tolerance of row i of x against the set y."""
    return TOL_SCALE * (norms2(x) + norms2(y).max())


def feature_knn(x, y=None, k=0, y_radius2=None):
    """The library's primitive: dict of kth2 (k >= 1), min2, argmin (lowest column on a tie), count (with y_radius2)."""
    same = y is None
    d = d2(x, x if same else y)
    if same:
        np.fill_diagonal(d, np.inf)  # by index: a duplicate row stays, at distance 0
    out = {"min2": d.min(1), "argmin": d.argmin(1).astype(np.int32)}
    if k >= 1:
        out["kth2"] = np.sort(d, axis=1)[:, k - 1]
    if y_radius2 is not None:
        out["count"] = (d <= np.asarray(y_radius2)[None, :]).sum(1).astype(np.int32)
    return out


def knn_radii(x, k):
    return feature_knn(x, None, k)["kth2"]


def manifold_metrics(real, fake, k):
    """The four metrics and the per-sample tensors behind them."""
    r2, s2 = knn_radii(real, k), knn_radii(fake, k)
    d = d2(real, fake)  # (N, M)
    inside_real = d <= r2[:, None]  # fake j in the ball of real i
    inside_fake = d <= s2[None, :]  # real i in the ball of fake j
    fake_count = inside_real.sum(0).astype(np.int32)
    out = dict(fake_in_real=fake_count > 0, fake_count=fake_count, real_in_fake=inside_fake.any(1), real_covered=d.min(1) <= r2,
               real_radius2=r2, fake_radius2=s2)
    out.update(precision=float(out["fake_in_real"].mean()), recall=float(out["real_in_fake"].mean()),
               density=float(fake_count.sum() / (k * len(fake))), coverage=float(out["real_covered"].mean()))
    return out


def _close_minima(d, t):
    """rows whose two smallest values are within 2 t of each other"""
    if d.shape[1] < 2:
        return 0
    s = np.sort(d, axis=1)
    return int((s[:, 1] - s[:, 0] <= 2 * t).sum())


def nonfirm(real, fake, k):
    """The number of non-firm decisions of the four passes of ``manifold_metrics(real, fake, k)``."""
    r2, s2 = knn_radii(real, k), knn_radii(fake, k)
    t_rr, t_ff, t_rf, t_fr = tol(real, real), tol(fake, fake), tol(real, fake), tol(fake, real)
    d = d2(real, fake)
    n = 0
    # fake j against real i with r_i^2 (pass F x R) and real i against fake j with s_j^2 (pass R x F)
    n += int((np.abs(d - r2[:, None]) <= 2 * np.maximum(t_fr[None, :], t_rr[:, None])).sum())
    n += int((np.abs(d - s2[None, :]) <= 2 * np.maximum(t_rf[:, None], t_ff[None, :])).sum())
    # (coverage compares min_j D2(R_i, F_j) with r_i^2: one of the comparisons of the first group)  the column of the minimum, in both cross passes:
    n += _close_minima(d, t_rf) + _close_minima(d.T, t_fr)
    return n


# ---- the shared cases ---------------------------------------------------------------------------------------------------------------
# name: (N, M, D, k, draw, seed, shift of the generated set, its scale)
CASES = {
    "gauss": (130, 97, 20, 3, "gauss", 101, 0.35, 0.9),
    "split": (1500, 1100, 8, 5, "gauss", 102, 0.35, 0.9),
    "k16": (50, 47, 3, 16, "gauss", 103, 1.5, 0.7),
    "d1": (65, 64, 1, 2, "gauss", 104, 1.0, 0.8),
    "feat1808": (70, 65, 1808, 5, "latent", 105, 0.35, 0.9),
    "feat4096": (40, 33, 4096, 1, "latent", 106, 0.35, 0.9),
}
LATENT = 4


def make_case(name):
    """(real (N,D), fake (M,D), k), fp32, seeded PCG64; the generated set comes from a shifted, slightly narrower distribution."""
    N, M, D, k, draw, seed, shift, scale = CASES[name]
    g = np.random.Generator(np.random.PCG64(seed))
    if draw == "gauss":
        real = g.standard_normal((N, D))
        fake = shift + scale * g.standard_normal((M, D))
    else:  # a 4-dimensional Gaussian latent through a fixed random linear map, 1 % isotropic noise, then max(., 0)
        A = g.standard_normal((LATENT, D))
        real = np.maximum(g.standard_normal((N, LATENT)) @ A + 0.01 * g.standard_normal((N, D)), 0.0)
        fake = np.maximum((shift + scale * g.standard_normal((M, LATENT))) @ A + 0.01 * g.standard_normal((M, D)), 0.0)
    return real.astype(np.float32), fake.astype(np.float32), k


LATTICE_K = 3


def make_lattice(duplicates=False):
    """Rows of integers in [-3, 3], D = 6: every product and sum is exact in fp64 in either form, and ties are real.  Returns
    (real (90,6), fake (77,6), k = 3); with ``duplicates`` one set of 90 rows, a few of which are copies of others, for ``same = 1``."""
    g = np.random.Generator(np.random.PCG64(107))
    real = g.integers(-3, 4, size=(90, 6)).astype(np.float32)
    fake = g.integers(-3, 4, size=(77, 6)).astype(np.float32)
    if duplicates:
        x = real.copy()
        x[[5, 17, 40, 41, 42, 89]] = x[[4, 3, 39, 39, 39, 0]]
        return x, LATTICE_K
    return real, fake, LATTICE_K
