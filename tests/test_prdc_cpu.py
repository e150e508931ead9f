"""CPU tests of the k-NN manifold metrics: the numpy oracle against the definitions, the shared cases' firmness, the library's scratch
bound and its host-side refusals (none of which needs a device)."""
import ctypes

import numpy as np
import pytest

import prdc_oracle as O

METRICS = ("precision", "recall", "density", "coverage")
INDICATORS = ("fake_in_real", "real_in_fake", "real_covered")


def _literal(real, fake, k):
    """The four definitions as loops over scalars."""
    R, F = real.astype(np.float64), fake.astype(np.float64)
    N, M, D = len(R), len(F), R.shape[1]

    def dist(a, b):
        s = 0.0
        for c in range(D):
            s += (a[c] - b[c]) * (a[c] - b[c])
        return s

    def radii(X):
        return [sorted(dist(X[i], X[j]) for j in range(len(X)) if j != i)[k - 1] for i in range(len(X))]

    r2, s2 = radii(R), radii(F)
    precision = sum(any(dist(R[i], F[j]) <= r2[i] for i in range(N)) for j in range(M)) / M
    recall = sum(any(dist(R[i], F[j]) <= s2[j] for j in range(M)) for i in range(N)) / N
    density = sum(sum(dist(R[i], F[j]) <= r2[i] for i in range(N)) for j in range(M)) / (k * M)
    coverage = sum(min(dist(R[i], F[j]) for j in range(M)) <= r2[i] for i in range(N)) / N
    return dict(precision=precision, recall=recall, density=density, coverage=coverage)


def test_oracle_matches_the_literal_definitions():
    g = np.random.Generator(np.random.PCG64(5))
    real = g.integers(-8, 9, size=(7, 3)).astype(np.float32) / 4  # (exact in either order of summation)
    fake = g.integers(-8, 9, size=(6, 3)).astype(np.float32) / 4 + 1.5
    for k in (1, 2, 3):
        got, want = O.manifold_metrics(real, fake, k), _literal(real, fake, k)
        assert {q: got[q] for q in METRICS} == want
    m = O.manifold_metrics(real, fake, 2)
    assert 0 < m["precision"] < 1 and 0 < m["recall"] < 1 and 0 < m["coverage"] < 1, m


def test_hand_worked_example():
    """real 0, 1, 3 and generated 0.5, 0.75, 10 on a line, k = 1.  r^2 = 1, 1, 4; s^2 = 1/16, 1/16, 9.25^2.
    D2 rows (real) x columns (generated): [1/4, 9/16, 100], [1/4, 1/16, 81], [6.25, 5.0625, 49].
    precision: 0.5 and 0.75 lie in the balls of 0 and 1, 10 in none: 2/3; density: (2 + 2 + 0) / (1 * 3) = 4/3.
    recall: 0 is in no generated ball; 1 is in the ball of 0.75 on a tie (1/16 <= 1/16) and in that of 10; 3 in the ball of 10: 2/3.
    coverage: nearest generated at 1/4 <= 1, 1/16 <= 1, 5.0625 > 4: 2/3."""
    real, fake = np.array([[0.0], [1.0], [3.0]], np.float32), np.array([[0.5], [0.75], [10.0]], np.float32)
    m = O.manifold_metrics(real, fake, 1)
    assert np.array_equal(m["real_radius2"], [1.0, 1.0, 4.0]) and np.array_equal(m["fake_radius2"], [0.0625, 0.0625, 85.5625])
    assert (m["precision"], m["recall"], m["density"], m["coverage"]) == (2 / 3, 2 / 3, 4 / 3, 2 / 3)
    assert m["fake_count"].tolist() == [2, 2, 0] and m["real_in_fake"].tolist() == [False, True, True]
    assert m["real_covered"].tolist() == [True, True, False]
    p = O.feature_knn(real, fake, 2, m["fake_radius2"])
    assert p["argmin"].tolist() == [0, 1, 1] and p["kth2"].tolist() == [0.5625, 0.25, 6.25] and p["count"].tolist() == [0, 2, 1]


@pytest.mark.parametrize("name", list(O.CASES))
def test_cases_are_firm_and_not_degenerate(name):
    real, fake, k = O.make_case(name)
    N, M, D, kk = O.CASES[name][:4]
    assert real.shape == (N, D) and fake.shape == (M, D) and k == kk and real.dtype == fake.dtype == np.float32
    assert O.nonfirm(real, fake, k) == 0
    m = O.manifold_metrics(real, fake, k)
    for q in INDICATORS:
        assert m[q].any() and not m[q].all(), q
    assert all(0 < m[q] for q in METRICS) and all(m[q] < 1 for q in ("precision", "recall", "coverage"))


def test_lattice_cases_hold_exact_ties():
    real, fake, k = O.make_lattice()
    d, r2, s2 = O.d2(real, fake), O.knn_radii(real, k), O.knn_radii(fake, k)
    assert (d == np.round(d)).all() and (d == r2[:, None]).sum() > 0 and (d == s2[None, :]).sum() > 0  # ties at a radius
    assert ((d == d.min(1, keepdims=True)).sum(1) > 1).any()  # ... and at a minimum: the lowest-column rule decides
    x, k = O.make_lattice(duplicates=True)
    dd = O.d2(x, x)
    np.fill_diagonal(dd, np.inf)
    assert (dd == 0).sum() >= 8 and (O.knn_radii(x, k) == 0).any()  # duplicates are neighbours at distance 0 (rows 39 ... 42 are one point: radius 0 at k = 3)
    assert (dd == O.knn_radii(x, k)[:, None]).sum() > len(x)


def test_scratch_bound():
    from r2dm_amd import _lib

    L = _lib.lib()
    b = L.r2dm_feature_knn_scratch_bytes(10000, 10000, 4096, 5)
    assert 0 < b <= 64 << 20
    assert b < 10000 * 10000 * 8 // 50  # nothing like an m x n buffer
    assert L.r2dm_feature_knn_scratch_bytes(1 << 20, 1 << 20, 16384, 16) > 0
    for bad in ((0, 5, 4, 1), (5, 0, 4, 1), (5, 5, 0, 1), (5, 5, 16385, 1), (5, 5, 4, 17), (5, 5, 4, -1), ((1 << 20) + 1, 5, 4, 1)):
        assert L.r2dm_feature_knn_scratch_bytes(*bad) == 0, bad


def test_host_side_refusals():
    """Every refusal happens before anything is launched or written, so no device (and no real memory) is needed: the pointers are
    aligned addresses that are never dereferenced."""
    from r2dm_amd import _lib

    L = _lib.lib()
    X, Y, R, O1, O2, S, ST = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000
    big = 1 << 30

    def call(x=X, m=8, y=Y, n=9, dim=4, same=0, k=2, r2=R, kth2=O1, min2=O2, argmin=None, count=None, scratch=S, nbytes=big, status=ST):
        chosen = (ctypes.c_int32 * 2)(-7, -7)
        rc = L.r2dm_feature_knn(x, m, y, n, dim, same, k, r2, kth2, min2, argmin, count, scratch, nbytes, status, chosen, None)
        assert list(chosen) == [-7, -7]  # (nothing written)
        return rc, L.r2dm_last_error().decode()

    for kw, text in ((dict(x=None), "null argument"), (dict(y=None), "null argument"), (dict(scratch=None), "null argument"),
                     (dict(status=None), "null argument"), (dict(dim=0), "dim must be in [1, 16384]"), (dict(dim=16385), "dim must be"),
                     (dict(k=17), "k must be in [0, 16]"), (dict(k=-1), "k must be"), (dict(m=0), "m and n must be"),
                     (dict(n=(1 << 20) + 1), "m and n must be"), (dict(same=1, y=X, n=9), "same = 1 needs y == x and m == n"),
                     (dict(same=1, n=8), "same = 1 needs y == x and m == n"), (dict(count=O1, kth2=None, r2=None), "count needs y_radius2"),
                     (dict(k=0), "kth2 needs k >= 1"), (dict(n=1), "fewer than k"), (dict(same=1, y=X, m=2, n=2), "fewer than k"),
                     (dict(x=X + 4), "16-byte aligned"), (dict(kth2=O1 + 4), "8-byte aligned"), (dict(argmin=O1 + 2), "4-byte aligned"),
                     (dict(nbytes=64), "scratch too small")):
        rc, err = call(**kw)
        assert rc == 1 and text in err, (kw, rc, err)
    rc, err = call(x=X + 4, y=Y + 4, dim=3, nbytes=64)  # (dim % 4 != 0: 4-byte alignment passes; refused further on)
    assert rc == 1 and "scratch too small" in err
