"""Plain numpy / float64 oracle of the earth mover's distance (r2dm_amd/geometry.py: emd_pairs, pairwise_emd), run on the same float32 inputs.

Clouds are (n,>=3) arrays whose first three columns are x, y, z in metres.  ``EMD(A, B) = (1/n) min_sigma sum_i |a_i - b_sigma(i)|``."""
import itertools
import math

import numpy as np


def cost_matrix(a, b):
    """(|a|,|b|) float64 Euclidean distances, in the difference form"""
    a, b = np.asarray(a, np.float64)[:, :3], np.asarray(b, np.float64)[:, :3]
    C = np.empty((len(a), len(b)))
    for k in range(0, len(a), 512):  # (rows in blocks: the (n, n, 3) differences of 3072 points would be 226 MB)
        C[k:k + 512] = np.sqrt(((a[k:k + 512, None, :] - b[None, :, :]) ** 2).sum(-1))
    return C


def hungarian(C):
    """Exact minimum-cost assignment of a square float64 matrix in O(n^3) (shortest augmenting paths with potentials).
    -> (assignment (n,) int64: row i takes column assignment[i], total cost)"""
    C = np.asarray(C, np.float64)
    n = C.shape[0]
    assert C.shape == (n, n) and n >= 1
    u, v = np.zeros(n + 1), np.zeros(n + 1)
    match = np.zeros(n + 1, np.int64)  # match[j]: the row of column j (1-based; 0 = none)
    way = np.zeros(n + 1, np.int64)
    for i in range(1, n + 1):
        match[0] = i
        j0 = 0
        minv = np.full(n + 1, np.inf)
        used = np.zeros(n + 1, bool)
        while True:
            used[j0] = True
            i0 = match[j0]
            cur = C[i0 - 1] - u[i0] - v[1:]
            free = ~used[1:]
            better = free & (cur < minv[1:])
            minv[1:][better] = cur[better]
            way[1:][better] = j0
            cand = np.where(free, minv[1:], np.inf)
            j1 = int(cand.argmin()) + 1
            delta = cand[j1 - 1]
            u[match[used]] += delta
            v[used] -= delta
            minv[1:][free] -= delta
            j0 = j1
            if match[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            match[j0] = match[j1]
            j0 = j1
    assignment = np.empty(n, np.int64)
    assignment[match[1:] - 1] = np.arange(n)
    return assignment, float(C[np.arange(n), assignment].sum())


def brute_force(C):
    """The minimum over all permutations (n <= 7)"""
    C = np.asarray(C, np.float64)
    n = C.shape[0]
    assert n <= 7
    rows = np.arange(n)
    return min(float(C[rows, list(s)].sum()) for s in itertools.permutations(range(n)))


def dual_bound(C, prices):
    """``sum_i min_j (c_ij + p_j) - sum_j p_j``: a lower bound of the minimum assignment cost for ANY prices (weak duality)"""
    C, p = np.asarray(C, np.float64), np.asarray(prices, np.float64)
    return float((C + p[None, :]).min(axis=1).sum() - p.sum())


def cost_of(C, assignment):
    C, s = np.asarray(C, np.float64), np.asarray(assignment, np.int64)
    return float(C[np.arange(C.shape[0]), s].sum())


def is_permutation(assignment, n):
    return np.array_equal(np.sort(np.asarray(assignment, np.int64)), np.arange(n))


# ---- clouds --------------------------------------------------------------------------------------------------------------------------------
def gaussian(seed, n, scale=30.0, offset=0.0):
    """(n,4) float32 normal points, as in tests/test_hip_geometry.py"""
    g = np.random.Generator(np.random.PCG64(seed))
    return (g.standard_normal((n, 4)) * scale + offset).astype(np.float32)


def rings(seed, n):
    """(n,4) float32, LiDAR-like: 64 beams (elevations +3 .. -25 degrees) from a sensor 1.7 m above a ground plane, inside walls 10 to 30 m
    away (one distance per 22.5-degree sector), 2 cm of range noise: dense rings near the sensor, sparse far structure."""
    g = np.random.Generator(np.random.PCG64(seed))
    el = np.deg2rad(np.linspace(3.0, -25.0, 64))[np.arange(n) % 64]
    az = g.uniform(-math.pi, math.pi, n)
    walls = g.uniform(10.0, 30.0, 16)
    r = walls[((az + math.pi) / (2 * math.pi) * 16).astype(np.int64) % 16] / np.cos(el)
    down = el < 0
    r[down] = np.minimum(r[down], 1.7 / np.sin(-el[down]))
    r = r + g.normal(0.0, 0.02, n)
    out = np.zeros((n, 4), np.float32)
    out[:, 0], out[:, 1], out[:, 2] = r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)
    out[:, 3] = g.uniform(0.0, 1.0, n)
    return out


# ---- the kernel's auction in numpy fp32 (a check of the test inputs on the CPU, not a reference for bits) -----------------------------------
def auction_fp32(a, b, eps=0.01, max_rounds=1 << 20):
    """Forward auction with epsilon-scaling (theta = 4, from max(C_hi / 2, eps) down to eps; Jacobi rounds; fp32 costs, prices and bids; a bid
    tie goes to the lowest person, a value tie to the lowest object).  -> dict(assignment, prices float32, rounds, converged)"""
    a, b = np.asarray(a, np.float32)[:, :3], np.asarray(b, np.float32)[:, :3]
    n = len(a)
    d = a[:, None, :] - b[None, :, :]
    C = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(np.float32)
    both = np.concatenate([a, b])
    ext = (both.max(0) - both.min(0)).astype(np.float32)
    c_hi = np.float32(np.sqrt(np.float32((ext * ext).sum())))
    eps = np.float32(eps)
    cur = max(np.float32(0.5) * c_hi, eps)
    price = np.zeros(n, np.float32)
    rounds = 0
    while True:
        owner, obj = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
        while True:
            un = np.flatnonzero(obj < 0)
            if un.size == 0:
                break
            if rounds == max_rounds:
                return {"assignment": obj, "prices": price, "rounds": rounds, "converged": False}
            W = C[un] + price[None, :]
            j1 = W.argmin(1)  # (the first occurrence: the lowest object)
            w1 = W[np.arange(un.size), j1]
            if n > 1:
                W[np.arange(un.size), j1] = np.inf
                w2 = W.min(1)
            else:
                w2 = w1
            bid = price[j1] + ((w2 - w1) + cur)
            for j in np.unique(j1):
                who = np.flatnonzero(j1 == j)
                k = who[np.flatnonzero(bid[who] == bid[who].max())[0]]  # (un ascends: the lowest person)
                if owner[j] >= 0:
                    obj[owner[j]] = -1
                owner[j], obj[un[k]], price[j] = un[k], j, bid[k]
            rounds += 1
        if cur == eps:
            return {"assignment": obj, "prices": price, "rounds": rounds, "converged": True}
        cur = max(np.float32(0.25) * cur, eps)
