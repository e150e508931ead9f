"""Plain numpy / float64 brute force of the geometry metrics' definitions (r2dm_amd/geometry.py), run on the same float32 inputs.

Clouds are (n,>=3) arrays whose first three columns are x, y, z in metres; ``d(x, Y) = min_y |x - y|``."""
import math

import numpy as np

RAW_NAMES = ("sum_sq_ab", "sum_d_ab", "within_ab", "sum_sq_ba", "sum_d_ba", "within_ba", "count_a", "count_b")


def sq_distances(a, b):
    """(|a|,|b|) float64 squared distances, in the difference form"""
    a, b = np.asarray(a, np.float64)[:, :3], np.asarray(b, np.float64)[:, :3]
    return ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)


def nearest(a, b):
    """for every point of a: (d^2 to its nearest neighbour in b, that neighbour's index -- the lowest on a tie); (+inf, -1) for an empty b"""
    if len(b) == 0:
        return np.full(len(a), np.inf), np.full(len(a), -1, np.int64)
    D = sq_distances(a, b)
    idx = D.argmin(1)  # numpy: the first occurrence
    return D[np.arange(len(a)), idx], idx.astype(np.int64)


def second_best_gap(a, b):
    """the smallest relative gap (d2_second - d2_best) / d2_second over the points of a (inf when b has fewer than two points)"""
    if len(b) < 2 or len(a) == 0:
        return math.inf
    D = np.sort(sq_distances(a, b), axis=1)
    return float(((D[:, 1] - D[:, 0]) / D[:, 1]).min())


def raw_sums(a, b, tau):
    """the eight raw values of a pair (RAW_NAMES)"""
    dab, _ = nearest(a, b)
    dba, _ = nearest(b, a)
    return np.array([dab.sum(), np.sqrt(dab).sum(), (np.sqrt(dab) <= tau).sum(), dba.sum(), np.sqrt(dba).sum(), (np.sqrt(dba) <= tau).sum(),
                     len(a), len(b)], np.float64)


def chamfer(a, b, tau=0.2):
    """cd_sq, cd, precision, recall, fscore of a pair (a is the prediction); all NaN if a cloud is empty"""
    if len(a) == 0 or len(b) == 0:
        return {k: math.nan for k in ("cd_sq", "cd", "precision", "recall", "fscore")}
    dab, dba = np.sqrt(nearest(a, b)[0]), np.sqrt(nearest(b, a)[0])
    p, r = float((dab <= tau).mean()), float((dba <= tau).mean())
    return {"cd_sq": float((dab ** 2).mean() + (dba ** 2).mean()), "cd": float(0.5 * (dab.mean() + dba.mean())), "precision": p, "recall": r,
            "fscore": 2 * p * r / (p + r) if p + r > 0 else 0.0}


def chamfer_matrix(A, B):
    """(len(A), len(B)) cd_sq between two lists of clouds"""
    return np.array([[chamfer(a, b)["cd_sq"] for b in B] for a in A], np.float64)


def argmin_lowest(row):
    return int(np.flatnonzero(row == row.min())[0])


def coverage(D):
    return len({argmin_lowest(D[g]) for g in range(D.shape[0])}) / D.shape[1]


def minimum_matching_distance(D):
    return math.fsum(float(D[:, r].min()) for r in range(D.shape[1])) / D.shape[1]  # (correctly rounded: no order of summation to agree on)


def one_nn_accuracy(D_gg, D_gr, D_rr):
    G, R = D_gr.shape
    M = np.block([[D_gg, D_gr], [D_gr.T, D_rr]]).astype(np.float64)
    good = 0
    for s in range(G + R):
        row = M[s].copy()
        row[s] = np.inf
        good += (argmin_lowest(row) < G) == (s < G)
    return good / (G + R)


def set_metrics(D_gg, D_gr, D_rr):
    return {"cov": coverage(D_gr), "mmd": minimum_matching_distance(D_gr), "1-nna": one_nn_accuracy(D_gg, D_gr, D_rr)}
