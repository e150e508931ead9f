#!/usr/bin/env python3
"""Generate tests/golden/bev_metrics.npz by running the REAL reference's metrics/bev.py on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_metrics.py /path/to/reference

Contents (the reference's outputs in fp32 as evaluate.py runs them, plus fp64 oracles):
  - point clouds with engineered edge cases -- coordinates on the fp32 bin edges and one ulp either side (also at +-80),
    depths on 3.0 / 70.0 and one ulp either side, masked zeros, NaN / inf -- and their histograms (uint16);
  - histograms of full-size 64x1024-point clouds regenerated from integer-only PCG64 draws (``full_cloud``);
  - sample-layout images (B,5,16,128) with depths around evaluate.py's 0.5 / 63 mask and their histograms, through the
    reference's masking (Samples + the xyz * mask of evaluate.py);
  - JSD and MMD of histogram sets regenerated from integer-only PCG64 draws (``mmd_hists``), Np != Nq included: the
    reference's values, fp64 oracles, and the reference's own error.
The two generator functions are imported by tests/test_hip_metrics.py: the inputs are platform-exact integers.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "bev_metrics.npz")
BINS, FIELD = 100, 160.0

# (name, field_size, bins, min_depth, max_depth) of the explicit edge-case clouds
CLOUD_CASES = [
    ("edges", FIELD, BINS, 3.0, 70.0),
    ("edges_wide", FIELD, BINS, 3.0, 1000.0),  # every edge, +-80 included, inside the depth window
    ("edges_bins64", 100.0, 64, 1.0, 45.0),
    ("depths", FIELD, BINS, 3.0, 70.0),
]
FULL_SEEDS = [11, 12, 13]
IMG_SHAPE = (6, 5, 16, 128)
# (seed P, seed Q, Np, Nq, shift of Q)
MMD_CASES = [(101, 202, 300, 300, 2), (103, 204, 200, 350, 1), (105, 206, 64, 17, 3), (107, 208, 129, 65, 0)]


def full_cloud(seed, n=64 * 1024):
    """(n,3) fp32 cloud from integer draws: coordinates k / 2^15 in +-75 (exact in fp32), a tenth of the points zero."""
    g = np.random.Generator(np.random.PCG64(seed))
    xyz = g.integers(-75 * 2**15, 75 * 2**15, size=(n, 3)).astype(np.float32) * np.float32(2.0**-15)
    xyz[g.integers(0, 10, size=n) == 0] = 0.0
    return xyz


def mmd_hists(seed, n, shift, bins=BINS):
    """(n, bins*bins) float32 counts: each row bins 500..3999 points whose x / y bins are sums of four integer draws."""
    g = np.random.Generator(np.random.PCG64(seed))
    out = np.zeros((n, bins * bins), dtype=np.float32)
    for r in range(n):
        m = int(g.integers(500, 4000))
        ix = np.clip(g.integers(0, 26, size=(4, m)).sum(0) + shift, 0, bins - 1)
        iy = np.clip(g.integers(0, 26, size=(4, m)).sum(0), 0, bins - 1)
        out[r] = np.bincount(ix * bins + iy, minlength=bins * bins)
    return out


def edge_cloud(g):
    import torch

    E = torch.linspace(-80.0, 80.0, BINS + 1, dtype=torch.float32).numpy()
    vals = np.concatenate([E, np.nextafter(E, np.float32(-np.inf)), np.nextafter(E, np.float32(np.inf))]).astype(np.float32)
    rnd = lambda n, a: (g.integers(-a * 2**16, a * 2**16, size=n) / 2**16).astype(np.float32)
    n = len(vals)
    pts = [np.stack([vals, rnd(n, 85), np.zeros(n, np.float32)], 1),
           np.stack([rnd(n, 85), vals, rnd(n, 2)], 1),
           np.stack([vals, g.permutation(vals), np.zeros(n, np.float32)], 1),
           np.stack([rnd(3000, 90), rnd(3000, 90), rnd(3000, 20)], 1),
           np.zeros((50, 3), np.float32),
           np.array([[np.nan, 0, 0], [np.inf, 0, 0], [0, -np.inf, 0], [5, np.nan, 0], [10, 10, np.inf]], np.float32)]
    return np.concatenate(pts).astype(np.float32)


def depth_cloud(g):
    d = g.integers(-2**20, 2**20, size=(800, 3)).astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(np.float32)
    pts = []
    for r in (np.float32(3.0), np.float32(70.0)):
        for rr in (np.nextafter(r, np.float32(0)), r, np.nextafter(r, np.float32(np.inf))):
            pts.append(d * rr)
            for ax in range(3):
                for s in (1, -1):
                    p = np.zeros((1, 3), np.float32)
                    p[0, ax] = s * rr
                    pts.append(p)
    return np.concatenate(pts).astype(np.float32)


def images(g):
    img = np.empty(IMG_SHAPE, np.float32)
    B, _, H, W = IMG_SHAPE
    img[:, 0] = g.integers(0, 80 * 2**10, size=(B, H, W)) / 2**10
    special = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1)), 63.0,
                        np.nextafter(np.float32(63), np.float32(0)), np.nextafter(np.float32(63), np.float32(100)), 0.0], np.float32)
    sel = g.integers(0, 4, size=(B, H, W)) == 0
    img[:, 0][sel] = special[g.integers(0, len(special), size=int(sel.sum()))]
    img[:, 1:4] = g.integers(-75 * 2**12, 75 * 2**12, size=(B, 3, H, W)) / 2**12
    img[:, 4] = g.integers(0, 2**12, size=(B, H, W)) / 2**12
    return img


def main(reference):
    sys.path.insert(0, reference)
    import einops
    import torch
    from metrics import bev  # (reference)

    g = np.random.Generator(np.random.PCG64(7))
    out = {}
    clouds = {"edges": edge_cloud(g), "depths": depth_cloud(g)}
    for name, field, bins, lo, hi in CLOUD_CASES:
        pc = clouds["depths" if name == "depths" else "edges"]
        h = bev.point_cloud_to_histogram(torch.from_numpy(pc), field_size=field, bins=bins, min_depth=lo, max_depth=hi).numpy()
        assert h.max() < 2**16
        out[f"hist_{name}"] = h.astype(np.uint16)
        out[f"params_{name}"] = np.array([field, bins, lo, hi], np.float64)
    out["cloud_edges"], out["cloud_depths"] = clouds["edges"], clouds["depths"]
    for s in FULL_SEEDS:
        out[f"hist_full_{s}"] = bev.point_cloud_to_histogram(torch.from_numpy(full_cloud(s))).numpy().astype(np.uint16)

    # evaluate.py's generated-sample path: Samples.__getitem__ (mask, img * mask), then xyz * mask -> (N,3) views
    img = images(g)
    out["images"] = img
    t = torch.from_numpy(img)
    depth = t[:, [0]]
    mask = torch.logical_and(depth > 0.5, depth < 63.0).float()
    t = t * mask
    clouds_img = einops.rearrange(t[:, 1:4] * mask, "B C H W -> B C (H W)")
    out["hist_images"] = np.stack([bev.point_cloud_to_histogram(einops.rearrange(c, "C N -> N C")).numpy()
                                   for c in clouds_img]).astype(np.uint16)

    # JSD / MMD: reference (fp32, CPU) against fp64 oracles
    rows = []
    for sp, sq, n_p, n_q, shift in MMD_CASES:
        P, Q = mmd_hists(sp, n_p, 0), mmd_hists(sq, n_q, shift)
        tp, tq = torch.from_numpy(P), torch.from_numpy(Q)
        jsd_ref = float(bev.compute_jsd_2d(tp, tq))
        mmd_ref = float(bev.compute_mmd_2d(tp, tq))
        from scipy.spatial.distance import jensenshannon

        s1, s2 = P.astype(np.float64).sum(0), Q.astype(np.float64).sum(0)
        jsd_64 = float(jensenshannon(s1 / s1.sum(), s2 / s2.sum()))
        p64 = tp.double() / tp.double().sum(1, keepdim=True)
        q64 = tq.double() / tq.double().sum(1, keepdim=True)
        m = lambda a, b: (-torch.expm1(-2.0 * torch.cdist(a, b, compute_mode="donot_use_mm_for_euclid_dist") ** 2)).mean().item()
        mmd_64 = 2 * m(p64, q64) - m(p64, p64) - m(q64, q64)
        rel = abs(mmd_ref - mmd_64) / abs(mmd_64)
        print(f"P{sp} x Q{sq} ({n_p} x {n_q}): jsd ref {jsd_ref:.12g} fp64 {jsd_64:.12g}; mmd ref {mmd_ref:.8g} fp64 {mmd_64:.12g} rel {rel:.2e}")
        assert rel > 2e-5, "the reference's own error must be measurable for the bar of one twentieth of it"
        rows.append([sp, sq, n_p, n_q, shift, jsd_ref, jsd_64, abs(jsd_ref - jsd_64), mmd_ref, mmd_64, abs(mmd_ref - mmd_64)])
    out["pairs"] = np.array(rows, np.float64)  # columns: seed P, seed Q, Np, Nq, shift, jsd ref, jsd fp64, |err|, mmd ref, mmd fp64, |err|
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
