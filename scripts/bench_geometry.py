#!/usr/bin/env python3
"""Times the nearest-neighbour search behind the geometry metrics (r2dm_nn_pairs, r2dm_amd.geometry) on one GPU and prints one JSON line:

  (a) ``--pairs`` (8) pairs of clouds of 64 x 1024 = 65 536 points, both directions, sums only (``chamfer_sums``);
  (b) the ``--sets`` x ``--sets`` (256 x 256) matrix of squared Chamfer distances between clouds of 2 048 points (``pairwise_chamfer``).

The comparison is the torch composition on the same GPU and inputs: ``torch.cdist`` on chunks that fit in memory, ``min`` along both axes of
every chunk (one distance matrix serves both directions), squares and means.  It is timed as torch ships it (for these sizes ``cdist`` takes
the matrix-multiply form |a|^2 + |b|^2 - 2ab) in alternating windows with the kernel, HIP events; medians and the spread of the windows
are reported, the ratio of the medians, the largest relative difference of the results, and the fraction of the VALU floor the kernel
reaches: 7 instructions per point pair and direction (3 subtractions, a multiply, 2 FMAs, a minimum) at the datasheet's 157.3 TFLOP/s,
which counts an FMA as two operations: 78.65e12 vector instructions per second.

``torch_exact`` is the same composition with ``compute_mode="donot_use_mm_for_euclid_dist"``, the form with the kernel's arithmetic.  Its
kernel takes one block per distance, so a call may hold at most 2^24 distances and the full shapes would take minutes: it is timed on
``--exact_pairs`` (1) of the large pairs and on an ``--exact_sets`` x ``--exact_sets`` (4 x 4) corner of the matrix, and every
implementation's time is also given per cloud pair (``per_pair_s``), which is what ``ratio_torch_exact`` compares."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from r2dm_amd import geometry  # noqa: E402

VALU_PEAK = 157.3e12 / 2  # fp32 vector instructions / s: the MI355X's specified 157.3 TFLOP/s counts an FMA as two operations
OPS_PER_PAIR = 7
CHUNK_BYTES = 1 << 30  # of one cdist result
EXACT_CHUNK_BYTES = 4 << 23  # ... without the matrix multiply: one block of 256 threads per distance, below 2^32 threads per launch


MODES = {"torch": "use_mm_for_euclid_dist_if_necessary", "torch_exact": "donot_use_mm_for_euclid_dist"}


def window(fn, reps):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    del out
    return a.elapsed_time(b) / 1e3 / reps


def stats(t):
    return {"median_s": float(f"{statistics.median(t):.4e}"), "min_s": float(f"{min(t):.4e}"), "max_s": float(f"{max(t):.4e}")}


def compare(fns, windows, reps):
    """Alternating timed windows after a warm-up of each -> per function (median, min, max) seconds per call."""
    for fn in fns.values():
        fn()
    times = {name: [] for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            times[name].append(window(fn, reps[name]))
    return {name: stats(t) for name, t in times.items()}


def torch_cd_sq_pair(a, b, mode):
    """cd_sq of two (n,3) clouds: cdist over chunks of a's rows, running minima for b"""
    rows = max(1, (EXACT_CHUNK_BYTES if mode == MODES["torch_exact"] else CHUNK_BYTES) // (4 * b.shape[0]))
    mins_a, min_b = [], None
    for k in range(0, a.shape[0], rows):
        d = torch.cdist(a[k:k + rows], b, compute_mode=mode)
        mins_a.append(d.min(dim=1).values)
        m = d.min(dim=0).values
        min_b = m if min_b is None else torch.minimum(min_b, m)
    return torch.cat(mins_a).double().pow(2).mean() + min_b.double().pow(2).mean()


def torch_cd_sq_matrix(A, B, mode):
    """(Na,Nb) cd_sq of (Na,n,3) against (Nb,n,3): per cloud of A a batched cdist against chunks of B"""
    Na, n, _ = A.shape
    cols = max(1, (EXACT_CHUNK_BYTES if mode == MODES["torch_exact"] else CHUNK_BYTES) // (4 * n * n))
    out = torch.empty(Na, B.shape[0], dtype=torch.float64, device=A.device)
    for i in range(Na):
        for j in range(0, B.shape[0], cols):
            d = torch.cdist(A[i][None].expand(min(cols, B.shape[0] - j), n, 3), B[j:j + cols], compute_mode=mode)
            out[i, j:j + cols] = d.min(dim=2).values.double().pow(2).mean(1) + d.min(dim=1).values.double().pow(2).mean(1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--points", type=int, default=64 * 1024)
    ap.add_argument("--sets", type=int, default=256)
    ap.add_argument("--set_points", type=int, default=2048)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch_reps", type=int, default=1)
    ap.add_argument("--exact_pairs", type=int, default=1)
    ap.add_argument("--exact_sets", type=int, default=4)
    args = ap.parse_args()
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(0)
    reps = {"hip": args.reps, "torch": args.torch_reps, "torch_exact": args.torch_reps}
    result = {"windows": args.windows, "reps": reps, "valu_peak": VALU_PEAK, "ops_per_point_pair": OPS_PER_PAIR}

    # (a) few large pairs: LiDAR-like clouds, 30 m wide
    P, n = args.pairs, args.points
    a = torch.randn(P * n, 4, generator=gen, device=dev) * 30
    b = a + torch.randn(P * n, 4, generator=gen, device=dev) * 0.5
    off = [k * n for k in range(P + 1)]
    fns = {"hip": lambda: geometry.chamfer_from_sums(geometry.chamfer_sums(a, off, b, off))["cd_sq"]}
    done = {"hip": P, "torch": P, "torch_exact": min(P, args.exact_pairs)}  # cloud pairs per call
    for name, mode in MODES.items():
        fns[name] = lambda mode=mode, k_end=done[name]: torch.stack([torch_cd_sq_pair(a[k * n:(k + 1) * n, :3], b[k * n:(k + 1) * n, :3], mode)
                                                                     for k in range(k_end)])
    got = {name: fn() for name, fn in fns.items()}
    entry = compare(fns, args.windows, reps)
    floor = 2 * P * n * n * OPS_PER_PAIR / VALU_PEAK
    entry.update(pairs=P, points=n, floor_s=float(f"{floor:.4e}"), fraction_of_floor=round(floor / entry["hip"]["median_s"], 3))
    for name in fns:
        entry[name].update(cloud_pairs=done[name], per_pair_s=float(f"{entry[name]['median_s'] / done[name]:.4e}"))
    for name in MODES:
        entry[f"ratio_{name}"] = round(entry[name]["per_pair_s"] / entry["hip"]["per_pair_s"], 2)
        k = done[name]
        entry[f"max_rel_diff_{name}"] = float(f"{((got[name] - got['hip'][:k]).abs() / got['hip'][:k]).max().item():.3e}")
    result["large_pairs"] = entry
    del a, b, got

    # (b) many small pairs: the matrix of the set metrics
    N, m = args.sets, args.set_points
    A = torch.randn(N, m, 4, generator=gen, device=dev) * 30
    B = torch.randn(N, m, 4, generator=gen, device=dev) * 30
    counts = torch.full((N,), m, dtype=torch.int64, device=dev)
    fns = {"hip": lambda: geometry.pairwise_chamfer(A, counts, B, counts)}
    A3, B3 = A[..., :3].contiguous(), B[..., :3].contiguous()
    E = min(N, args.exact_sets)
    done = {"hip": N * N, "torch": N * N, "torch_exact": E * E}
    fns["torch"] = lambda: torch_cd_sq_matrix(A3, B3, MODES["torch"])
    fns["torch_exact"] = lambda: torch_cd_sq_matrix(A3[:E], B3[:E], MODES["torch_exact"])
    got = {name: fn() for name, fn in fns.items()}
    entry = compare(fns, args.windows, reps)
    floor = 2 * N * N * m * m * OPS_PER_PAIR / VALU_PEAK
    entry.update(sets=N, points=m, floor_s=float(f"{floor:.4e}"), fraction_of_floor=round(floor / entry["hip"]["median_s"], 3))
    for name in fns:
        entry[name].update(cloud_pairs=done[name], per_pair_s=float(f"{entry[name]['median_s'] / done[name]:.4e}"))
    for name, k in (("torch", N), ("torch_exact", E)):
        entry[f"ratio_{name}"] = round(entry[name]["per_pair_s"] / entry["hip"]["per_pair_s"], 2)
        entry[f"max_rel_diff_{name}"] = float(f"{((got[name] - got['hip'][:k, :k]).abs() / got['hip'][:k, :k]).max().item():.3e}")
    result["matrix"] = entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
