#!/usr/bin/env python3
"""Times the earth mover's distance (r2dm_emd_pairs, r2dm_amd.geometry.emd_pairs) on one GPU and prints one JSON line: for ``--pairs`` (256)
cloud pairs of 512, 1024 and 2048 points, Gaussian (scale 30) and LiDAR-like (``rings``) clouds from the tests' generators
(tests/emd_oracle.py), the seconds per call, cloud pairs per second, the mean and the largest number of bidding rounds and the largest
certified gap.  One workgroup solves one pair, so a call of 256 pairs is one wave of workgroups on the 256 CUs and lasts as long as its
slowest pair; ``--pairs`` above that measures throughput.

The standard recipe: a warm-up call of every configuration, then ``--windows`` alternating timed windows of ``--reps`` calls each between
HIP events; medians and the spread of the windows are reported.  Where scipy is installed the host solver
(``scipy.optimize.linear_sum_assignment`` on the float64 cost matrix) is timed on one pair of each configuration, and the distance it finds
is compared with the kernel's bracket.  For the record: no bar is attached to any of these numbers."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import emd_oracle as O  # noqa: E402
from r2dm_amd import geometry  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--points", type=int, nargs="+", default=[512, 1024, 2048])
    ap.add_argument("--eps", type=float, default=0.01)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=1)
    args = ap.parse_args()
    dev, P = "cuda", args.pairs
    fns, host = {}, {}
    for kind in ("gaussian", "rings"):
        for n in args.points:
            make = (lambda s: O.gaussian(s, n)) if kind == "gaussian" else (lambda s: O.rings(s, n))
            a, b = np.concatenate([make(2 * k) for k in range(P)]), np.concatenate([make(2 * k + 1) for k in range(P)])
            da, db, off = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), np.arange(P + 1) * n
            fns[f"{kind}_{n}"] = lambda da=da, db=db, off=off: geometry.emd_pairs(da, off, db, off, eps=args.eps)
            host[f"{kind}_{n}"] = (a[:n], b[:n])
    result = {"pairs": P, "eps": args.eps, "windows": args.windows, "reps": args.reps}
    first = {name: fn() for name, fn in fns.items()}  # (the warm-up)
    times = {name: [] for name in fns}
    for _ in range(args.windows):
        for name, fn in fns.items():
            times[name].append(window(fn, args.reps))
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError:
        linear_sum_assignment = None
    for name, t in times.items():
        out = first[name]
        med = statistics.median(t)
        entry = {"median_s": float(f"{med:.4e}"), "min_s": float(f"{min(t):.4e}"), "max_s": float(f"{max(t):.4e}"),
                 "pairs_per_s": float(f"{P / med:.4e}"), "mean_rounds": round(out["rounds"].double().mean().item(), 1),
                 "max_rounds": int(out["rounds"].max().item()), "max_gap": float(f"{(out['emd'] - out['lower']).max().item():.4e}")}
        if linear_sum_assignment is not None:
            C = O.cost_matrix(*host[name])
            t0 = time.perf_counter()
            r, c = linear_sum_assignment(C)
            entry["scipy_s_per_pair"] = float(f"{time.perf_counter() - t0:.4e}")
            best = C[r, c].mean()
            entry["scipy_inside_bracket"] = bool(out["lower"][0].item() * (1 - 1e-6) <= best <= out["emd"][0].item() * (1 + 1e-6))
            entry["emd_minus_optimum"] = float(f"{out['emd'][0].item() - best:.4e}")
        result[name] = entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
