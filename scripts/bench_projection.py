#!/usr/bin/env python3
"""Times the projection of raw scans to range images on one GPU and prints one JSON line: r2dm_amd.projection.project_scans on
--scans regenerated scans of about 120 k points at 64 x 2048, scan unfolding and spherical,
  - the kernels alone (points already on the device; GPU events around one call for the whole batch), and
  - end to end from ``.bin`` files on disk (read, concatenate, upload, project, synchronise; wall clock), with the file reading
    alone next to it,
against the numpy closed form of the same projection (tests/golden/make_golden_projection.py) on this host, timed on --numpy-scans
scans.  Every figure is the median of --reps runs after a warm-up, with the spread (min .. max) next to it."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import make_golden_projection as G  # noqa: E402
from r2dm_amd import projection  # noqa: E402

H, W = 64, 2048


def spread(ts, per):
    """median and (min .. max) of the runs, in ms per scan"""
    ms = [1e3 * t / per for t in ts]
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def gpu_times(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / 1e3)
    return out


def wall_times(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--numpy-scans", type=int, default=4)
    args = ap.parse_args()
    clouds = [G.centred_unfolding(H, W, rings=64, mid=bool(k % 2), seed=1000 + k, sparse=True) for k in range(args.scans)]
    offsets = np.zeros(len(clouds) + 1, np.int64)
    np.cumsum([len(c) for c in clouds], out=offsets[1:])
    points = torch.from_numpy(np.concatenate(clouds)).cuda()
    res = {"scans": args.scans, "points_per_scan": int(offsets[-1] // args.scans), "grid": [H, W], "reps": args.reps, "unit": "ms per scan"}
    with tempfile.TemporaryDirectory() as d:
        files = []
        for k, c in enumerate(clouds):
            files.append(os.path.join(d, f"{k:010d}.bin"))
            c.tofile(files[-1])
        wall_times(lambda: projection.load_scans(files), 2)  # (the page cache holds the files from here on)
        res["read_files"] = spread(wall_times(lambda: projection.load_scans(files), args.reps), args.scans)
        for mode, unfolding in (("unfolding", True), ("spherical", False)):
            kernels = lambda: projection.project_scans(points, offsets, H=H, W=W, scan_unfolding=unfolding)
            files_to_images = lambda: projection.project_scans(*projection.load_scans(files), H=H, W=W, scan_unfolding=unfolding)
            kernels(), files_to_images()  # warm-up
            got = kernels()[:args.numpy_scans].cpu().numpy()
            t = []
            for k in range(args.numpy_scans):
                t0 = time.perf_counter()
                _, want = G.project_numpy(clouds[k], H, W, unfolding, apply_mask=True)
                t.append(time.perf_counter() - t0)
                if unfolding:  # (the spherical rows of these clouds are not centred in their cells: nothing to hold to the bit there)
                    assert np.array_equal(got[k].view(np.uint32), want.view(np.uint32)), "the kernels and the numpy closed form disagree"
            res[mode] = {"kernels": spread(gpu_times(kernels, args.reps), args.scans),
                         "files_to_images": spread(wall_times(files_to_images, args.reps), args.scans),
                         "numpy_closed_form": spread(t, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
