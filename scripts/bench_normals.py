#!/usr/bin/env python3
"""Times the surface normals on one GPU and prints one JSON line: r2dm_amd.render.estimate_surface_normal at batch 64 of 64 x 1024 in
both modes, and r2dm_amd.render.render_normals at batch 8 and 800 x 800 pixels, each against the torch composition the reference
executes there (tests/normals_oracle.py in fp32 on the same GPU and inputs), after comparing the outputs.  Every pair is timed in
alternating windows; the medians and the spread of the windows are reported, and for the normals the fraction of the HBM bound that
the 24 bytes per pixel (12 read, 12 written) make of the median."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import make_golden_normals as G  # noqa: E402  (the scenes of the tests)
import normals_oracle as O  # noqa: E402
from r2dm_amd import render  # noqa: E402
from r2dm_amd.lidar import LiDARUtility  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, the MI355X's specification


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


def compare(hip, composition, windows, hip_reps, torch_reps):
    """Alternating timed windows after a warm-up of each -> (median, min, max) seconds per call of both."""
    hip(), composition()
    th, tt = [], []
    for _ in range(windows):
        th.append(window(hip, hip_reps))
        tt.append(window(composition, torch_reps))
    stats = lambda t: {"median_s": float(f"{statistics.median(t):.4e}"), "min_s": float(f"{min(t):.4e}"), "max_s": float(f"{max(t):.4e}")}
    return stats(th), stats(tt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64, help="images of estimate_surface_normal")
    ap.add_argument("--view-batch", type=int, default=8, help="frames of render_normals")
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--d", type=int, default=2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--hip-reps", type=int, default=50)
    ap.add_argument("--torch-reps", type=int, default=3)
    args = ap.parse_args()
    dev, res = "cuda", (64, 1024)
    lu = LiDARUtility(res, "log_depth", G.MIN_DEPTH, G.MAX_DEPTH)
    trig = O.ray_trig(lu.ray_angles).to(dev)
    scenes = torch.from_numpy(G.depth_scene(1000, (8, *res))).to(dev)
    depth = scenes.repeat(-(-args.batch // 8), 1, 1, 1)[:args.batch].contiguous()
    xyz = O.frame_xyz(depth, trig, G.MIN_DEPTH, G.MAX_DEPTH)
    pixels = xyz.numel() // 3
    out = {"batch": args.batch, "resolution": list(res), "d": args.d, "windows": args.windows}
    for mode in G.MODES:
        hip = lambda: render.estimate_surface_normal(xyz, args.d, mode)
        composition = lambda: O.estimate_surface_normal(xyz, args.d, mode)
        got, want = hip(), composition()
        differ = (got.view(torch.int32) != want.view(torch.int32)).any(1)
        th, tt = compare(hip, composition, args.windows, args.hip_reps, args.torch_reps)
        out[f"normals_{mode}"] = {"pixels_differing": int(differ.sum()), "max_abs_diff": float(f"{(got - want).abs().max().item():.3e}"), "hip": th,
                                  "torch": tt, "ratio": round(tt["median_s"] / th["median_s"], 1),
                                  "hbm_bound_fraction": round(24 * pixels / HBM_PEAK / th["median_s"], 3)}
        del got, want
    metric = depth[:args.view_batch]
    hip = lambda: render.render_normals(metric, lu, size=args.size, d=args.d, trig=trig)
    composition = lambda: O.render_normals(metric, trig, G.MIN_DEPTH, G.MAX_DEPTH, args.size, args.d)
    (c, bev), (c_r, bev_r) = hip(), composition()
    diff = (bev - bev_r).abs()
    th, tt = compare(hip, composition, args.windows, max(1, args.hip_reps // 5), args.torch_reps)
    out["render_normals"] = {"frames": int(metric.shape[0]), "size": args.size,
                             "colour_pixels_differing": int((c.view(torch.int32) != c_r.view(torch.int32)).any(1).sum()),
                             "bev_pixels_over_1e-3": int((diff.amax(1) > 1e-3).sum()), "bev_rms_diff": float(f"{diff.pow(2).mean().sqrt().item():.3e}"),
                             "hip": th, "torch": tt, "ratio": round(tt["median_s"] / th["median_s"], 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
