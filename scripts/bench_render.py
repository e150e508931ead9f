#!/usr/bin/env python3
"""Times the rendering of a whole sampling run on one GPU and prints one JSON line: r2dm_amd.render.render_frames on the
(S+1) x B = 257 x 8 frames of 64 x 1024 that generate.py --render_frames renders, at 800 x 800 pixels, against the torch
composition the reference executes there (tests/render_oracle.py in fp32 on the same GPU: eight scatter_add_ per frame), timed
on --torch-frames frames."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import render_oracle as O  # noqa: E402
from r2dm_amd import render  # noqa: E402
from r2dm_amd.lidar import LiDARUtility  # noqa: E402


def gpu_time(fn, reps=1):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--chunk", type=int, default=64, help="frames per render_frames call (generate.py's)")
    ap.add_argument("--torch-frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    dev, res = "cuda", (64, 1024)
    lu = LiDARUtility(res, "log_depth", 1.45, 80.0).to(dev)
    n = (args.steps + 1) * args.batch
    # the stack of a run: the same few synthetic scans, each frame with its own noise level (early frames are noise)
    base = O.synthetic_frames(args.batch, *res, seed=0).to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    level = torch.linspace(1, 0, args.steps + 1, device=dev)[:, None, None, None, None]
    xs = (base[None] * (1 - level) + level * torch.rand(args.steps + 1, *base.shape, device=dev, generator=g)).clamp(0, 1).flatten(0, 1)
    turbo, viridis = render.colormap_lut("turbo").to(dev), render.colormap_lut("viridis").to(dev)

    def hip():
        for k in range(0, n, args.chunk):
            out = render.render_frames(xs[k:k + args.chunk], lu, size=args.size)
        return out

    def composition():
        for k in range(0, args.torch_frames, args.batch):  # batches of B frames, as the reference's loop over the stack
            out = O.render_frames(xs[n - args.torch_frames + k:n - args.torch_frames + k + args.batch], lu.ray_angles, lu.min_depth, lu.max_depth,
                                  turbo, viridis, args.size)
        return out

    hip()  # warm-up
    t_hip, (img, bev) = gpu_time(hip, args.reps)
    composition()
    t_ref, (img_r, bev_r, _) = gpu_time(composition, args.reps)
    same = (bev[-args.batch:] - bev_r).abs()
    out = {"frames": n, "size": args.size, "hip_s": round(t_hip, 4), "hip_frames_per_s": round(n / t_hip, 1),
           "torch_frames_timed": args.torch_frames, "torch_frames_per_s": round(args.torch_frames / t_ref, 1),
           "ratio": round((n / t_hip) / (args.torch_frames / t_ref), 2), "img_equal": bool(torch.equal(img[-args.batch:], img_r)),
           "bev_pixels_over_1e-3": int((same.amax(1) > 1e-3).sum()), "bev_rms_diff": float(f"{same.pow(2).mean().sqrt().item():.3e}")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
