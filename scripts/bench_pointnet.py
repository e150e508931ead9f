#!/usr/bin/env python3
"""Times the PointNet feature extractor of the FPD on one GPU and prints one JSON line:
  - the fused HIP extractor (r2dm_amd.pointnet) on --batch sample-layout images of 64 x 1024 (65 536 points each): clouds/s, and the
    share of the matrix-core bound (3 fp16 products per multiply-add: 3 x 36.6 GFLOP per cloud against 2.5 PFLOP/s dense fp16);
  - the baseline: the same network layer by layer in fp32 torch on the same device (tests/pointnet_oracle.py, the activations in HBM,
    --chunk clouds at a time) -- the yardstick, not the code under test;
  - the largest difference between the two, and the time of the extractor over a 10 000-sample evaluation (generated set only)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pointnet_oracle as O  # noqa: E402
from r2dm_amd import pointnet, synthetic  # noqa: E402

MACS_PER_CLOUD_POINT = 2 * (3 * 64 + 64 * 128 + 128 * 1024)  # two trunks
PEAK_FP16 = 2.5e15


def gpu_time(fn, reps):
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
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=4, help="clouds per call of the torch baseline (its activations are 0.3 GB per cloud)")
    ap.add_argument("--samples", type=int, default=10_000, help="size of the evaluation the total is scaled to")
    args = ap.parse_args()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    B, H, W = args.batch, args.height, args.width
    N = H * W
    depth = torch.rand(B, 1, H, W, device=dev, generator=g) * 80
    d = torch.randn(B, 3, H, W, device=dev, generator=g)
    imgs = torch.cat([depth, d / d.norm(dim=1, keepdim=True) * depth, torch.rand(B, 1, H, W, device=dev, generator=g)], 1).contiguous()
    del d

    state = synthetic.synthetic_pointnet_state(0)
    ext = pointnet.pretrained_pointnet(state, device=dev)
    pointnet.pointnet_features(ext, imgs)  # warm-up
    t_hip, feats = gpu_time(lambda: pointnet.pointnet_features(ext, imgs), args.reps)
    flop = 2.0 * MACS_PER_CLOUD_POINT * N
    res = {"batch": B, "points": N, "hip_s": round(t_hip, 5), "hip_clouds_per_s": round(B / t_hip, 1),
           "GFLOP_per_cloud": round(flop / 1e9, 1), "matrix_core_bound_fraction": round(3 * flop * B / t_hip / PEAK_FP16, 4),
           "eval_samples": args.samples, "eval_extractor_s": round(t_hip / B * args.samples, 2)}

    sd = {k: v.to(dev) for k, v in state.items()}
    clouds = O.sample_clouds(imgs)

    def baseline():
        return torch.cat([O.features(sd, clouds[k:k + args.chunk]) for k in range(0, B, args.chunk)])

    with torch.no_grad():
        baseline()  # warm-up
        t_ref, ref = gpu_time(baseline, max(1, args.reps // 3))
    res.update({"torch_fp32_s": round(t_ref, 5), "torch_fp32_clouds_per_s": round(B / t_ref, 1), "speedup": round(t_ref / t_hip, 2),
                "max_abs_diff": float((feats - ref).abs().max())})

    # the distribution metrics at the evaluation's size: two sets of `samples` features
    import time

    import numpy as np

    from r2dm_amd import metrics

    f1 = torch.randn(args.samples, pointnet.FEATURE_DIM, device=dev, generator=g)
    f2 = torch.randn(args.samples, pointnet.FEATURE_DIM, device=dev, generator=g) * 1.1 + 0.05
    metrics.feature_moments(f1[:64])
    t_mom, _ = gpu_time(lambda: metrics.feature_moments(f1), 1)
    metrics.compute_squared_mmd(f1[:128], f2[:128], num_subsets=2, rng=np.random.RandomState(0))
    t_mmd, mmd = gpu_time(lambda: metrics.compute_squared_mmd(f1, f2, rng=np.random.RandomState(0)), 1)
    t0 = time.perf_counter()
    fd = metrics.compute_frechet_distance(f1, f2)
    t_fd = time.perf_counter() - t0
    res.update({"moments_s": round(t_mom, 4), "squared_mmd_s": round(t_mmd, 4), "frechet_s": round(t_fd, 2), "squared_mmd": mmd,
                "frechet_distance": fd, "eval_fpd_s": round(t_hip / B * args.samples + t_mmd + t_fd, 2)})
    print(json.dumps(res))
    if t_hip > t_ref:
        raise SystemExit("the fused extractor is slower than the layer-by-layer torch baseline")


if __name__ == "__main__":
    main()
