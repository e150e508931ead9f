#!/usr/bin/env python3
"""Times the RangeNet-53 extractor of the FRD on one GPU and prints one JSON line:
  - the HIP extractor (r2dm_amd.rangenet), ``extract(feature="lidargen")`` on --batch images of 64 x 1024 with synthetic weights:
    images/s, median and spread over --reps timed runs after a warm-up, and the share of the matrix-core bound (3 fp16 products per
    multiply-add against 2.5 PFLOP/s dense fp16);
  - the baseline: the same network in fp32 torch on the same device (tests/rangenet_oracle.py: F.conv2d / F.conv_transpose2d /
    F.batch_norm, --chunk images at a time) -- the test oracle run in fp32, the yardstick, not the code under test;
  - the largest difference between the two decoder features, and the extractor's time over a 10 000-sample evaluation.
``--only hip`` times the extractor alone (for a kernel trace)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rangenet_oracle as O  # noqa: E402
from r2dm_amd import rangenet, synthetic  # noqa: E402

PEAK_FP16 = 2.5e15


def macs_per_image(H, W, backbone=53, classes=20):
    """multiply-adds of one forward pass, from the layer shapes"""
    total, w = 9 * 5 * 32 * H * W, W
    ch = lambda i: 32 << i
    for i, n in enumerate(rangenet.RESIDUAL_BLOCKS[backbone], 1):
        w //= 2
        total += H * w * (9 * ch(i - 1) * ch(i) + n * (ch(i) * ch(i - 1) + 9 * ch(i - 1) * ch(i)))
    for i in range(5, 0, -1):
        w *= 2
        total += H * w * (2 * ch(i) * ch(i - 1) + ch(i - 1) * ch(i) + 9 * ch(i) * ch(i - 1))
    return total + 9 * 32 * classes * H * W


def gpu_times(fn, reps):
    """seconds of each of ``reps`` runs (device events), and the last result"""
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / 1e3)
    return times, out


def summary(times):
    return {"median_s": round(statistics.median(times), 5), "min_s": round(min(times), 5), "max_s": round(max(times), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=8, help="images per call of the torch baseline")
    ap.add_argument("--samples", type=int, default=10_000, help="size of the evaluation the total is scaled to")
    ap.add_argument("--only", choices=["hip"], default=None)
    args = ap.parse_args()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    B, H, W = args.batch, args.height, args.width
    depth = torch.rand(B, 1, H, W, device=dev, generator=g) * 70
    d = torch.randn(B, 3, H, W, device=dev, generator=g)
    imgs = torch.cat([depth, d / d.norm(dim=1, keepdim=True) * depth, torch.rand(B, 1, H, W, device=dev, generator=g)], 1).contiguous()
    del d

    state = synthetic.synthetic_rangenet_state(0)
    ext = rangenet.RangeNetExtractor(state, device=dev)
    ext.extract(imgs)  # warm-up
    t_hip, feats = gpu_times(lambda: ext.extract(imgs), args.reps)
    flop = 2.0 * macs_per_image(H, W)
    med = statistics.median(t_hip)
    res = {"batch": B, "height": H, "width": W, "hip": summary(t_hip), "hip_images_per_s": round(B / med, 1),
           "GFLOP_per_image": round(flop / 1e9, 1), "matrix_core_bound_fraction": round(3 * flop * B / med / PEAK_FP16, 4),
           "eval_samples": args.samples, "eval_extractor_s": round(med / B * args.samples, 1)}
    if args.only is None:
        sd = O.cast(state, torch.float32, dev)
        index = torch.tensor(rangenet.subsample_indices(32 * H * W), device=dev)

        def baseline():
            parts = [O.forward(sd, O.preprocess(imgs[k:k + args.chunk]), 53)[0].flatten(1)[:, index] for k in range(0, B, args.chunk)]
            return torch.cat(parts)

        with torch.no_grad():
            baseline()  # warm-up (the library picks its algorithms)
            t_ref, ref = gpu_times(baseline, args.reps)
        med_ref = statistics.median(t_ref)
        res.update({"torch_fp32": summary(t_ref), "torch_fp32_images_per_s": round(B / med_ref, 1), "speedup": round(med_ref / med, 2),
                    "max_abs_diff": float((feats - ref).abs().max()), "max_abs_feature": float(ref.abs().max())})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
