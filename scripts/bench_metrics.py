#!/usr/bin/env python3
"""Times the BEV metrics of evaluate.py at its sizes on one GPU and prints one JSON line:
  - histograms of 10,000 scans of 64 x 1024 in the sample layout (r2dm_amd.metrics.bev_histograms, batches of --batch);
  - the MMD of 10,000 x 10,000 histograms of D = 10,000 bins (r2dm_amd.metrics.compute_mmd_2d);
  - baselines with the reference's formulas on the same inputs: torch.histogramdd per scan on the CPU (timed on
    --cpu-scans scans, scaled to 10,000) and the torch.cdist RBF MMD in fp32 on the GPU."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from r2dm_amd import metrics  # noqa: E402


def gpu_time(fn, reps=1):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / reps, out


def ref_mmd(p_h, q_h, sigma=0.5):
    """The reference's compute_mmd_2d arithmetic (fp32, cdist matrices)."""
    p = p_h / p_h.sum(1, keepdim=True)
    q = q_h / q_h.sum(1, keepdim=True)
    k = lambda a, b: torch.exp(-torch.cdist(a, b) ** 2 / (2 * sigma**2))
    return (k(p, p).mean() + k(q, q).mean() - 2 * k(p, q).mean()).item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=10_000)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--sets", type=int, default=10_000, help="rows of each MMD set")
    ap.add_argument("--cpu-scans", type=int, default=100)
    ap.add_argument("--no-baselines", action="store_true")
    args = ap.parse_args()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)

    # scans in the sample layout: depth in [0, 80), xyz along random directions at that depth
    B, H, W = args.batch, 64, 1024
    depth = torch.rand(B, 1, H, W, device=dev, generator=g) * 80
    d = torch.randn(B, 3, H, W, device=dev, generator=g)
    imgs = torch.cat([depth, d / d.norm(dim=1, keepdim=True) * depth, torch.rand(B, 1, H, W, device=dev, generator=g)], 1).contiguous()
    del d
    metrics.bev_histograms(imgs)  # warm-up
    reps = max(1, args.scans // B)
    t_hist, h = gpu_time(lambda: metrics.bev_histograms(imgs), reps)
    t_hist *= args.scans / B
    res = {"hist_scans": args.scans, "hist_s": round(t_hist, 5), "hist_GBps": round(args.scans * 4 * H * W * 4 / t_hist / 1e9, 1)}

    # MMD sets: Poisson counts around two nearby occupancy maps
    N, D = args.sets, 10_000
    lam = torch.rand(D, device=dev, generator=g) * 0.4
    P = torch.poisson(lam.expand(N, D).contiguous(), generator=g)
    Q = torch.poisson((lam * (1 + 0.2 * torch.rand(D, device=dev, generator=g))).expand(N, D).contiguous(), generator=g)
    metrics.compute_mmd_2d(P[:256], Q[:256])  # warm-up
    t_mmd, mmd = gpu_time(lambda: metrics.compute_mmd_2d(P, Q))
    pairs = N * N + N * (N + 1)  # P x Q and the two upper triangles
    res.update({"mmd_sets": N, "mmd_bins": D, "mmd_s": round(t_mmd, 5), "mmd": mmd,
                "mmd_pair_bins_per_s": float(f"{pairs * D / t_mmd:.4g}")})

    if not args.no_baselines:
        # reference histograms: torch.histogramdd on the CPU, one scan at a time (evaluate.py's loop)
        clouds = (imgs[: args.cpu_scans, 1:4] * ((imgs[: args.cpu_scans, :1] > 0.5) & (imgs[: args.cpu_scans, :1] < 63))).flatten(2).transpose(1, 2).cpu()
        t0 = time.perf_counter()
        for pc in clouds:
            dd = pc.norm(p=2, dim=1)
            torch.histogramdd(pc[(dd > 3) & (dd < 70), 0:2], bins=100, range=[-80.0, 80.0, -80.0, 80.0])
        t_cpu = (time.perf_counter() - t0) / len(clouds) * args.scans
        res.update({"ref_hist_cpu_s": round(t_cpu, 3), "ref_hist_cpu_scans_timed": len(clouds)})
        ref_mmd(P[:256], Q[:256])  # warm-up
        t_ref, v_ref = gpu_time(lambda: ref_mmd(P, Q))
        res.update({"ref_mmd_cdist_gpu_s": round(t_ref, 4), "ref_mmd": v_ref})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
