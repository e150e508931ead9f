#!/usr/bin/env python3
"""Times the k-NN manifold metrics (precision / recall / density / coverage) on one GPU and prints one JSON line.  Per shape
(N = M real and generated features of D dimensions, k = 5, seeded inputs):
  - the fused HIP path: r2dm_amd.metrics.manifold_metrics, four passes of r2dm_feature_knn (fp64, Gram term on the fp64 matrix pipe,
    no N x M matrix); its rate is the 4 x 2 N M D flop of the four passes over the CALL time (norms, merge and host reads included), and
    "pass_tflops" the 2 N M D flop of one cross pass over that pass alone (the tile kernel is 98.5 % of it: profiles/prdc.txt);
  - the other side, the yardstick and not the code under test: the torch composition in the same arithmetic class -- fp64 x @ y.T, norms,
    kthvalue, min, comparisons, row-chunked so that the chunk of the matrix fits;
  - torch's fp64 matmul alone on the same shape, the practical ceiling of the Gram term (the guides give no fp64 matrix-pipe peak).
Both sides are warmed up, timed with device events and alternate inside one process."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from r2dm_amd import metrics  # noqa: E402

LATENT = 16


def features(n, d, shift, scale, g, A):
    """a low-dimensional latent through a fixed linear map, 5 % isotropic noise, ReLU: no metric ends at 0 or 1"""
    z = shift + scale * torch.randn(n, LATENT, device="cuda", generator=g)
    return torch.relu(z @ A + 0.05 * torch.randn(n, d, device="cuda", generator=g)).contiguous()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3, out


def torch_pass(x, y, same, k, radius2, chunk):
    """(kth2 or None, min2, count or None) of one pass in fp64 torch ops, ``chunk`` rows of the matrix at a time"""
    nx, ny = x.square().sum(1), y.square().sum(1)
    kth, mn, cnt = [], [], []
    for a in range(0, len(x), chunk):
        d = (nx[a:a + chunk, None] + ny[None, :] - 2.0 * (x[a:a + chunk] @ y.T)).clamp_min_(0.0)
        if same:
            r = torch.arange(d.shape[0], device=d.device)
            d[r, r + a] = float("inf")
        if k:
            kth.append(d.kthvalue(k, dim=1).values)
        mn.append(d.min(1).values)
        if radius2 is not None:
            cnt.append((d <= radius2[None, :]).sum(1))
    return torch.cat(kth) if k else None, torch.cat(mn), torch.cat(cnt) if radius2 is not None else None


def torch_metrics(real, fake, k, chunk):
    r, f = real.double(), fake.double()
    r2, s2 = torch_pass(r, r, True, k, None, chunk)[0], torch_pass(f, f, True, k, None, chunk)[0]
    fake_count = torch_pass(f, r, False, 0, r2, chunk)[2]
    _, min2, real_count = torch_pass(r, f, False, 0, s2, chunk)
    return {"precision": (fake_count > 0).double().mean().item(), "recall": (real_count > 0).double().mean().item(),
            "density": fake_count.sum().item() / (k * len(f)), "coverage": (min2 <= r2).double().mean().item()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 10000])
    ap.add_argument("--dims", type=int, nargs="+", default=[1808, 4096])
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=2048, help="rows of the fp64 matrix the torch composition holds at a time")
    ap.add_argument("--fused_only", action="store_true", help="run the fused path alone (for a kernel trace)")
    args = ap.parse_args()
    shapes = []
    for n in args.sizes:
        for d in args.dims:
            g = torch.Generator(device="cuda").manual_seed(1000 * d + n)
            A = torch.randn(LATENT, d, device="cuda", generator=g) / LATENT ** 0.5
            real, fake = features(n, d, 0.0, 1.0, g, A), features(n, d, 0.25, 0.9, g, A)
            flop = 4 * 2.0 * n * n * d
            got = metrics.manifold_metrics(real, fake, args.k)  # warm-up
            if args.fused_only:
                t, _ = timed(lambda: metrics.manifold_metrics(real, fake, args.k))
                shapes.append({"n": n, "dim": d, "k": args.k, "fused_s": round(t, 5), "fused_tflops": round(flop / t / 1e12, 2), **got})
                continue
            ref = torch_metrics(real, fake, args.k, args.chunk)  # warm-up
            r64, f64 = real.double(), fake.double()
            (r64 @ f64.T).sum().item()
            t_fused, t_torch, t_mm = [], [], []
            for _ in range(args.reps):  # the sides alternate
                t_fused.append(timed(lambda: metrics.manifold_metrics(real, fake, args.k))[0])
                t_torch.append(timed(lambda: torch_metrics(real, fake, args.k, args.chunk))[0])
                t_mm.append(timed(lambda: r64 @ f64.T)[0])
            del r64, f64
            tf, tt, tm = min(t_fused), min(t_torch), min(t_mm)
            s2 = metrics.knn_radii(fake, args.k)
            tp = min(timed(lambda: metrics.feature_knn(real, fake, 0, s2, want=("count", "min2")))[0] for _ in range(args.reps))  # one cross pass
            shapes.append({"n": n, "dim": d, "k": args.k, "fused_s": round(tf, 5), "torch_fp64_s": round(tt, 5), "torch_over_fused": round(tt / tf, 3),
                           "fused_tflops": round(flop / tf / 1e12, 2), "torch_dgemm_tflops": round(flop / 4 / tm / 1e12, 2),
                           "fused_share_of_dgemm_rate": round((flop / tf) / (flop / 4 / tm), 3),
                           "pass_s": round(tp, 5), "pass_tflops": round(flop / 4 / tp / 1e12, 2),
                           "fused_s_all": [round(t, 5) for t in t_fused], "torch_fp64_s_all": [round(t, 5) for t in t_torch],
                           "fused": got, "torch": ref, "metrics_equal": got == ref})
    print(json.dumps({"bench": "prdc", "device": torch.cuda.get_device_name(0), "flop_per_pass": "2 n m dim", "shapes": shapes}))


if __name__ == "__main__":
    main()
