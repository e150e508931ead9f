#!/usr/bin/env python3
"""Times r2dm_ensemble_score (r2dm_amd.completion.ensemble_score_sums) on one GPU and prints one JSON line: K = 16 members, batch 8,
64 x 1024, with and without the per-pixel maps, each against its torch composition on the same GPU and inputs, after comparing the outputs.

The composition is what one would write without the kernel, float64 where the kernel is: a sort over the member axis for the sums in
sorted order, the K x K tensor of pairwise |differences| for the pair terms, boolean masks and ``torch.where`` reductions for the thirteen
sums and the per-member sums, a ``bincount`` per scan for the rank histogram and, for the maps, a second sort with the dropped members
pushed to the end, gathers for the median and masked reductions for mean, std, min and max.

Every pair is timed in alternating windows with HIP events (scripts/bench_completion.py's scheme); the medians and the spread of the windows
are reported, the bytes the kernel has to move ((2 K + 3) floats in per pixel, 8 floats out with the maps), those bytes over the median
time, and that as a fraction of the HBM specification."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_completion import HBM_PEAK, HI, LO, compare  # noqa: E402
from r2dm_amd import completion  # noqa: E402


def torch_ensemble(samples, target, known, maps):
    B, K = samples.shape[:2]
    d, rho = samples[:, :, 0].flatten(2), samples[:, :, 4].flatten(2)
    r, rt = target[:, 0].flatten(1), target[:, 4].flatten(1).double()
    U = known[:, 0].flatten(1) == 0
    G = (r > LO) & (r < HI)
    E = U & G
    ret = (d > LO) & (d < HI)
    n = ret.sum(1)
    p = n.double() / K
    rhat = torch.where(ret, d, torch.zeros_like(d)).double()
    rho = torch.nan_to_num(rho, nan=0.0, posinf=float("inf"), neginf=-float("inf")).double()
    r64 = r.double()
    zero = torch.zeros((), dtype=torch.float64, device=samples.device)
    on = lambda m, v: torch.where(m, v, zero).sum(-1)
    raw = [U.sum(1).double(), E.sum(1).double()]
    member, means, sss = [], [], []
    for x, t in ((rhat, r64), (rho, rt)):
        s = x.sort(dim=1).values
        mean = s.sum(1) / K
        ss = (s - mean[:, None]).square().sum(1)
        pair = (x[:, :, None] - x[:, None, :]).abs().sum((1, 2)) / 2
        raw += [on(E, (s - t[:, None]).abs().sum(1)), on(E, pair), on(E, (mean - t).square()), on(E, ss / (K - 1)) if K > 1 else zero.expand(B)]
        member.append(on(E[:, None], (x - t[:, None]).abs()))
        means.append(mean), sss.append(ss)
    raw += [on(U, (p - G.double()).square()), on(E, p), on(U & ~G, p)]
    below = (rhat < r64[:, None]).sum(1)
    rank = torch.stack([torch.bincount(below[b][E[b]], minlength=K + 1) for b in range(B)])
    out = None
    if maps:
        v = torch.where(ret, d, torch.full_like(d, float("inf"))).double().sort(dim=1).values
        some = n > 0
        cnt = n.clamp(min=1).double()
        dm = torch.where(ret, d.double(), zero).sum(1) / cnt
        dev = torch.where(ret, (d.double() - dm[:, None]).square(), zero).sum(1)
        lo_i, hi_i = ((n - 1).clamp(min=0) // 2)[:, None], (n // 2).clamp(max=K - 1)[:, None]
        med = (v.gather(1, lo_i) + v.gather(1, hi_i))[:, 0] * 0.5
        mx = torch.where(ret, d, torch.full_like(d, -float("inf"))).max(1).values.double()
        pick = lambda a: torch.where(some, a, zero)
        out = torch.stack([p, pick(dm), torch.where(n > 1, (dev / cnt).sqrt(), zero), pick(med), pick(v[:, 0]), pick(mx), means[1],
                           (sss[1] / K).sqrt()], 1).float().reshape(B, 8, *samples.shape[-2:])
    return torch.stack(raw, 1), torch.stack(member, 1), rank, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev, B, K, H, W = "cuda", args.batch, args.members, 64, 1024
    gen = torch.Generator(device=dev).manual_seed(0)
    target = torch.rand(B, 5, H, W, generator=gen, device=dev)
    target[:, 0] = 0.5 + 89.5 * target[:, 0]
    samples = target[:, None] + 0.3 * torch.randn(B, K, 5, H, W, generator=gen, device=dev)
    samples[:, :, 0] = torch.where(torch.rand(B, K, H, W, generator=gen, device=dev) < 0.2, torch.zeros_like(samples[:, :, 0]), samples[:, :, 0])
    known = completion.corruption_mask("beams:4", H, W).to(dev)[None].expand(B, 1, H, W).contiguous()
    result = {"shape": [B, K, H, W], "windows": args.windows, "reps": args.reps}
    for name, maps in (("with_maps", True), ("without_maps", False)):
        hip = lambda: completion.ensemble_score_sums(samples, target, known, LO, HI, maps=maps)
        comp = lambda: torch_ensemble(samples, target, known, maps)
        got, want = hip(), comp()
        rel = lambda a, b: float(f"{((a - b).abs() / b.abs().clamp(min=1e-300)).max().item():.3e}")
        entry = {"counts_equal": bool(torch.equal(got[0][:, :2], want[0][:, :2])), "rank_equal": bool(torch.equal(got[2], want[2])),
                 "max_rel_diff_of_sums": rel(got[0][:, 2:], want[0][:, 2:]), "max_rel_diff_of_member_sums": rel(got[1], want[1])}
        if maps:
            entry["max_abs_diff_of_maps"] = float(f"{(got[3] - want[3]).abs().max().item():.3e}")
        del got, want
        th, tt = compare(hip, comp, args.windows, args.reps)
        nbytes = 4 * B * H * W * (2 * K + 3 + (8 if maps else 0))
        entry.update(hip=th, torch=tt, ratio=round(tt["median_s"] / th["median_s"], 1), bytes=nbytes,
                     bytes_per_s=float(f"{nbytes / th['median_s']:.4e}"), hbm_bound_fraction=round(nbytes / HBM_PEAK / th["median_s"], 3))
        result[name] = entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
