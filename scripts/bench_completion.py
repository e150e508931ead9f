#!/usr/bin/env python3
"""Times the three completion-metric kernels on one GPU and prints one JSON line: r2dm_completion_error, r2dm_confusion_matrix and
r2dm_fill_beams (r2dm_amd.completion) at batch 8, 64 x 1024, each against its torch composition on the same GPU and inputs, after
comparing the outputs.

  - errors: the four counts and six sums per sample from boolean masks, ``torch.where`` and float64 reductions over the five planes;
  - confusion: ``torch.bincount`` of ``target * C + pred`` over the masked pixels, per sample (its size argument costs a device read);
  - fill (linear, ``beams:4``): per-row up / down indices from ``cummax`` / ``cummin``, two gathers per channel and ``torch.where``.

Every pair is timed in alternating windows with HIP events; the medians and the spread of the windows are reported, and for the two
streaming kernels the fraction of the HBM bound that their bytes make of the median."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from r2dm_amd import completion  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, the MI355X's specification
LO, HI = 1.45, 80.0


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


def compare(hip, composition, windows, reps):
    """Alternating timed windows after a warm-up of each -> (median, min, max) seconds per call of both."""
    hip(), composition()
    th, tt = [], []
    for _ in range(windows):
        th.append(window(hip, reps))
        tt.append(window(composition, reps))
    stats = lambda t: {"median_s": float(f"{statistics.median(t):.4e}"), "min_s": float(f"{min(t):.4e}"), "max_s": float(f"{max(t):.4e}")}
    return stats(th), stats(tt)


def torch_errors(pred, target, known):
    r, rp = target[:, 0].flatten(1), pred[:, 0].flatten(1)
    U = known[:, 0].flatten(1) == 0
    G, P = (r > LO) & (r < HI), (rp > LO) & (rp < HI)
    E, Bo = U & G, U & G & P
    zero = torch.zeros((), dtype=torch.float64, device=pred.device)
    d = torch.where(P, rp, torch.zeros_like(rp)).double() - r.double()
    e = pred[:, 4].flatten(1).double() - target[:, 4].flatten(1).double()
    on = lambda m, v: torch.where(m, v, zero).sum(1)
    return torch.stack([U.sum(1).double(), E.sum(1).double(), Bo.sum(1).double(), (U & P & ~G).sum(1).double(), on(E, d.abs()), on(E, d * d),
                        on(Bo, d.abs()), on(Bo, d * d), on(E, e.abs()), on(E, e * e)], 1)


def torch_confusion(pred, target, C, mask):
    out = []
    for b in range(pred.shape[0]):
        keep = mask[b] != 0
        out.append(torch.bincount(target[b][keep] * C + pred[b][keep], minlength=C * C).reshape(C, C))
    return torch.stack(out)


def torch_fill_linear(x, rows, nodata=-1.0):
    B, C, H, W = x.shape
    h = torch.arange(H, device=x.device)[None].expand(B, H)
    known = rows != 0
    up = torch.where(known, h, torch.full_like(h, -1)).cummax(1).values            # nearest known row at or above
    dn = torch.where(known, h, torch.full_like(h, H)).flip(1).cummin(1).values.flip(1)  # ... at or below
    iu, id_ = up.clamp(min=0)[:, None, :, None].expand(B, C, H, W), dn.clamp(max=H - 1)[:, None, :, None].expand(B, C, H, W)
    a, e = x.gather(2, iu), x.gather(2, id_)
    ua = (up >= 0)[:, None, :, None] & (a[:, :1] != nodata)
    ub = (dn < H)[:, None, :, None] & (e[:, :1] != nodata)
    t = ((h - up).float() / (dn - up).clamp(min=1).float())[:, None, :, None]
    out = torch.where(ua & ub, a + (e - a) * t, torch.where(ua, a, torch.where(ub, e, torch.full_like(a, nodata))))
    return torch.where(known[:, None, :, None], x, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=100)
    args = ap.parse_args()
    dev, B, H, W, C = "cuda", args.batch, 64, 1024, args.classes
    gen = torch.Generator(device=dev).manual_seed(0)
    target = torch.rand(B, 5, H, W, generator=gen, device=dev)
    target[:, 0] = 0.5 + 89.5 * target[:, 0]
    pred = target + 0.3 * torch.randn(B, 5, H, W, generator=gen, device=dev)
    known = completion.corruption_mask("beams:4", H, W).to(dev)[None].expand(B, 1, H, W).contiguous()
    result = {"shape": [B, H, W], "classes": C, "windows": args.windows, "reps": args.reps}

    hip = lambda: completion.completion_error_sums(pred, target, known, LO, HI)
    comp = lambda: torch_errors(pred, target, known)
    got, want = hip(), comp()
    rel = ((got - want).abs() / want.abs().clamp(min=1e-300)).max().item()
    th, tt = compare(hip, comp, args.windows, args.reps)
    nbytes = 4 * B * H * W * 5  # two planes of pred, two of target, the mask
    result["errors"] = {"counts_equal": bool(torch.equal(got[:, :4], want[:, :4])), "max_rel_diff_of_sums": float(f"{rel:.3e}"), "hip": th, "torch": tt,
                        "ratio": round(tt["median_s"] / th["median_s"], 1), "bytes": nbytes,
                        "hbm_bound_fraction": round(nbytes / HBM_PEAK / th["median_s"], 3)}

    lp, lt = (torch.randint(0, C, (B, H * W), generator=gen, device=dev) for _ in range(2))
    measured = (target[:, 0].flatten(1) > LO).float() * (target[:, 0].flatten(1) < HI).float()
    hip = lambda: completion.confusion_matrix(lp, lt, C, measured)
    comp = lambda: torch_confusion(lp, lt, C, measured)
    equal = bool(torch.equal(hip(), comp()))
    th, tt = compare(hip, comp, args.windows, args.reps)
    nbytes = B * H * W * (8 + 8 + 4)
    result["confusion"] = {"equal": equal, "hip": th, "torch": tt, "ratio": round(tt["median_s"] / th["median_s"], 1), "bytes": nbytes,
                           "hbm_bound_fraction": round(nbytes / HBM_PEAK / th["median_s"], 3)}

    x = torch.randn(B, 2, H, W, generator=gen, device=dev)
    x[:, 0] = torch.where(torch.rand(B, H, W, generator=gen, device=dev) < 0.2, torch.full_like(x[:, 0], -1.0), x[:, 0].abs())
    rows = completion.rows_of_mask(known)
    hip = lambda: completion.fill_beams(x, rows, "linear")
    comp = lambda: torch_fill_linear(x, rows)
    diff = (hip() - comp()).abs().max().item()  # (the composition's float32 expression may be evaluated with other roundings)
    th, tt = compare(hip, comp, args.windows, args.reps)
    nbytes = 4 * 2 * x.numel()
    result["fill_linear"] = {"max_abs_diff": float(f"{diff:.3e}"), "hip": th, "torch": tt, "ratio": round(tt["median_s"] / th["median_s"], 1),
                             "bytes": nbytes, "hbm_bound_fraction": round(nbytes / HBM_PEAK / th["median_s"], 3)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
