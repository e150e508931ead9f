#!/usr/bin/env python3
"""Times the fused denoising-loss kernel on one GPU and prints one JSON line: r2dm_amd._lib.diffusion_loss (target, criterion, mask and
the float64 sums in one pass, r2dm_diffusion_loss) at 8 x 2 x 64 x 1024 against its torch composition on the same GPU and inputs
(``get_target``, the criterion, the mask product and the two reductions of base.py:133-137), after comparing the outputs.  The pair is
timed in alternating windows; the medians and the spread of the windows are reported, and the fraction of the HBM bound that the
kernel's bytes (prediction, x_0, noise and the mask read once) make of its median.  For the record: the loss moves about 2 MB per
sample next to a 234 GFLOP U-Net call."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from r2dm_amd import _lib, synthetic  # noqa: E402
from r2dm_amd.inference import setup_model  # noqa: E402

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


def compare(hip, composition, windows, reps):
    """Alternating timed windows after a warm-up of each -> (median, min, max) seconds per call of both."""
    hip(), composition()
    th, tt = [], []
    for _ in range(windows):
        th.append(window(hip, reps))
        tt.append(window(composition, reps))
    stats = lambda t: {"median_s": float(f"{statistics.median(t):.4e}"), "min_s": float(f"{min(t):.4e}"), "max_s": float(f"{max(t):.4e}")}
    return stats(th), stats(tt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--objective", default="v", choices=["eps", "v", "x_0"])
    ap.add_argument("--criterion", default="l2", choices=["l2", "l1", "huber"])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    dev, shape = "cuda", (args.batch, 2, 64, 1024)
    # the diffusion class alone (its U-Net is never run here): get_target and the schedule scalars of the composition
    ddpm = setup_model(synthetic.synthetic_checkpoint(seed=0, resolution=(16, 128), prediction_type=args.objective), device=dev, show_info=False)[0]
    gen = torch.Generator(device=dev).manual_seed(0)
    pred, noise = (torch.randn(*shape, generator=gen, device=dev) for _ in range(2))
    x_0 = torch.randn(*shape, generator=gen, device=dev).clamp(-1, 1)
    mask = (torch.rand(args.batch, 1, *shape[2:], generator=gen, device=dev) > 0.3).float()
    steps = torch.linspace(0.05, 0.95, args.batch, device=dev)
    coef = ddpm._loss_coef(steps).to(dev)
    criterion = {"l2": torch.nn.MSELoss(reduction="none"), "l1": torch.nn.L1Loss(reduction="none"),
                 "huber": torch.nn.SmoothL1Loss(reduction="none")}[args.criterion]
    alpha, sigma = coef[:, 0][:, None, None, None], coef[:, 1][:, None, None, None]

    def target():  # get_target with the schedule scalars already on the device, as the fused call has them
        if args.objective == "v":
            return alpha * noise - sigma * x_0
        return noise if args.objective == "eps" else x_0

    hip = lambda: _lib.diffusion_loss(pred, x_0, noise, mask, coef, args.objective, args.criterion)
    composition = lambda: ((criterion(pred, target()) * mask).flatten(1).sum(1), mask.flatten(1).sum(1))
    (num, den), (num_t, den_t) = hip(), composition()
    assert torch.equal(target(), ddpm.get_target(x_0, steps, noise))
    rel = ((num.sum(1) - num_t.double()).abs() / num_t.double().abs()).max().item()
    th, tt = compare(hip, composition, args.windows, args.reps)
    nbytes = 4 * (3 * pred.numel() + mask.numel())
    print(json.dumps({"shape": list(shape), "objective": args.objective, "criterion": args.criterion, "mask_channels": 1, "windows": args.windows,
                      "reps": args.reps, "max_rel_diff_of_sums": float(f"{rel:.3e}"), "den_equal": bool(torch.equal(den, den_t.double())),
                      "hip": th, "torch": tt, "ratio": round(tt["median_s"] / th["median_s"], 1), "bytes": nbytes,
                      "hbm_bound_fraction": round(nbytes / HBM_PEAK / th["median_s"], 3)}))


if __name__ == "__main__":
    main()
