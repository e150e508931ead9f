#!/usr/bin/env python3
"""Times completion on DPM-Solver++(2M) on one GPU and prints one JSON line: ``r2dm_dpm_step_known`` at 8 x 2 x 64 x 1024 against its torch
composition on the same GPU and inputs (the contract's expressions in torch ops), after comparing both outputs with ``torch.equal``, with
every operand (noise and a one-channel mask) and with none of the optional ones but the history, with the bytes it moves and the fraction
of the HBM bound they make of its median; one step of ``complete_dpm`` (a draw, the denoiser call, the fused kernel) against one reverse
sub-step of ``complete`` (a draw, the denoiser call, ``r2dm_posterior_step_known``) at batch 8; and a ``--steps``-step ``complete_dpm`` call
against the ``--complete_steps``-step ``complete`` call at batch 8.  The pairs are timed in alternating windows; the medians and the spread
of the windows are reported.  Every figure is a report: there is no bar.  What it cannot report: the quality of either completion, and how
many steps ``complete_dpm`` needs to match ``complete`` or RePaint, which need a trained checkpoint (``completion_eval.py --methods dpmpp
ddnm repaint``)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_complete import HBM_PEAK, OBJECTIVES, compare  # noqa: E402
from r2dm_amd import _lib, synthetic  # noqa: E402
from r2dm_amd.inference import setup_model, setup_rng  # noqa: E402


def torch_dpm_step_known(x, pr, h, z, y, m, coef, objective, clip):
    a_t, s_t, c_x, c_0, c_1, c_z = (coef[:, k][:, None, None, None] for k in range(6))
    if objective == "eps":
        x0 = (x - s_t * pr) / a_t
    elif objective == "v":
        x0 = a_t * x - s_t * pr
    else:
        x0 = pr
    x0 = x0.clamp(-clip, clip)
    if y is not None:
        x0 = m * y + (1.0 - m) * x0
    x_s = (c_x * x + c_0 * x0) + c_1 * h
    if z is not None:
        x_s = x_s + c_z * z
    return x_s, x0


def bench_kernel(batch, objective, full, windows, reps, ddpm, gen):
    dev, shape = "cuda", (batch, 2, 64, 1024)
    x, pr, z = (torch.randn(*shape, generator=gen, device=dev) for _ in range(3))
    h, y = (torch.tanh(torch.randn(*shape, generator=gen, device=dev)) for _ in range(2))
    m = (torch.rand(batch, 1, 64, 1024, generator=gen, device=dev) < 0.25).float()
    if not full:
        z = y = m = None
    _, table, second = ddpm._dpm_table(batch + 1, 1, 2, "logsnr", 1.0, False, dev, eta=1.0)
    coef = table[1:, 0].contiguous()  # a different second-order row per sample
    assert bool(second[1:].all())
    est = torch.empty_like(x)
    hip = lambda: _lib.dpm_step_known(x, pr, h, z, y, m, coef, OBJECTIVES[objective], 1.0, x0_out=est)
    comp = lambda: torch_dpm_step_known(x, pr, h, z, y, m, coef, objective, 1.0)
    equal = all(bool(torch.equal(a, b)) for a, b in zip(hip(), comp()))
    th, tt = compare(hip, comp, windows, reps)
    # x_t, prediction, x0_prev read, x_s and x0 written; with every operand also noise, known and the one-channel mask
    nbytes = 4 * (7 * x.numel() + m.numel()) if full else 4 * 5 * x.numel()
    return {"bit_equal": equal, "hip": th, "torch": tt, "ratio": round(tt["median_s"] / th["median_s"], 2), "bytes": nbytes,
            "hbm_bound_fraction": round(nbytes / HBM_PEAK / th["median_s"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objective", default="eps", choices=list(OBJECTIVES))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step_reps", type=int, default=10)
    ap.add_argument("--loop_windows", type=int, default=3)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--complete_steps", type=int, default=32)
    args = ap.parse_args()
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(0)
    ddpm = setup_model(synthetic.synthetic_checkpoint(seed=0, prediction_type=args.objective), device=dev, show_info=False, max_batch=8)[0]
    result = {"objective": args.objective, "windows": args.windows, "reps": args.reps,
              "8x2x64x1024": {"noise_and_mask": bench_kernel(8, args.objective, True, args.windows, args.reps, ddpm, gen),
                              "neither": bench_kernel(8, args.objective, False, args.windows, args.reps, ddpm, gen)}}
    # one step of each sampler at batch 8, the draw and the denoiser call included (64 x 1024, the flagship geometry)
    B = 8
    x = torch.randn(B, 2, 64, 1024, generator=gen, device=dev)
    hist, known = (torch.tanh(torch.randn(B, 2, 64, 1024, generator=gen, device=dev)) for _ in range(2))
    mask = torch.zeros(B, 1, 64, 1024, device=dev)
    mask[:, :, ::4] = 1
    rng = setup_rng(range(B), dev)
    t, s = torch.full((B,), 0.5), torch.full((B,), 0.4)
    objective, clip = ddpm._objective_id(), ddpm._clip()
    cond, coef, _ = ddpm._dpm_table(args.steps, B, 2, "logsnr", 1.0, True, dev, eta=1.0)
    mid, est = args.steps // 2, torch.empty_like(x)

    def dpm_one():
        noise = ddpm.randn_like(x, rng=rng)
        return _lib.dpm_step_known(x, ddpm.model(x, cond[mid]), hist, noise, known, mask, coef[mid], objective, clip, x0_out=est)[0]

    def complete_one():
        c, k, mode_id = ddpm._coefficients(t, s, "ddpm", 0.0)
        noise = ddpm.randn_like(x, rng=rng)
        return _lib.posterior_step_known(x, ddpm.model(x, c.to(dev)), noise, known, mask, k.to(dev), mode_id, objective, clip)

    td, tc = compare(dpm_one, complete_one, args.windows, args.step_reps)
    result["step_batch8"] = {"complete_dpm_step": td, "complete_step": tc, "ratio": round(td["median_s"] / tc["median_s"], 3), "reps": args.step_reps}
    # the whole calls
    fast = lambda: ddpm.complete_dpm(known, mask, args.steps, progress=False, rng=rng)
    slow = lambda: ddpm.complete(known, mask, args.complete_steps, progress=False, rng=rng)
    tf, ts = compare(fast, slow, args.loop_windows, 1)
    result["call_batch8"] = {f"complete_dpm_{args.steps}": tf, f"complete_{args.complete_steps}": ts, "ratio": round(ts["median_s"] / tf["median_s"], 2),
                             "windows": args.loop_windows}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
