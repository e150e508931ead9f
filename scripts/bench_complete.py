#!/usr/bin/env python3
"""Times data-consistent completion on one GPU and prints one JSON line: ``r2dm_posterior_step_known`` at 8 x 2 x 64 x 1024 and
32 x 2 x 64 x 1024 against its torch composition on the same GPU and inputs (the contract's expressions in torch ops), after comparing the
outputs with ``torch.equal``, with the bytes it moves and the fraction of the HBM bound they make of its median; one reverse sub-step of
``complete`` (draw, denoiser call, the fused kernel) against one of ``repaint`` (two draws, ``p_step``, ``r2dm_repaint_blend``) at batch 8;
and ``complete(32 steps, 1 resampling)`` against ``repaint(32 steps, 10 resamplings)`` at batch 8.  The pairs are timed in alternating
windows; the medians and the spread of the windows are reported.  Exits non-zero if the fused kernel's median is slower than its torch
composition's; every other figure is a report."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from r2dm_amd import _lib, synthetic  # noqa: E402
from r2dm_amd.inference import setup_model, setup_rng  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, the MI355X's specification
OBJECTIVES = {"eps": 0, "v": 1, "x_0": 2}


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


def compare(first, second, windows, reps):
    """Alternating timed windows after a warm-up of each -> (median, min, max) seconds per call of both."""
    first(), second()
    ta, tb = [], []
    for _ in range(windows):
        ta.append(window(first, reps))
        tb.append(window(second, reps))
    stats = lambda t: {"median_s": float(f"{statistics.median(t):.4e}"), "min_s": float(f"{min(t):.4e}"), "max_s": float(f"{max(t):.4e}")}
    return stats(ta), stats(tb)


def torch_step_known(x, pr, z, y, m, coef, mode, objective, clip):
    a_t, s_t, a_s, _, c, sd, c1, c2 = (coef[:, k][:, None, None, None] for k in range(8))
    if objective == "eps":
        x0 = (x - s_t * pr) / a_t
    elif objective == "v":
        x0 = a_t * x - s_t * pr
    else:
        x0 = pr
    x0 = x0.clamp(-clip, clip)
    x0 = m * y + (1.0 - m) * x0
    if mode == "ddpm":
        return a_s * (x * (1.0 - c) / a_t + c * x0) + sd * z
    return a_s * x0 + c1 * z + c2 * ((x - a_t * x0) / s_t)


def bench_kernel(batch, objective, mode, windows, reps, ddpm, gen):
    dev, shape = "cuda", (batch, 2, 64, 1024)
    x, pr, z = (torch.randn(*shape, generator=gen, device=dev) for _ in range(3))
    y = torch.tanh(torch.randn(*shape, generator=gen, device=dev))
    m = (torch.rand(batch, 1, 64, 1024, generator=gen, device=dev) < 0.25).float()
    _, coef, mode_id = ddpm._coefficients(torch.linspace(1.0, 0.1, batch), torch.linspace(0.9, 0.0, batch), mode, 0.5)
    coef = coef.to(dev)
    hip = lambda: _lib.posterior_step_known(x, pr, z, y, m, coef, mode_id, OBJECTIVES[objective], 1.0)
    comp = lambda: torch_step_known(x, pr, z, y, m, coef, mode, objective, 1.0)
    equal = bool(torch.equal(hip(), comp()))
    th, tt = compare(hip, comp, windows, reps)
    nbytes = 4 * (5 * x.numel() + m.numel())  # x_t, prediction, noise, known read, x_s written, the one-channel mask read
    return {"bit_equal": equal, "hip": th, "torch": tt, "ratio": round(tt["median_s"] / th["median_s"], 2), "bytes": nbytes,
            "hbm_bound_fraction": round(nbytes / HBM_PEAK / th["median_s"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objective", default="eps", choices=list(OBJECTIVES))
    ap.add_argument("--mode", default="ddpm", choices=["ddpm", "ddim"])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step_reps", type=int, default=10)
    ap.add_argument("--loop_windows", type=int, default=3)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--repaint_resample_steps", type=int, default=10)
    args = ap.parse_args()
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(0)
    ddpm = setup_model(synthetic.synthetic_checkpoint(seed=0, prediction_type=args.objective), device=dev, show_info=False, max_batch=8)[0]
    result = {"objective": args.objective, "mode": args.mode, "windows": args.windows, "reps": args.reps}
    for batch in (8, 32):
        result[f"{batch}x2x64x1024"] = {"posterior_step_known": bench_kernel(batch, args.objective, args.mode, args.windows, args.reps, ddpm, gen)}
    # one reverse sub-step of each sampler at batch 8, the denoiser call included (64 x 1024, the flagship geometry), as its loop runs it
    B = 8
    x = torch.randn(B, 2, 64, 1024, generator=gen, device=dev)
    known = torch.tanh(torch.randn(B, 2, 64, 1024, generator=gen, device=dev))
    mask = torch.zeros(B, 1, 64, 1024, device=dev)
    mask[:, :, ::4] = 1
    rng = setup_rng(range(B), dev)
    t, s = torch.full((B,), 0.5), torch.full((B,), 0.4)
    objective, clip = ddpm._objective_id(), ddpm._clip()

    def complete_step():
        cond, coef, mode_id = ddpm._coefficients(t, s, "ddpm", 0.0)
        noise = ddpm.randn_like(x, rng=rng)
        return _lib.posterior_step_known(x, ddpm.model(x, cond.to(dev)), noise, known, mask, coef.to(dev), mode_id, objective, clip)

    def repaint_step():
        noise_k = ddpm.randn_like(known, rng=rng)
        unknown = ddpm.p_step(x, t, s, rng=rng)
        return _lib.repaint_blend(known, noise_k, unknown, mask, ddpm._alpha_sigma_rows(s).to(dev))

    tc, tr = compare(complete_step, repaint_step, args.windows, args.step_reps)
    result["step_batch8"] = {"complete_step": tc, "repaint_step": tr, "ratio": round(tc["median_s"] / tr["median_s"], 3), "reps": args.step_reps}
    # the whole loops, at the defaults of completion_eval.py for RePaint
    full = lambda: ddpm.complete(known, mask, args.steps, progress=False, rng=rng)
    rp = lambda: ddpm.repaint(known, mask, args.steps, args.repaint_resample_steps, progress=False, rng=rng)
    tc, tr = compare(full, rp, args.loop_windows, 1)
    result["loop_batch8"] = {"steps": args.steps, "complete_r1": tc, f"repaint_r{args.repaint_resample_steps}": tr,
                             "ratio": round(tr["median_s"] / tc["median_s"], 2), "windows": args.loop_windows}
    print(json.dumps(result))
    slow = [k for k in ("8x2x64x1024", "32x2x64x1024") if result[k]["posterior_step_known"]["hip"]["median_s"] > result[k]["posterior_step_known"]["torch"]["median_s"]]
    if slow:
        raise SystemExit(f"the fused kernel is slower than its torch composition at {slow}")


if __name__ == "__main__":
    main()
