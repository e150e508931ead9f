#!/usr/bin/env python3
"""Times the DPM-Solver++(2M) sampler on one GPU and prints one JSON line: ``r2dm_dpm_step`` at 8 x 2 x 64 x 1024 and 32 x 2 x 64 x 1024
against its torch composition on the same GPU and inputs (the contract's expressions in torch ops), after comparing both outputs with
``torch.equal``, with the bytes it moves and the fraction of the HBM bound they make of its median; one step of ``sample_dpm`` (denoiser
call, the fused kernel) against one ``p_step`` (denoiser call, a draw, ``r2dm_posterior_step``) at batch 8; and a ``--steps``-step
``sample_dpm`` call against the 256-step ancestral ``sample`` call (unchanged by this sampler) at batch 8, as images per second.  The pairs
are timed in alternating windows; the medians and the spread of the windows are reported.  Exits non-zero if the fused kernel's median is
slower than its torch composition's; every other figure is a report.  What it cannot report: sample quality at 20 steps, which needs a
trained checkpoint (``evaluate.py`` on the output of ``sample_and_save.py --mode dpmpp``)."""
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


def torch_dpm_step(x, pr, h, coef, objective, clip):
    a_t, s_t, c_x, c_0, c_1 = (coef[:, k][:, None, None, None] for k in range(5))
    if objective == "eps":
        x0 = (x - s_t * pr) / a_t
    elif objective == "v":
        x0 = a_t * x - s_t * pr
    else:
        x0 = pr
    x0 = x0.clamp(-clip, clip)
    return (c_x * x + c_0 * x0) + c_1 * h, x0


def bench_kernel(batch, objective, windows, reps, ddpm, gen):
    dev, shape = "cuda", (batch, 2, 64, 1024)
    x, pr = (torch.randn(*shape, generator=gen, device=dev) for _ in range(2))
    h = torch.tanh(torch.randn(*shape, generator=gen, device=dev))
    _, table, second = ddpm._dpm_table(batch + 1, 1, 2, "logsnr", 1.0, False, dev)
    coef = table[1:, 0].contiguous()  # a different second-order row per sample
    assert bool(second[1:].all())
    est = torch.empty_like(x)
    hip = lambda: _lib.dpm_step(x, pr, h, coef, OBJECTIVES[objective], 1.0, x0_out=est)
    comp = lambda: torch_dpm_step(x, pr, h, coef, objective, 1.0)
    equal = all(bool(torch.equal(a, b)) for a, b in zip(hip(), comp()))
    th, tt = compare(hip, comp, windows, reps)
    nbytes = 4 * 5 * x.numel()  # x_t, prediction, x0_prev read; x_s, x0 written
    return {"bit_equal": equal, "hip": th, "torch": tt, "ratio": round(tt["median_s"] / th["median_s"], 2), "bytes": nbytes,
            "hbm_bound_fraction": round(nbytes / HBM_PEAK / th["median_s"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objective", default="eps", choices=list(OBJECTIVES))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step_reps", type=int, default=10)
    ap.add_argument("--loop_windows", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sample_steps", type=int, default=256)
    args = ap.parse_args()
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(0)
    ddpm = setup_model(synthetic.synthetic_checkpoint(seed=0, prediction_type=args.objective), device=dev, show_info=False, max_batch=8)[0]
    result = {"objective": args.objective, "windows": args.windows, "reps": args.reps}
    for batch in (8, 32):
        result[f"{batch}x2x64x1024"] = {"dpm_step": bench_kernel(batch, args.objective, args.windows, args.reps, ddpm, gen)}
    # one step of each sampler at batch 8, the denoiser call included (64 x 1024, the flagship geometry), as its loop runs it
    B = 8
    x = torch.randn(B, 2, 64, 1024, generator=gen, device=dev)
    hist = torch.tanh(torch.randn(B, 2, 64, 1024, generator=gen, device=dev))
    rng = setup_rng(range(B), dev)
    t, s = torch.full((B,), 0.5), torch.full((B,), 0.4)
    objective, clip = ddpm._objective_id(), ddpm._clip()
    cond, coef, _ = ddpm._dpm_table(args.steps, B, 2, "logsnr", 1.0, True, dev)
    mid, est = args.steps // 2, torch.empty_like(x)
    dpm_one = lambda: _lib.dpm_step(x, ddpm.model(x, cond[mid]), hist, coef[mid], objective, clip, x0_out=est)[0]
    p_one = lambda: ddpm.p_step(x, t, s, rng=rng)
    td, tp = compare(dpm_one, p_one, args.windows, args.step_reps)
    result["step_batch8"] = {"dpm_step": td, "p_step": tp, "ratio": round(td["median_s"] / tp["median_s"], 3), "reps": args.step_reps}
    # the whole calls
    fast = lambda: ddpm.sample_dpm(B, args.steps, progress=False, rng=rng)
    slow = lambda: ddpm.sample(B, args.sample_steps, progress=False, rng=rng)
    tf, ts = compare(fast, slow, args.loop_windows, 1)
    result["call_batch8"] = {f"sample_dpm_{args.steps}": tf, f"sample_ddpm_{args.sample_steps}": ts,
                             "images_per_s": {f"sample_dpm_{args.steps}": round(B / tf["median_s"], 2), f"sample_ddpm_{args.sample_steps}": round(B / ts["median_s"], 2)},
                             "ratio": round(ts["median_s"] / tf["median_s"], 2), "windows": args.loop_windows}
    print(json.dumps(result))
    lag = [k for k in ("8x2x64x1024", "32x2x64x1024") if result[k]["dpm_step"]["hip"]["median_s"] > result[k]["dpm_step"]["torch"]["median_s"]]
    if lag:
        raise SystemExit(f"the fused kernel is slower than its torch composition at {lag}")


if __name__ == "__main__":
    main()
