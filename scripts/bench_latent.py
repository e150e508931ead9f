#!/usr/bin/env python3
"""Times the two latent-space kernels on one GPU and prints one JSON line: ``r2dm_ddim_transfer`` and ``r2dm_slerp`` (K = 8 weights) at
8 x 2 x 64 x 1024 and 32 x 2 x 64 x 1024 against their torch compositions on the same GPU and inputs (the contract's expressions in
torch ops; for the slerp three float64 reductions, the coefficient arithmetic and a broadcast blend), after comparing the outputs; and
one ``invert`` step against one ``p_step`` at batch 8, each with its denoiser call.  The pairs are timed in alternating windows; the
medians and the spread of the windows are reported, and the fraction of the HBM bound that each kernel's bytes make of its median."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from r2dm_amd import latent, synthetic  # noqa: E402
from r2dm_amd.inference import setup_model, setup_rng  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, the MI355X's specification
K = 8


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


def torch_transfer(x, pr, coef, objective):
    a_t, s_t, a_u, s_u = (coef[:, k][:, None, None, None] for k in range(4))
    if objective == "eps":
        e, x0 = pr, (x - s_t * pr) / a_t
    elif objective == "v":
        x0, e = a_t * x - s_t * pr, s_t * x + a_t * pr
    else:
        x0, e = pr, (x - a_t * pr) / s_t
    return a_u * x0 + s_u * e


def torch_slerp(a, b, w):
    """the same result from torch ops: float64 sums of the float32 products, the coefficients in float64, the blend in float32"""
    fa, fb = a.flatten(1), b.flatten(1)
    ab, aa, bb = ((p.double()).sum(1) for p in (fa * fb, fa * fa, fb * fb))
    cos = (ab / (aa * bb).sqrt()).clamp(-1, 1)
    omega = cos.acos()
    lerp = (1 - cos * cos < 1e-10) | (aa == 0) | (bb == 0)
    so = omega.sin()
    c_a = torch.where(lerp, 1 - w[:, None], ((1 - w[:, None]) * omega).sin() / so)
    c_b = torch.where(lerp, w[:, None].expand_as(c_a), (w[:, None] * omega).sin() / so)
    v = lambda c: c.float()[:, :, None, None, None]
    return v(c_a) * a[None] + v(c_b) * b[None], torch.stack([c_a, c_b], dim=-1)


def bench_shape(batch, objective, windows, reps, ddpm, gen):
    dev, shape = "cuda", (batch, 2, 64, 1024)
    x, pr, b2 = (torch.randn(*shape, generator=gen, device=dev) for _ in range(3))
    rows_t, rows_u = ddpm._alpha_sigma_rows(torch.linspace(0.0, 0.9, batch)), ddpm._alpha_sigma_rows(torch.linspace(0.1, 1.0, batch))
    coef = torch.cat([rows_t, rows_u], dim=-1).to(dev)
    hip, comp = (lambda: latent.ddim_transfer(x, pr, coef, objective)), (lambda: torch_transfer(x, pr, coef, objective))
    equal = bool(torch.equal(hip(), comp()))
    th, tt = compare(hip, comp, windows, reps)
    nbytes = 4 * 3 * x.numel()
    out = {"ddim_transfer": {"bit_equal": equal, "hip": th, "torch": tt, "ratio": round(tt["median_s"] / th["median_s"], 2), "bytes": nbytes,
                             "hbm_bound_fraction": round(nbytes / HBM_PEAK / th["median_s"], 3)}}
    weights = torch.linspace(0.0, 1.0, K).tolist()
    w64 = torch.tensor(weights, dtype=torch.float32, device=dev).double()
    hip, comp = (lambda: latent.slerp(x, b2, weights)), (lambda: torch_slerp(x, b2, w64)[0])
    got, coef64 = latent.slerp(x, b2, weights, return_coefficients=True)
    want, coef_t = torch_slerp(x, b2, w64)
    th, tt = compare(hip, comp, windows, reps)
    nbytes = 4 * (2 * 2 + K) * x.numel()  # a and b read by both launches, K outputs written
    out["slerp"] = {"K": K, "max_abs_diff": float(f"{(got - want).abs().max().item():.3e}"),
                    "max_coef_diff": float(f"{(coef64 - coef_t).abs().max().item():.3e}"), "hip": th, "torch": tt,
                    "ratio": round(tt["median_s"] / th["median_s"], 2), "bytes": nbytes, "hbm_bound_fraction": round(nbytes / HBM_PEAK / th["median_s"], 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objective", default="eps", choices=["eps", "v", "x_0"])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step_reps", type=int, default=10)
    args = ap.parse_args()
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(0)
    ddpm = setup_model(synthetic.synthetic_checkpoint(seed=0, prediction_type=args.objective), device=dev, show_info=False, max_batch=8)[0]
    result = {"objective": args.objective, "windows": args.windows, "reps": args.reps}
    for batch in (8, 32):
        result[f"{batch}x2x64x1024"] = bench_shape(batch, args.objective, args.windows, args.reps, ddpm, gen)
    # one inversion step against one reverse step at batch 8, the denoiser call included (64 x 1024, the flagship geometry)
    x = torch.randn(8, 2, 64, 1024, generator=gen, device=dev).clamp(-1, 1)
    rng = setup_rng(range(8), dev)
    t, s = torch.full((8,), 0.5), torch.full((8,), 0.4)
    inv = lambda: ddpm.invert(x, 1, t_end=0.1, progress=False)
    rev = lambda: ddpm.p_step(x, t, s, rng=rng, mode="ddim")
    ti, tp = compare(inv, rev, args.windows, args.step_reps)
    result["step_batch8"] = {"invert_step": ti, "p_step_ddim": tp, "ratio": round(ti["median_s"] / tp["median_s"], 3), "reps": args.step_reps}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
