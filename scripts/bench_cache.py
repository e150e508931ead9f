#!/usr/bin/env python3
"""Times the feature cache (DeepCache: ``EfficientUNet.forward_cached``) on one GPU at 64 x 1024, batch 8, and prints one JSON line: milliseconds per
full step (the store forward) and per shallow step at depth 1 / 2 / 3 in the ``fp32`` and ``fp16`` precisions, each step as its loop runs it (denoiser
call, a draw, the posterior update); milliseconds of the store kernel (``r2dm_cache_store``) on the depth-1 tensor of both storage formats with the bytes it
moves and their share of the HBM bound; and images per second of a 256-step ``sample`` call and a 20-step ``sample_dpm`` call at cache intervals 1, 2, 3
and 5 (depth 1).  Every group is timed in alternating windows; medians and the windows' spread are reported.  ``--plain_windows N`` adds N more windows
of the plain 256-step ``sample`` call alone (the series to compare with another build's).  Every figure is a report: what the cache costs in sample
quality needs a trained checkpoint (``generate.py --cache_interval 2 --cache_drift`` prints the drift table to start from)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_complete import HBM_PEAK, window  # noqa: E402
from r2dm_amd import _lib, synthetic  # noqa: E402
from r2dm_amd.inference import setup_model, setup_rng  # noqa: E402


def stats(t):
    return {"median_s": float(f"{statistics.median(t):.4e}"), "min_s": float(f"{min(t):.4e}"), "max_s": float(f"{max(t):.4e}")}


def alternate(fns: dict, windows: int, reps: int):
    """every function warmed up once, then ``windows`` rounds over all of them in turn -> {name: stats}"""
    for fn in fns.values():
        fn()
    times = {name: [] for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            times[name].append(window(fn, reps))
    return {name: stats(t) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--step_reps", type=int, default=10)
    ap.add_argument("--kernel_reps", type=int, default=50)
    ap.add_argument("--loop_windows", type=int, default=3)
    ap.add_argument("--sample_steps", type=int, default=256)
    ap.add_argument("--dpm_steps", type=int, default=20)
    ap.add_argument("--plain_windows", type=int, default=0)
    ap.add_argument("--skip_loops", action="store_true")
    args = ap.parse_args()
    dev, B = "cuda", 8
    gen = torch.Generator(device=dev).manual_seed(0)
    ddpm = setup_model(synthetic.synthetic_checkpoint(seed=0), device=dev, show_info=False, max_batch=B)[0]
    net = ddpm.model
    x = torch.randn(B, 2, 64, 1024, generator=gen, device=dev)
    rng = setup_rng(range(B), dev)
    row, mode_id = ddpm._table_rows(args.sample_steps, B, "ddpm", 0.0, torch.device(dev))
    cond, coef = row(args.sample_steps // 2)
    result = {"batch": B, "resolution": [64, 1024], "windows": args.windows, "step_reps": args.step_reps}

    def step(call):  # one sampler step around a denoiser call, as _run_loop runs it
        noise, drawn = ddpm._randn_like_ahead(x, rng=rng)
        pred = call()
        if drawn is not None:
            torch.cuda.current_stream().wait_event(drawn)
        return ddpm._posterior(x, pred, noise, coef, mode_id)

    for precision in ("fp32", "fp16"):
        net.set_precision(precision)
        with net.deferred_range_check():
            caches = {d: net.new_cache(B, d) for d in (1, 2, 3)}
            drifting = net.new_cache(B, 1, drift=True)
            fns = {"plain": lambda: step(lambda: net(x, cond)), "full_depth1": lambda: step(lambda: net.forward_cached(x, cond, caches[1], refresh=True)),
                   "full_depth1_drift": lambda: step(lambda: net.forward_cached(x, cond, drifting, refresh=True))}
            for d in (1, 2, 3):
                net.forward_cached(x, cond, caches[d], refresh=True)
                fns[f"shallow_depth{d}"] = (lambda d: lambda: step(lambda: net.forward_cached(x, cond, caches[d], refresh=False)))(d)
            t = alternate(fns, args.windows, args.step_reps)
            drifting._drift.clear()
        result[f"step_ms_{precision}"] = {k: {"median": round(1e3 * v["median_s"], 4), "min": round(1e3 * v["min_s"], 4), "max": round(1e3 * v["max_s"], 4)} for k, v in t.items()}
    net.set_precision("fp32")

    # the store kernel on the depth-1 tensor (B, 64, 64, 1024): 2 reads + 1 write per value
    n = 64 * 64 * 1024
    partial, sums = torch.empty(B * 512 * 2, dtype=torch.float64, device=dev), torch.empty(B, 2, dtype=torch.float64, device=dev)
    kernel = {}
    for name, dtype in (("fp32", torch.float32), ("fp16", torch.float16)):
        fresh, cached = (torch.randn(B, n, generator=gen, device=dev).to(dtype) for _ in range(2))
        call = lambda: _lib.check(_lib.lib().r2dm_cache_store(fresh.data_ptr(), cached.data_ptr(), B, n, int(dtype == torch.float16), partial.data_ptr(),
                                                              sums.data_ptr(), _lib.stream_ptr(torch.device(dev))))
        call()
        t = stats([window(call, args.kernel_reps) for _ in range(args.windows)])
        nbytes = 3 * B * n * fresh.element_size()
        kernel[name] = {"ms": round(1e3 * t["median_s"], 4), "min_ms": round(1e3 * t["min_s"], 4), "max_ms": round(1e3 * t["max_s"], 4), "bytes": nbytes,
                        "hbm_bound_fraction": round(nbytes / HBM_PEAK / t["median_s"], 3)}
    result["cache_store_depth1"] = kernel

    if not args.skip_loops:
        intervals = (1, 2, 3, 5)
        loops = {f"sample_{args.sample_steps}_interval{k}": (lambda k: lambda: ddpm.sample(B, args.sample_steps, progress=False, rng=rng, cache_interval=k))(k) for k in intervals}
        loops.update({f"sample_dpm_{args.dpm_steps}_interval{k}": (lambda k: lambda: ddpm.sample_dpm(B, args.dpm_steps, progress=False, rng=rng, cache_interval=k))(k)
                      for k in intervals})
        t = alternate(loops, args.loop_windows, 1)
        result["calls"] = {name: {**v, "images_per_s": round(B / v["median_s"], 2)} for name, v in t.items()}
        for kind in (f"sample_{args.sample_steps}", f"sample_dpm_{args.dpm_steps}"):
            base = t[f"{kind}_interval1"]["median_s"]
            result[f"speedup_{kind}"] = {f"interval{k}": round(base / t[f"{kind}_interval{k}"]["median_s"], 3) for k in intervals}
    if args.plain_windows:
        plain = lambda: ddpm.sample(B, args.sample_steps, progress=False, rng=rng)
        plain()
        series = [window(plain, 1) for _ in range(args.plain_windows)]
        result["plain_sample_series_s"] = [float(f"{s:.4e}") for s in series]
        result["plain_sample_images_per_s"] = round(B / statistics.median(series), 2)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
