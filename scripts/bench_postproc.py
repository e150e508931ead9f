#!/usr/bin/env python3
"""Times the two post-processors of the segmentation on one GPU and prints one JSON line.  Workload: --batch images of 64 x 1024; the kNN
vote at 3 x 3 / k 3 and at 5 x 5 / k 5, the CRF-RNN at 20 classes x 3 iterations (theta_beta 0.5, so that the appearance term is alive).
For each:
  - the kernel alone: the C entry point on preallocated buffers between device events;
  - the public call (r2dm_amd.postproc.KNN / CRFRNN), allocations and the flag read included;
  - the yardstick: the torch composition of tests/postproc_oracle.py in fp32 on the same device and inputs, --chunk images at a time -- the
    test oracle, not the code under test --, held to the same results first (kNN: equal labels on every pixel; CRF: the largest difference);
  - after a warm-up the three are timed in alternating windows, --reps times: median, min and max; images/s, the ratio to the yardstick,
    and the achieved bytes/s of the kernel against its algorithmic traffic (kNN: 20 B per pixel -- depth, label in, label out; CRF: per
    iteration (2 N + 4) 4 B per pixel -- Q in and out, xyz, mask; the unary, the halo and the second read of Q are extra)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import make_golden_postproc as G  # noqa: E402  (the scenes of the tests)
import postproc_oracle as O  # noqa: E402
from r2dm_amd import _lib, postproc  # noqa: E402


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3


def alternate(fns, reps):
    """every function once per round, ``reps`` rounds: {name: seconds}"""
    for fn in fns.values():
        fn()  # warm-up
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(window(fn))
    return times


def summary(times):
    return {"median_s": round(statistics.median(times), 6), "min_s": round(min(times), 6), "max_s": round(max(times), 6)}


def tiled(a, B):
    """(B, ...) from the first images of ``a``, repeated"""
    t = torch.from_numpy(a)
    return t.repeat(-(-B // t.shape[0]), *([1] * (t.ndim - 1)))[:B].contiguous().cuda()


def bench_knn(B, H, W, ks, k, reps, chunk):
    depth, label = (tiled(a, B) for a in G.knn_scene(7, (min(B, 8), H, W)))
    knn = postproc.KNN(G.NUM_CLASSES, k=k, kernel_size=ks)
    weight, out, flag = knn.dist_kernel.cuda(), torch.empty_like(label), torch.zeros(1, dtype=torch.int32, device="cuda")
    L, stream = _lib.lib(), _lib.stream_ptr(depth.device)

    def kernel():
        _lib.check(L.r2dm_knn_vote(depth.data_ptr(), label.data_ptr(), weight.data_ptr(), out.data_ptr(), B, H, W, ks, ks, k, G.NUM_CLASSES, 1.0,
                                   flag.data_ptr(), stream))

    def oracle():
        return torch.cat([O.knn(depth[s:s + chunk], label[s:s + chunk], ks, k, 1.0, 1.0, G.NUM_CLASSES) for s in range(0, B, chunk)])

    kernel()
    equal = torch.equal(knn(depth, label), oracle()) and torch.equal(out, knn(depth, label))
    t = alternate({"kernel": kernel, "call": lambda: knn(depth, label), "torch": oracle}, reps)
    med = {n: statistics.median(v) for n, v in t.items()}
    return {"window": ks, "k": k, "equal_labels": equal, **{n: summary(v) for n, v in t.items()},
            "kernel_images_per_s": round(B / med["kernel"], 1), "call_images_per_s": round(B / med["call"], 1),
            "torch_images_per_s": round(B / med["torch"], 1), "kernel_over_torch": round(med["torch"] / med["kernel"], 1),
            "call_over_torch": round(med["torch"] / med["call"], 1), "kernel_GB_per_s": round(20.0 * B * H * W / med["kernel"] / 1e9, 1)}


def bench_crf(B, H, W, N, iters, reps, chunk):
    unary, xyz, mask = (tiled(a, B) for a in G.crf_inputs(8, (min(B, 4), N, H, W)))
    crf = postproc.CRFRNN(N, num_iters=iters, **G.crf_kwargs("beta", N))
    state = {k: v.cuda() for k, v in crf.state_dict().items()}
    params, mask4 = crf._params.cuda(), mask[:, None].contiguous()
    bufs = [torch.empty_like(unary) for _ in range(2)]
    L, stream = _lib.lib(), _lib.stream_ptr(unary.device)
    kh, kw = crf.kernel_size

    def kernel():
        q = unary
        for it in range(iters):
            _lib.check(L.r2dm_crf_iter(q.data_ptr(), unary.data_ptr(), xyz.data_ptr(), mask4.data_ptr(), params.data_ptr(), bufs[it % 2].data_ptr(), B, N,
                                       H, W, kh, kw, 1, stream))
            q = bufs[it % 2]
        return q

    def oracle():
        return torch.cat([O.crf(unary[s:s + chunk], xyz[s:s + chunk], mask[s:s + chunk], state, (kh, kw), iters, torch.float32)
                          for s in range(0, B, chunk)])

    crf.max_batch = max(crf.max_batch, B)
    got, want = crf(unary, xyz, mask), oracle()
    diff = float((got - want).abs().max())
    equal = torch.equal(kernel(), got)
    del want
    t = alternate({"kernel": kernel, "call": lambda: crf(unary, xyz, mask), "torch": oracle}, reps)
    med = {n: statistics.median(v) for n, v in t.items()}
    return {"classes": N, "iterations": iters, "window": [kh, kw], "max_abs_diff_to_torch_fp32": diff, "kernel_equals_call": equal,
            **{n: summary(v) for n, v in t.items()}, "kernel_images_per_s": round(B / med["kernel"], 1),
            "call_images_per_s": round(B / med["call"], 1), "torch_images_per_s": round(B / med["torch"], 1),
            "kernel_over_torch": round(med["torch"] / med["kernel"], 1), "call_over_torch": round(med["torch"] / med["call"], 1),
            "kernel_GB_per_s": round(iters * (2 * N + 4) * 4.0 * B * H * W / med["kernel"] / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=16, help="images per call of the torch composition")
    args = ap.parse_args()
    B, H, W = args.batch, args.height, args.width
    np.seterr(all="raise")
    with torch.no_grad():
        res = {"batch": B, "height": H, "width": W, "reps": args.reps,
               "knn3": bench_knn(B, H, W, 3, 3, args.reps, args.chunk), "knn5": bench_knn(B, H, W, 5, 5, args.reps, args.chunk),
               "crf": bench_crf(B, H, W, G.NUM_CLASSES, 3, args.reps, args.chunk)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
