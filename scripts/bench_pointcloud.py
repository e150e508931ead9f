#!/usr/bin/env python3
"""Times the export of range images as point clouds on one GPU and prints one JSON line: r2dm_amd.pointcloud.images_to_points on
batches of 8 and 64 images of 64 x 1024, both layouts, scan and image order,
  - ``kernels``: the C call alone (r2dm_unproject: count, prefix sum, write) on preallocated buffers, --iters calls between two GPU
    events, no host synchronisation inside the window;
  - ``call``: images_to_points as a user calls it (allocations, the three kernels, the host read of the offsets), GPU events around
    one call;
against the torch composition on the same GPU and the same inputs (``postprocess`` for the model layout, then the mask, a permute,
boolean indexing and a cumsum of the mask counts -- image order; scan order adds a gather of the columns), which is also held to
the same bits.  Every figure is the median of --reps windows after a warm-up, the two sides alternating, with the spread (min ..
max) next to it.  Next to the times: points/s and the achieved bytes/s of the kernels over the traffic the algorithm needs -- the
planes (8 B a pixel for the model layout plus 8 B of angles, 20 B for the sample layout) read in each of the two passes and 16 B
written per kept point."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import r2dm_amd  # noqa: E402
from r2dm_amd import _lib, pointcloud  # noqa: E402

H, W = 64, 1024
DEV = "cuda"


def spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def window(fn, iters=1):
    """ms per call of ``iters`` calls between two GPU events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def torch_export(x, lidar, layout, perm):
    post = lidar.postprocess(x) if layout == "model" else x
    if perm is not None:
        post = post.flatten(2)[:, :, perm]
    else:
        post = post.flatten(2)
    keep = (post[:, 0] > lidar.min_depth) & (post[:, 0] < lidar.max_depth) & torch.isfinite(post[:, 1:4]).all(1)
    points = post[:, 1:5].permute(0, 2, 1)[keep]
    offsets = torch.cat([keep.new_zeros(1, dtype=torch.int64), keep.sum(1).cumsum(0)]).cpu().numpy()
    return points, offsets


def kernels_call(x, lidar, layout, order):
    """The C call on buffers allocated once."""
    L = _lib.lib()
    B = x.shape[0]
    ang = lidar.ray_angles[0].float().contiguous()
    row_start = torch.from_numpy(pointcloud.scan_row_start(ang)).to(DEV) if order == "scan" else None
    points = torch.empty(B * H * W, 4, device=DEV)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=DEV)
    need = L.r2dm_unproject_scratch_bytes(B, H, W)
    scratch = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    sptr = scratch.data_ptr() + (-scratch.data_ptr()) % 256
    stream = _lib.stream_ptr(torch.device(DEV))
    keep = (x, ang, row_start, points, offsets, scratch)

    def call():
        _lib.check(L.r2dm_unproject(x.data_ptr(), pointcloud.LAYOUTS[layout], ang.data_ptr(), _lib.ptr(row_start), points.data_ptr(), None,
                                    offsets.data_ptr(), B, H, W, float(lidar.min_depth), float(lidar.max_depth),
                                    _lib.DEPTH_FORMATS[lidar.depth_format], float(lidar.min_depth), float(lidar.max_depth), sptr, need, stream))

    call.keep = keep
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=50, help="C calls per timed window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pointcloud.py measures on an MI355X: no ROCm device found")
    lidar = r2dm_amd.LiDARUtility((H, W), "log_depth", 1.45, 80.0).to(DEV)
    rs = torch.from_numpy(pointcloud.scan_row_start(lidar.ray_angles).astype(np.int64)).to(DEV)
    perm = (rs[:, None] - torch.arange(W, device=DEV)[None]) % W + torch.arange(H, device=DEV)[:, None] * W  # scan order, as a gather
    res = {"grid": [H, W], "reps": args.reps, "iters": args.iters, "unit": "ms per batch", "cases": []}
    for B in args.batches:
        g = torch.Generator(device=DEV).manual_seed(B)
        x = torch.rand(B, 2, H, W, device=DEV, generator=g) * 2 - 1
        post = lidar.postprocess(x)
        for layout, src in (("model", x), ("sample", post)):
            for order in ("scan", "image"):
                p = perm.flatten() if order == "scan" else None
                hip = lambda: pointcloud.images_to_points(src, lidar, layout=layout, order=order)
                ref = lambda: torch_export(src, lidar, layout, p)
                kern = kernels_call(src, lidar, layout, order)
                (pts, off), (want, want_off) = hip(), ref()
                assert np.array_equal(off, want_off) and torch.equal(pts.view(torch.int32), want.contiguous().view(torch.int32)), \
                    "the kernels and the torch composition disagree"
                for _ in range(3):  # warm-up of every shape the windows use
                    hip(), ref(), window(kern, args.iters)
                t_hip, t_ref, t_kern = [], [], []
                for _ in range(args.reps):
                    t_hip.append(window(hip))
                    t_ref.append(window(ref))
                    t_kern.append(window(kern, args.iters))
                kept, pixels = int(off[-1]), B * H * W
                traffic = 2 * pixels * (16 if layout == "model" else 20) + 16 * kept
                k_med, h_med, r_med = (statistics.median(t) for t in (t_kern, t_hip, t_ref))
                res["cases"].append({
                    "batch": B, "layout": layout, "order": order, "points": kept, "needed_bytes": traffic,
                    "kernels": spread(t_kern), "call": spread(t_hip), "torch_composition": spread(t_ref),
                    "kernels_points_per_s": round(kept / (k_med * 1e-3)), "kernels_bytes_per_s": round(traffic / (k_med * 1e-3)),
                    "call_points_per_s": round(kept / (h_med * 1e-3)), "torch_over_call": round(r_med / h_med, 3),
                    "torch_over_kernels": round(r_med / k_med, 3)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
