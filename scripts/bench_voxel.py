#!/usr/bin/env python3
"""Times voxel occupancy (r2dm_voxel_occupancy, r2dm_amd.geometry.voxel_occupancy_counts) on one GPU and prints one JSON line.

Workload: ``--batch`` (8) scans of 64 x 1024 rays, voxel sizes 0.1 / 0.2 / 0.5 m, as pairs (K = 1: a prediction against the scan) and as
ensembles of K = 16 members per scan.  The scans are synthetic: the HDL-64E ray grid of ``r2dm_amd.synthetic`` looking at a ground plane
inside a box of walls, per scan a different sensor height and box; a member is the scan with 1 % multiplicative range noise and 5 % of
its rays dropped.  Clouds are in image order, as ``clouds_of_samples`` returns them.

The comparison is the torch composition on the same GPU and inputs: keys by the same float32 division, ``torch.unique`` per cloud, and
the set sizes through a second ``unique`` over the concatenation of a group's key sets (its inverse index counts the members per voxel).
The script first asserts that the two agree exactly, then times them in alternating windows (HIP events; medians and the spread of the
windows).  Both times include the host side of their wrappers.  ``hip_split`` times the library call alone (``_voxel_launch`` on device
tensors already in place, no status read), and gives the insert rate: point-size insertions (one compare-and-swap and one atomic OR each
when the first slot is the right one) per second."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from r2dm_amd import geometry, synthetic  # noqa: E402

HALF = 1 << 20


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


def stats(t):
    return {"median_s": float(f"{statistics.median(t):.4e}"), "min_s": float(f"{min(t):.4e}"), "max_s": float(f"{max(t):.4e}")}


def compare(fns, windows, reps):
    for fn in fns.values():
        fn()
    times = {name: [] for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            times[name].append(window(fn, reps))
    return {name: stats(t) for name, t in times.items()}


def scans(B, H, W, gen, dev):
    """(B,H,W,3) points and (B,H,W) depth of B synthetic scans"""
    el, az = synthetic.hdl64e_ray_angles(H, W)[0].to(dev)
    d = torch.stack([el.cos() * az.cos(), el.cos() * az.sin(), el.sin()], dim=-1)                   # (H,W,3) unit rays
    height = 1.5 + 0.5 * torch.rand(B, 1, 1, generator=gen, device=dev)
    half = 10 + 30 * torch.rand(B, 1, 1, 2, generator=gen, device=dev)                              # the box's half widths in x and y
    ground = torch.where(d[..., 2] < 0, height / (-d[..., 2]).clamp_min(1e-6), torch.full_like(height, 1e9).expand(B, H, W))
    wall = (half / d[..., :2].abs().clamp_min(1e-6)).min(dim=-1).values
    depth = torch.minimum(ground, wall).clamp(max=79.0)
    return depth[..., None] * d, depth


def clouds(points, depth, keep):
    """image-ordered ragged clouds of the kept rays: ((total,4), offsets)"""
    n = keep.flatten(1).sum(1)
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device=n.device), n.cumsum(0)]).cpu().numpy()
    rows = torch.cat([points, depth[..., None]], dim=-1)[keep]
    return rows.float().contiguous(), off


def torch_keys(p, size):
    v = torch.floor(p[:, :3] / size).long() + HALF   # (float32 / float32: the same division)
    return v[:, 0] << 42 | v[:, 1] << 21 | v[:, 2]


def torch_counts(a, off_a, b, off_b, members, targets, sizes):
    """member (G,S,K,2), hist (G,S,2,K+1) by unique per cloud and a second unique over a group's concatenated key sets"""
    G, K = members.shape
    dev = a.device
    member = torch.zeros(G, len(sizes), K, 2, dtype=torch.int64, device=dev)
    hist = torch.zeros(G, len(sizes), 2, K + 1, dtype=torch.int64, device=dev)
    for s, size in enumerate(sizes):
        size = torch.tensor(size, dtype=torch.float32, device=dev)
        ka, kb = torch_keys(a, size), torch_keys(b, size)
        for g in range(G):
            sets = [torch.unique(ka[off_a[k]:off_a[k + 1]]) for k in members[g]]
            tset = torch.unique(kb[off_b[targets[g]]:off_b[targets[g] + 1]])
            every = torch.cat(sets)
            union, inv = torch.unique(torch.cat([every, tset]), return_inverse=True)
            c = torch.bincount(inv[:every.numel()], minlength=union.numel())
            o = torch.bincount(inv[every.numel():], minlength=union.numel())
            hist[g, s] = torch.bincount(o * (K + 1) + c, minlength=2 * (K + 1)).reshape(2, K + 1)
            ends = np.cumsum([0] + [t.numel() for t in sets])
            in_target = o[inv[:every.numel()]]
            for k in range(K):
                member[g, s, k, 0] = sets[k].numel()
                member[g, s, k, 1] = in_target[ends[k]:ends[k + 1]].sum()
    return member, hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--sizes", type=float, nargs="+", default=[0.1, 0.2, 0.5])
    ap.add_argument("--members", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(0)
    B, H, W = args.batch, args.height, args.width
    sizes = [float(s) for s in geometry._voxel_sizes(args.sizes)]
    points, depth = scans(B, H, W, gen, dev)
    b, off_b = clouds(points, depth, depth < 78.0)
    result = {"batch": B, "rays": H * W, "sizes": sizes, "windows": args.windows, "reps": args.reps, "target_points": int(off_b[-1])}
    for K in args.members:
        noise = 1 + 0.01 * torch.randn(B, K, H, W, generator=gen, device=dev)
        keep = (torch.rand(B, K, H, W, generator=gen, device=dev) > 0.05) & (depth[:, None] < 78.0)
        a, off_a = clouds((points[:, None] * noise[..., None]).flatten(0, 1), (depth[:, None] * noise).flatten(0, 1), keep.flatten(0, 1))
        members, targets = np.arange(B * K).reshape(B, K), np.arange(B)
        got = geometry.voxel_occupancy_counts(a, off_a, b, off_b, members, targets, sizes)
        want = torch_counts(a, off_a, b, off_b, members, targets, sizes)
        assert torch.equal(got["member"], want[0]) and torch.equal(got["hist"], want[1]), f"K = {K}: the kernel and the torch composition differ"
        # the library call alone: everything on the device already
        oa, ob = torch.from_numpy(off_a).to(dev), torch.from_numpy(off_b).to(dev)
        md, td = torch.from_numpy(members).to(dev), torch.from_numpy(targets).to(dev)
        group_points = int(max((off_a[K * (g + 1)] - off_a[K * g]) + (off_b[g + 1] - off_b[g]) for g in range(B)))
        fns = {"hip": lambda: geometry.voxel_occupancy_counts(a, off_a, b, off_b, members, targets, sizes)["hist"],
               "hip_split": lambda: geometry._voxel_launch(a, oa, B * K, b, ob, B, md, td, np.asarray(sizes, np.float32), group_points)[1],
               "torch": lambda: torch_counts(a, off_a, b, off_b, members, targets, sizes)[1]}
        entry = compare(fns, args.windows, args.reps)
        inserts = (int(off_a[-1]) + int(off_b[-1])) * len(sizes)
        hist = got["hist"].sum(0)
        entry.update(members=K, member_points=int(off_a[-1]), max_group_points=group_points, table_slots=geometry._voxel_capacity(group_points),
                     scratch_bytes=B * len(sizes) * geometry._voxel_capacity(group_points) * 16, inserts=inserts,
                     voxels=[int(v) for v in hist.sum((1, 2)).tolist()],
                     inserts_per_s=float(f"{inserts / entry['hip_split']['median_s']:.4e}"),
                     ratio_torch=round(entry["torch"]["median_s"] / entry["hip"]["median_s"], 2),
                     iou=[float(f"{v:.4f}") for v in geometry.occupancy_from_counts(got["member"].sum(0), hist)["any_iou"].tolist()])
        result[f"K{K}"] = entry
        del a, got, want
    print(json.dumps(result))


if __name__ == "__main__":
    main()
