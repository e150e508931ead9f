#!/usr/bin/env python3
"""Times r2dm_ensemble_coherence on one GPU and prints one JSON line: K = 16 members, batch 8, 64 x 1024, the default eight offsets; the
squared distances (``dist``, with ``vario`` left out) and the variogram sums (``vario``, with ``dist`` left out) each against its float64
torch composition on the same GPU and inputs, after comparing the outputs.

The compositions are what one would write without the kernels.  For ``dist``: members and target stacked per channel, masked to E, widened,
and the pairwise squared differences summed over the pixels -- the difference form, no matrix-multiply distance -- in chunks of rows so that
the (rows x K+1 x pixels) intermediate fits.  For ``vario``: per offset ``torch.roll`` of the stacked values and of E, the rows that would
wrap in elevation masked out, float64 roots and masked sums.

Both sides are timed per CALL into buffers allocated once (the C entry itself; ``ensemble_coherence_sums`` adds four allocations), in
alternating windows with HIP events (scripts/bench_completion.py's scheme); medians and the spread of the windows are reported, with the
bytes each part has to read at least ((2 K + 3) floats per pixel), the float64 operations it does, and both over the median time."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_completion import HBM_PEAK, HI, LO, compare  # noqa: E402
from r2dm_amd import _lib, completion  # noqa: E402


def stacked(samples, target, known):
    """v (B,2,K+1,H,W) float64 with the conventions of the kernels, E (B,H,W)"""
    d, rho = samples[:, :, 0], samples[:, :, 4]
    r = target[:, 0]
    E = (known[:, 0] == 0) & (r > LO) & (r < HI)
    depth = torch.cat([torch.where((d > LO) & (d < HI), d, torch.zeros_like(d)), r[:, None]], 1)
    refl = torch.cat([torch.nan_to_num(rho, nan=0.0, posinf=float("inf"), neginf=-float("inf")), target[:, None, 4]], 1)
    return torch.stack([depth, refl], 1).double(), E


def torch_dist(samples, target, known, chunk=4):
    v, E = stacked(samples, target, known)
    v = torch.where(E[:, None, None], v, torch.zeros((), dtype=torch.float64, device=v.device)).flatten(3)  # (B,2,R,P)
    R = v.shape[2]
    rows = [(v[:, :, i:i + chunk, None] - v[:, :, None]).square().sum(-1) for i in range(0, R, chunk)]
    return torch.stack([(known[:, 0] == 0).flatten(1).sum(1).double(), E.flatten(1).sum(1).double()], 1), torch.cat(rows, 2)


def torch_vario(samples, target, known, offsets):
    v, E = stacked(samples, target, known)
    B, _, R, H, W = v.shape
    K = R - 1
    zero = torch.zeros((), dtype=torch.float64, device=v.device)
    h = torch.arange(H, device=v.device)
    out = []
    for dh, dw in offsets:
        pair = E & torch.roll(E, (-dh, -dw), (-2, -1)) & ((h + dh >= 0) & (h + dh < H))[None, :, None]
        root = (v - torch.roll(v, (-dh, -dw), (-2, -1))).abs().sqrt()
        a, m = root[:, :, K], root[:, :, :K].sum(2) / K
        on = lambda x: torch.where(pair[:, None], x, zero).sum((-2, -1))
        out.append(torch.stack([pair.sum((-2, -1)).double()[:, None].expand(B, 2), on((a - m).square()), on(a * a), on(m * m)], -1))
    return torch.stack(out, 2)  # (B,2,O,4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    dev, B, K, H, W = "cuda", args.batch, args.members, 64, 1024
    offsets = completion.DEFAULT_OFFSETS
    gen = torch.Generator(device=dev).manual_seed(0)
    target = torch.rand(B, 5, H, W, generator=gen, device=dev)
    target[:, 0] = 0.5 + 89.5 * target[:, 0]
    samples = target[:, None] + 0.3 * torch.randn(B, K, 5, H, W, generator=gen, device=dev)
    samples[:, :, 0] = torch.where(torch.rand(B, K, H, W, generator=gen, device=dev) < 0.2, torch.zeros_like(samples[:, :, 0]), samples[:, :, 0])
    known = completion.corruption_mask("beams:4", H, W).to(dev)[None].expand(B, 1, H, W).contiguous()

    L = _lib.lib()
    scratch = torch.empty(L.r2dm_ensemble_coherence_scratch_bytes(B, K, H, W, len(offsets)) // 8, dtype=torch.float64, device=dev)
    counts = torch.empty(B, 2, dtype=torch.float64, device=dev)
    dist = torch.empty(B, 2, K + 1, K + 1, dtype=torch.float64, device=dev)
    vario = torch.empty(B, 2, len(offsets), 4, dtype=torch.float64, device=dev)
    host = (ctypes.c_int32 * (2 * len(offsets)))(*[x for o in offsets for x in o])
    stream = _lib.stream_ptr(torch.device(dev))

    def call(d, v):
        _lib.check(L.r2dm_ensemble_coherence(_lib.ptr(samples), _lib.ptr(target), _lib.ptr(known), LO, HI, B, K, H, W, ctypes.cast(host, ctypes.c_void_p),
                                             len(offsets), _lib.ptr(scratch), _lib.ptr(counts), _lib.ptr(d), _lib.ptr(v), stream))
        return counts

    rel = lambda a, b: float(f"{((a - b).abs() / b.abs().clamp(min=1e-300)).max().item():.3e}")
    pixels = B * H * W
    tiles = (K + 1 + 7) // 8
    pairs = tiles * (tiles + 1) // 2
    result = {"shape": [B, K, H, W], "offsets": [list(o) for o in offsets], "windows": args.windows, "reps": args.reps}

    call(dist, None)
    wc, wd = torch_dist(samples, target, known)
    off = ~torch.eye(K + 1, dtype=torch.bool, device=dev)
    entry = {"counts_equal": bool(torch.equal(counts, wc)), "max_rel_diff": rel(dist[:, :, off], wd[:, :, off]),
             "diagonal_zero": bool((dist.diagonal(dim1=-2, dim2=-1) == 0).all()), "symmetric": bool(torch.equal(dist, dist.transpose(-1, -2)))}
    del wc, wd
    th, tt = compare(lambda: call(dist, None), lambda: torch_dist(samples, target, known), args.windows, args.reps)
    nbytes, flops = 4 * pixels * (2 * K + 3), 3 * 64 * pairs * 2 * pixels  # per pixel, channel and tile pair 64 x (subtract, multiply-add)
    entry.update(hip=th, torch=tt, ratio=round(tt["median_s"] / th["median_s"], 1), bytes=nbytes, hbm_bound_fraction=round(nbytes / HBM_PEAK / th["median_s"], 3),
                 fp64_ops=flops, fp64_ops_per_s=float(f"{flops / th['median_s']:.4e}"), tile_pairs=pairs)
    result["dist"] = entry

    call(None, vario)
    wv = torch_vario(samples, target, known, offsets)
    scale = (wv[..., 2] + wv[..., 3]).clamp(min=1e-300)
    entry = {"pairs_equal": bool(torch.equal(vario[..., 0], wv[..., 0])), "max_rel_diff_of_sum_a2": rel(vario[..., 2], wv[..., 2]),
             "max_diff_of_the_other_sums_over_scale": float(f"{((vario[..., [1, 3]] - wv[..., [1, 3]]).abs() / scale[..., None]).max().item():.3e}"),
             "pairs": int(wv[:, 0, :, 0].sum().item())}
    del wv
    th, tt = compare(lambda: call(None, vario), lambda: torch_vario(samples, target, known, offsets), args.windows, args.reps)
    roots = 2 * (K + 1) * int(vario[:, 0, :, 0].sum().item())
    entry.update(hip=th, torch=tt, ratio=round(tt["median_s"] / th["median_s"], 1), bytes=nbytes, hbm_bound_fraction=round(nbytes / HBM_PEAK / th["median_s"], 3),
                 fp64_roots=roots, fp64_roots_per_s=float(f"{roots / th['median_s']:.4e}"))
    result["vario"] = entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
