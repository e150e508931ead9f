"""Torch restatement of the surface-normal contract (include/r2dm_hip.h, DESIGN.md section 4, "Surface normals"; the reference's
utils/render.py:145-236 and train.py:227-239), parametrised by dtype, every operation written out in the contract's order: no
``torch.norm``, no ``torch.cross``, no ``mean``.  In fp32 it is what the kernels must return bit for bit; in fp64 it equals the
reference's fp64 run up to the order of a few additions (tests/test_normals_cpu.py) and is the truth of the GPU tests."""
import numpy as np
import torch

import render_oracle as R

# (dh, dw) in units of d, k = 0 .. 7
OFFSETS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))


def neighbours(points, d):
    """(B,3,H,W) -> (8,B,3,H,W): the point at (clamp(h + dh, 0, H - 1), (w + dw) mod W) for the eight offsets."""
    H, W = points.shape[2:]
    h, w = torch.arange(H, device=points.device), torch.arange(W, device=points.device)
    return torch.stack([points[:, :, (h + dh * d).clamp(0, H - 1)][:, :, :, (w + dw * d) % W] for dh, dw in OFFSETS])


def sqrt(s):
    """The correctly rounded square root the contract asks for.  torch's own fp32 ``sqrt`` on the CPU is not that on every build (the AVX-512
    one is an ulp off on 0.65 % of random values, measured against numpy); taken in fp64 and rounded it is: 53 >= 2 x 24 + 2 bits, so the
    second rounding cannot change the result, even where the fp64 root itself is an ulp off."""
    if s.dtype == torch.float32 and not s.is_cuda:
        return torch.sqrt(s.double()).float()
    return torch.sqrt(s)


def norm(v):
    """(...,3,H,W) -> (...,H,W): sqrt((v0 v0 + v1 v1) + v2 v2)."""
    x, y, z = v.unbind(-3)
    return sqrt((x * x + y * y) + z * z)


def cross(u, v):
    u0, u1, u2 = u.unbind(-3)
    v0, v1, v2 = v.unbind(-3)
    return torch.stack([u1 * v2 - u2 * v1, u2 * v0 - u0 * v2, u0 * v1 - u1 * v0], dim=-3)


def closest_pair(V):
    """(8,B,3,H,W) -> (B,H,W) int64: the k with the smallest |V_k| + |V_(k+2)%8|, the lowest on a tie."""
    length = norm(V)
    dist = length + length.roll(-2, 0)
    best, index = dist[0], torch.zeros(dist.shape[1:], dtype=torch.int64, device=dist.device)
    for k in range(1, 8):
        better = dist[k] < best
        best, index = torch.where(better, dist[k], best), torch.where(better, torch.full_like(index, k), index)
    return index


def estimate_surface_normal(points, d=2, mode="closest", dtype=torch.float32, return_index=False):
    """(B,3,H,W) -> (B,3,H,W) in ``dtype``; with ``return_index`` also the chosen k (B,H,W) of the closest mode."""
    p = points.to(dtype)
    V = neighbours(p, d) - p
    V2 = V.roll(-2, 0)  # V2[k] = V[(k + 2) % 8]
    index = None
    if mode == "closest":
        index = closest_pair(V)
        pick = index[None, :, None].expand(1, -1, 3, -1, -1)
        n = cross(V.gather(0, pick)[0], V2.gather(0, pick)[0])
    elif mode == "mean":
        c = cross(V, V2)
        n = c[0]
        for k in range(1, 8):
            n = n + c[k]
        n = n / 8
    else:
        raise NotImplementedError(mode)
    out = n / (norm(n)[:, None] + 1e-8)
    return (out, index) if return_index else out


def ray_trig(ray_angles):
    """(1,2,H,W) [elevation, azimuth] -> (4,H,W) fp32 on the CPU: cos / sin of the elevation, cos / sin of the azimuth."""
    ang = ray_angles[0].float()
    return torch.stack([ang[0].cos(), ang[0].sin(), ang[1].cos(), ang[1].sin()])


def frame_xyz(metric, trig, min_depth, max_depth, dtype=torch.float32):
    """train.py:228-232 on the fp32 planes ``trig`` (4,H,W): metric (B,1,H,W) -> to_xyz(metric) / max_depth * mask, (B,3,H,W)."""
    lo, hi = float(np.float32(min_depth)), float(np.float32(max_depth))  # (the thresholds are fp32 numbers in every dtype)
    metric = metric.to(dtype)
    mask = ((metric > lo) & (metric < hi)).to(dtype)
    cp, sp, ct, st = trig.to(dtype)
    xyz = torch.cat((((metric * cp) * ct) * mask, ((metric * cp) * st) * mask, (metric * sp) * mask), dim=1)
    return xyz / hi * mask


def normal_colors(normals):
    return (-normals + 1) / 2


def flat(a):
    """(B,3,H,W) -> (B,HW,3)."""
    return a.reshape(a.shape[0], 3, -1).permute(0, 2, 1)


VIEW_T = (0.0, 0.0, 1.0)  # train.py:238; no rotation


def render_normals(metric, trig, min_depth, max_depth, size=800, d=2, mode="closest", dtype=torch.float32, colors=None, return_hit=False):
    """train.py:227-239 -> colors (B,3,H,W), bev (B,3,size,size) [, hit (B,size,size)].  ``colors`` given: they replace the normals'
    colours in the view (the GPU tests fix them to the fp32 restatement's, so that a near-tie of the closest pair cannot flip a
    colour between two precisions)."""
    xyz = frame_xyz(metric, trig, min_depth, max_depth, dtype)
    if colors is None:
        colors = normal_colors(estimate_surface_normal(xyz, d, mode, dtype))
    colors = colors.to(dtype)
    out = R.render_point_clouds(flat(xyz), flat(colors), size, None, torch.tensor(VIEW_T), dtype=dtype, return_hit=return_hit)
    return (colors, *out) if return_hit else (colors, out)
