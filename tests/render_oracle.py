"""Torch restatement of the rendering contract ("Rendering"; the reference's utils/render.py and
generate.py:44-59), parametrised by dtype.  In fp32 on the CPU it reproduces the reference bit for bit
(tests/test_render_cpu.py pins it to tests/golden/render.npz); its fp64 evaluation is the truth of the GPU tests.

Colour-table look-ups are part of the fp32 contract in every dtype: a table's bytes come from its fp32 values."""
import math

import numpy as np
import torch


def lut_bytes(lut):
    """(256,3) fp32 table -> the uint8 colours colorize() returns."""
    return lut.float().mul(255).clamp(0, 255).byte()  # (on the table's device)


def colorize(tensor, lut):
    """(B,1,H,W) / (B,H,W) -> uint8 (B,3,H,W)."""
    t = tensor.squeeze(1) if tensor.ndim == 4 else tensor
    ids = (t * 256).clamp(0, 255).long()
    return lut_bytes(lut.to(t.device))[ids].permute(0, 3, 1, 2)


def raster_terms(coords, values, out_shape):
    """The four (index, term) sets of every point, in the dtype of ``values``: indices (4,B,N) int64 in the order top-left,
    top-right, bottom-left, bottom-right, terms (4,B,N,C).  A point with a non-finite coordinate has zero terms."""
    H, W = out_shape
    ok = torch.isfinite(coords).all(-1, keepdim=True)
    coords = torch.where(ok, coords, torch.zeros_like(coords)).to(values.dtype)
    h, w = coords[..., [0]], coords[..., [1]]
    h_t, w_l = torch.floor(h), torch.floor(w)
    h_b, w_r = h_t + 1, w_l + 1
    h_ts, h_bs = h_t.clamp(0.0, H - 1), h_b.clamp(0.0, H - 1)
    w_ls, w_rs = w_l.clamp(0.0, W - 1), w_r.clamp(0.0, W - 1)
    one = lambda m: m.to(values.dtype)
    wh = ((h_b - h) * one(h_t == h_ts), (h - h_t) * one(h_b == h_bs))
    ww = ((w_r - w) * one(w_l == w_ls), (w - w_l) * one(w_r == w_rs))
    idx, terms = [], []
    for a, hs in enumerate((h_ts, h_bs)):
        for b, ws in enumerate((w_ls, w_rs)):
            bw = wh[a] * ww[b]
            bw = bw * one(bw >= 1e-3)
            terms.append(torch.where(ok, values * bw, torch.zeros_like(values)))
            idx.append((ws.long() + W * hs.long())[..., 0])
    return torch.stack(idx), torch.stack(terms)


def bilinear_rasterizer(coords, values, out_shape, dtype=torch.float32):
    """(B,N,2) [h, w], (B,N,C) -> (B,C,H,W): four scatter_adds in the reference's order."""
    H, W = out_shape
    B, _, C = values.shape
    idx, terms = raster_terms(coords.to(dtype), values.to(dtype), out_shape)
    out = torch.zeros(B, H * W, C, dtype=dtype, device=values.device)
    for k in range(4):
        out.scatter_add_(1, idx[k][..., None].expand(-1, -1, C), terms[k])
    return out.reshape(B, H, W, C).permute(0, 3, 1, 2)


def exact_sums(coords, values, out_shape):
    """Per pixel and channel, of the fp32 terms T_k: (sum T_k, sum |T_k|) in fp64, each (B,C,H,W), and max |T| of the call."""
    H, W = out_shape
    B, _, C = values.shape
    idx, terms = raster_terms(coords.float(), values.float(), out_shape)
    s, a = torch.zeros(B, H * W, C, dtype=torch.float64), torch.zeros(B, H * W, C, dtype=torch.float64)
    for k in range(4):
        i = idx[k][..., None].expand(-1, -1, C)
        s.scatter_add_(1, i, terms[k].double())
        a.scatter_add_(1, i, terms[k].double().abs())
    shape = lambda t: t.reshape(B, H, W, C).permute(0, 3, 1, 2)
    return shape(s), shape(a), terms.abs().max().item()


def project(points, colors, size, R, t, focal_length=1.0, dtype=torch.float32):
    """The per-point half of render_point_clouds: uv (B,N,2), weight (B,N,1), masked colours (B,N,3)."""
    p = points.to(dtype).clone()
    p[..., 2] *= -1
    colors = torch.ones_like(p) if colors is None else colors.to(dtype)
    R, t = R.to(p.device, dtype).reshape(3, 3), t.to(p.device, dtype).reshape(3)
    # torch's own product, as the reference: on the CPU it evaluates sum_i p_i R[i][j] in the order i = 0, 1, 2 as a chain of
    # fused multiply-adds, within an ulp of the unfused sum the kernel forms
    p = p @ R
    p = p + t
    z = p[..., 2]
    s = torch.where(z.abs() > 1e-8, 1.0 / (z + 1e-8), torch.ones_like(z))
    uv = torch.stack([(s * p[..., 0]) * focal_length + 0.5, (s * p[..., 1]) * focal_length + 0.5], dim=-1)
    uv = uv * size
    mask = (0 < uv) & (uv < size - 1)
    mask = torch.logical_and(mask[..., [0]], mask[..., [1]])
    colors = colors * mask
    uv = size - uv
    depth = torch.norm(p, p=2, dim=-1, keepdim=True)
    weight = 1.0 / torch.exp(3.0 * depth)
    weight = weight * (depth > 1e-8)
    return uv, weight, colors


def render_point_clouds(points, colors=None, size=800, R=None, t=None, focal_length=1.0, dtype=torch.float32, return_hit=False):
    """(B,N,3), (B,N,3) or None -> (B,3,size,size); with ``return_hit`` also the (B,size,size) mask of the pixels that received weight."""
    R = torch.eye(3) if R is None else R
    t = torch.zeros(3) if t is None else t
    uv, weight, colors = project(points, colors, size, R, t, focal_length, dtype)
    bev = bilinear_rasterizer(uv, weight * colors, (size, size), dtype)
    den = bilinear_rasterizer(uv, weight, (size, size), dtype)
    bev = bev / (den + 1e-8)
    return (bev, den[:, 0] > 0) if return_hit else bev


def rotation(roll=0.0, pitch=0.0, yaw=0.0):
    """Rz(yaw) Ry(pitch) Rx(roll) in closed form, fp64."""
    cr, sr, cp, sp, cy, sy = math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch), math.cos(yaw), math.sin(yaw)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    Rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return Rz @ Ry @ Rx


def generate_view():
    """generate.py:52: (R (1,3,3), t (1,3)) in fp32."""
    return (torch.from_numpy(rotation(pitch=math.pi / 3, yaw=math.pi / 4)).float()[None], torch.tensor([[0.0, 0.0, 0.8]]))


def to_xyz(metric, ray_angles, min_depth, max_depth):
    """LiDARUtility.to_xyz: metric (B,1,H,W), ray_angles (1,2,H,W) [elevation, azimuth] -> (B,3,H,W), in metric's dtype."""
    mask = (metric > min_depth) & (metric < max_depth)
    phi, theta = ray_angles[:, [0]].to(metric.dtype), ray_angles[:, [1]].to(metric.dtype)
    xyz = torch.cat((metric * phi.cos() * theta.cos(), metric * phi.cos() * theta.sin(), metric * phi.sin()), dim=1)
    return xyz * mask.to(metric.dtype)


def render_frames(x, ray_angles, min_depth, max_depth, turbo, viridis, size=800, dtype=torch.float32):
    """generate.py:44-59: x (N,2,H,W) -> img (N,3,2H,W), bev (N,3,size,size), and the (N,size,size) mask of the pixels any point hit."""
    x = x.to(dtype)
    N, _, H, W = x.shape
    img = colorize(x.reshape(N, 1, 2 * H, W), turbo).to(dtype) / 255
    xyz = to_xyz(x[:, [0]] * max_depth, ray_angles, min_depth, max_depth)
    xyz = xyz / max_depth
    z_min, z_max = -2 / max_depth, 0.5 / max_depth
    z = (xyz[:, [2]] - z_min) / (z_max - z_min)
    colors = colorize(z.clamp(0, 1), viridis).to(dtype) / 255
    R, t = generate_view()
    flat = lambda a: a.reshape(N, 3, H * W).permute(0, 2, 1)
    bev, hit = render_point_clouds(flat(xyz), 1 - flat(colors), size, R, t, dtype=dtype, return_hit=True)
    return img, 1 - bev, hit


def synthetic_frames(n, H, W, seed=0, max_depth=80.0):
    """(n,2,H,W) fp32 frames as generate.py leaves them: a smooth depth (walls at 4 .. 45 m around the sensor, nearer towards
    the lower rings) plus noise, divided by max_depth, one point in 35 zeroed; reflectance in [0,1]."""
    g = np.random.Generator(np.random.PCG64(seed))
    az = np.linspace(0, 2 * np.pi, W, endpoint=False)[None, None, :]
    ring = np.linspace(0, 1, H)[None, :, None]
    phase = g.uniform(0, 2 * np.pi, size=(n, 1, 1))
    depth = 24.5 + 20.5 * np.sin(3 * az + phase) * np.cos(az - phase)
    depth = depth * (1.0 - 0.6 * ring) + g.normal(0, 0.15, size=(n, H, W))
    depth = np.clip(depth, 0.0, max_depth)
    depth[g.integers(0, 35, size=depth.shape) == 0] = 0.0
    refl = np.clip(0.3 + 0.2 * np.sin(5 * az + ring) + g.normal(0, 0.05, size=(n, H, W)), 0, 1)
    return torch.from_numpy(np.stack([depth / max_depth, refl], 1).astype(np.float32))
