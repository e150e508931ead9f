#!/usr/bin/env python3
"""Generate tests/golden/render.npz by running the REAL reference's utils/render.py on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_render.py /path/to/reference

The reference module imports kornia, which is not needed for anything but ``project_points`` and the rotation matrices of
``make_Rt``: a tiny stand-in module is placed in ``sys.modules`` first.  Its ``project_points`` is kornia's documented closed
form (convert_points_from_homogeneous, then u = fx x + cx, v = fy y + cy); ``axis_angle_to_rotation_matrix`` is a placeholder
(the view comes from r2dm_amd.render.make_Rt, which runs on the host).  The result was NOT run against kornia itself.

Contents (inputs and the reference's outputs only):
  - ``lut_turbo`` / ``lut_viridis``: the two (256,3) tables as the reference computes them;
  - ``colorize_in`` and its uint8 images for both tables: 0, 1, every k/256 with its two fp32 neighbours, values slightly
    outside [0,1];
  - ``raster_coords`` / ``raster_values`` / ``raster_out``: coordinates on integers, within one ulp of the borders 0, H-1, -1
    and H, bilinear weights on either side of 1e-3, on a 12 x 20 image;
  - ``cloud_points`` / ``cloud_colors`` (2,2048,3), a quarter of the points exactly at the origin, rendered through
    generate.py's view at size 64 and 96 (``cloud_bev64`` / ``cloud_bev96``), with ``view_R`` / ``view_t``.
"""
import math
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "render.npz")
RASTER_SHAPE = (12, 20)


def install_kornia_stand_in():
    import torch

    def project_points(point_3d, camera_matrix):
        z = point_3d[..., 2:]
        scale = torch.where(z.abs() > 1e-8, 1.0 / (z + 1e-8), torch.ones_like(z))
        xy = scale * point_3d[..., :2]
        fx, fy = camera_matrix[..., 0, 0], camera_matrix[..., 1, 1]
        cx, cy = camera_matrix[..., 0, 2], camera_matrix[..., 1, 2]
        return torch.stack([xy[..., 0] * fx + cx, xy[..., 1] * fy + cy], dim=-1)

    def axis_angle_to_rotation_matrix(axis_angle):
        raise NotImplementedError("placeholder: the goldens take their view from r2dm_amd.render.make_Rt")

    kornia = types.ModuleType("kornia")
    geometry = types.ModuleType("kornia.geometry")
    conversions = types.ModuleType("kornia.geometry.conversions")
    geometry.project_points = project_points
    conversions.axis_angle_to_rotation_matrix = axis_angle_to_rotation_matrix
    geometry.conversions = conversions
    kornia.geometry = geometry
    sys.modules.update({"kornia": kornia, "kornia.geometry": geometry, "kornia.geometry.conversions": conversions})


def f32(v):
    return np.asarray(v, np.float32)


def neighbours(v):
    v = f32(v)
    return np.concatenate([np.nextafter(v, f32(-np.inf)), v, np.nextafter(v, f32(np.inf))]).astype(np.float32)


def colorize_input():
    k = np.arange(257, dtype=np.float32) / np.float32(256)
    vals = np.concatenate([neighbours(k), f32([-0.25, -1e-6, 1.0 + 1e-6, 1.5, 0.999, 0.5])])
    vals = np.concatenate([vals, np.zeros(-len(vals) % 8, np.float32)])
    return vals.reshape(1, 8, -1)


def raster_case(g):
    H, W = RASTER_SHAPE

    def axis(n):
        special = np.concatenate([np.arange(-1, n + 1, dtype=np.float32), neighbours(f32([0, n - 1, -1, n])),
                                  f32([0.5, n - 1.5, -0.5, n - 0.5, -3.25, n + 2.75])])
        # a fraction f next to an integer: with the other axis on an integer the bilinear weights are f and 1 - f exactly
        fr = neighbours(f32([1e-3, 2e-3]))
        return np.concatenate([special, fr, f32(1.0) - fr, f32(3.0) + f32(2e-3) * f32([0.4, 0.5, 0.6])]).astype(np.float32)

    hs, ws = axis(H), axis(W)
    hh, ww = np.meshgrid(hs, ws, indexing="ij")
    grid = np.stack([hh.ravel(), ww.ravel()], 1)
    rnd = np.stack([g.integers(-2 * 2**12, (H + 2) * 2**12, size=600), g.integers(-2 * 2**12, (W + 2) * 2**12, size=600)], 1) / 2**12
    half = np.stack([np.full(len(ws), 2.5, np.float32), ws], 1)  # weights 0.5 f on either side of 1e-3
    coords = np.concatenate([grid, rnd, half]).astype(np.float32)
    values = (g.integers(-2**12, 2**12, size=(len(coords), 3)) / 2**10).astype(np.float32)
    return coords[None], values[None]


def cloud_case(g, n=16 * 128, batch=2):
    pts = (g.integers(-2**14, 2**14, size=(batch, n, 3)) / 2**15).astype(np.float32)  # +-0.5: a scan divided by max_depth
    pts[..., 2] *= np.float32(0.125)
    pts[:, g.permutation(n)[: n // 4]] = 0.0
    cols = (g.integers(0, 256, size=(batch, n, 3)) / 255).astype(np.float32)
    return pts, cols


def main(reference):
    sys.path.insert(0, reference)
    sys.path.insert(0, ROOT)
    import matplotlib.cm as cm
    import torch

    install_kornia_stand_in()
    from utils import render  # (reference)

    from r2dm_amd.render import make_Rt

    g = np.random.Generator(np.random.PCG64(2024))
    out = {}
    for name, fn in (("turbo", cm.turbo), ("viridis", cm.viridis)):
        out[f"lut_{name}"] = fn(np.linspace(0, 1, 256))[:, :3].astype(np.float32)
    x = colorize_input()
    out["colorize_in"] = x
    out["colorize_turbo"] = render.colorize(torch.from_numpy(x)).numpy()
    out["colorize_viridis"] = render.colorize(torch.from_numpy(x)[:, None], cm.viridis).numpy()

    coords, values = raster_case(g)
    out["raster_coords"], out["raster_values"] = coords, values
    out["raster_out"] = render.bilinear_rasterizer(torch.from_numpy(coords), torch.from_numpy(values), RASTER_SHAPE).numpy()

    pts, cols = cloud_case(g)
    R, t = make_Rt(pitch=math.pi / 3, yaw=math.pi / 4, z=0.8)
    out["cloud_points"], out["cloud_colors"], out["view_R"], out["view_t"] = pts, cols, R.numpy(), t.numpy()
    for size in (64, 96):
        bev = render.render_point_clouds(torch.from_numpy(pts), torch.from_numpy(cols), size=size, R=R, t=t)
        assert torch.isfinite(bev).all() and (bev != 0).any()
        out[f"cloud_bev{size}"] = bev.numpy()
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
