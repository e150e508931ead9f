"""Raw LiDAR scans to range images as HIP kernels: ``load_points_as_images`` of the reference's dataset builders
(data/kitti_360/kitti_360.py:34-93, the same in data/kitti_raw) and the builder's ``xyzrdm *= mask``, for a batch of scans.

- ``load_scans`` reads Velodyne ``.bin`` files into one ``(total,4)`` buffer with ``offsets``.
- ``project_scans`` maps every point to its grid cell (spherical, or scan unfolding), keeps the nearest point of every cell and
  writes the ``[x, y, z, reflectance, depth, mask]`` planes.  It runs on the GPU; nothing falls back to the CPU.
- ``load_points_as_images`` has the reference's signature and return value.
- ``known_from_scan`` turns the planes into the ``(B,2,H,W)`` input of ``repaint`` (completion_demo.py:66-75).

Where the reference leaves a choice open (equal depths in one cell: unstable ``argsort``) the lowest index in the file wins, on every
call.  A point whose depth is not a finite number > 0 (NaN / inf coordinates, the origin) never wins a cell; under scan unfolding it
still counts in the sequence.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib

LAYOUTS = {"xyzrdm": 0, "sample": 1}
_PROJECTIONS = {"unfolding": True, "spherical": False}


def parse_projection(name: str):
    """``cfg.data.projection`` -> (scan_unfolding, width): ``"unfolding-2048"`` -> ``(True, 2048)``."""
    try:
        kind, width = str(name).split("-")
        return _PROJECTIONS[kind], _positive(int(width))
    except (ValueError, KeyError):
        raise ValueError(f"unknown projection {name!r}: expected 'unfolding-<width>' or 'spherical-<width>'") from None


def _positive(v: int) -> int:
    if v < 1:
        raise ValueError(v)
    return v


def load_scans(paths):
    """Velodyne ``.bin`` files (fp32 [x, y, z, reflectance] rows) -> ``points`` (total,4) float32 and ``offsets`` (len + 1) int64:
    scan k is ``points[offsets[k]:offsets[k + 1]]``."""
    scans = []
    for p in paths:
        size = os.path.getsize(p)
        if size % 16:
            raise ValueError(f"{p}: {size} bytes is not a whole number of 16-byte [x, y, z, reflectance] points")
        scans.append(np.fromfile(p, dtype=np.float32).reshape(-1, 4))
    offsets = np.zeros(len(scans) + 1, np.int64)
    np.cumsum([len(s) for s in scans], out=offsets[1:])
    points = np.concatenate(scans) if scans else np.zeros((0, 4), np.float32)
    return points, offsets


def _check_offsets(offsets, total: int) -> np.ndarray:
    if isinstance(offsets, torch.Tensor):
        offsets = offsets.detach().cpu().numpy()
    off = np.ascontiguousarray(np.asarray(offsets), dtype=np.int64)
    if off.ndim != 1 or off.size < 1:
        raise ValueError(f"offsets must be (B+1,), got shape {off.shape}")
    if off[0] != 0 or off[-1] != total or (np.diff(off) < 0).any():
        raise ValueError(f"offsets must rise from 0 to the number of points ({total}), got {off[0]} .. {off[-1]}")
    return off


@torch.no_grad()
def project_scans(points, offsets, H: int = 64, W: int = 2048, scan_unfolding: bool = True, min_depth: float = 1.45,
                  max_depth: float = 80.0, apply_mask: bool = True, out_width: int | None = None, layout: str = "xyzrdm",
                  device=None) -> torch.Tensor:
    """``points`` (total,4) [x, y, z, reflectance] -- a ROCm tensor, or a numpy array that is uploaded to ``device`` -- and
    ``offsets`` (B+1,) as ``load_scans`` returns them -> ``(B,6,H,out_width)`` [x, y, z, reflectance, depth, mask]
    (``layout="xyzrdm"``) or ``(B,5,H,out_width)`` [depth, x, y, z, reflectance] (``layout="sample"``: what the BEV metrics read).

    ``apply_mask`` multiplies every plane by the depth-window mask, as the dataset builder does; ``False`` is the raw return value
    of the reference's ``load_points_as_images``.  ``out_width`` < ``W`` picks columns as ``F.interpolate(mode="nearest-exact")``."""
    if layout not in LAYOUTS:
        raise ValueError(f"unknown layout {layout!r}: expected one of {sorted(LAYOUTS)}")
    if tuple(points.shape[1:]) != (4,) or len(points.shape) != 2:
        raise ValueError(f"expected points (total,4), got {tuple(points.shape)}")
    H, W = int(H), int(W)
    out_width = W if out_width is None else int(out_width)
    if H < 1 or W < 1 or not 1 <= out_width <= W:
        raise ValueError(f"grid {H}x{W}, out_width {out_width}: sizes must be >= 1 and out_width <= W")
    off = _check_offsets(offsets, points.shape[0])
    B = off.size - 1
    if isinstance(points, np.ndarray):
        if not torch.cuda.is_available():
            raise _lib.R2DMError("project_scans runs as HIP kernels on an MI355X and has no CPU fallback: no ROCm device found")
        points = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to("cuda" if device is None else device)
    _lib.require_gpu(points, "points")
    points = _lib.f32c(points)
    out = torch.empty(B, 6 if layout == "xyzrdm" else 5, H, out_width, dtype=torch.float32, device=points.device)
    if not B:
        return out
    L = _lib.lib()
    need = L.r2dm_project_scratch_bytes(points.shape[0], B, H, W, int(bool(scan_unfolding)))
    if not need:
        raise ValueError(f"{B} scans of {H}x{W} with {points.shape[0]} points: beyond the limits of r2dm_project_scans")
    scratch = torch.empty(need + 256, dtype=torch.uint8, device=points.device)
    base = (-scratch.data_ptr()) % 256  # 256-byte aligned start
    with torch.cuda.device(points.device):
        _lib.check(L.r2dm_project_scans(_lib.ptr(points), off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _lib.ptr(out), B, H, W, out_width,
                                        int(bool(scan_unfolding)), float(min_depth), float(max_depth), int(bool(apply_mask)), LAYOUTS[layout],
                                        scratch.data_ptr() + base, scratch.numel() - base, _lib.stream_ptr(points.device)))
    return out


def load_points_as_images(point_path, scan_unfolding: bool = True, H: int = 64, W: int = 2048, min_depth: float = 1.45,
                          max_depth: float = 80.0) -> np.ndarray:
    """The reference's function: one ``.bin`` file -> ``(H,W,6)`` float32 [x, y, z, reflectance, depth, mask], unmasked."""
    points, offsets = load_scans([point_path])
    out = project_scans(points, offsets, H=H, W=W, scan_unfolding=scan_unfolding, min_depth=min_depth, max_depth=max_depth,
                        apply_mask=False)
    return out[0].permute(1, 2, 0).contiguous().cpu().numpy()


@torch.no_grad()
def known_from_scan(xyzrdm: torch.Tensor, lidar_utils, resolution) -> torch.Tensor:
    """completion_demo.py:66-75: masked planes ``(B,6,H,W)`` (``project_scans(..., apply_mask=True)``) -> ``(B,2,*resolution)``, the
    depth in the model's coding and the reflectance, both in [-1,1], with -1 where no point was measured."""
    if xyzrdm.ndim != 4 or xyzrdm.shape[1] != 6:
        raise ValueError(f"expected (B,6,H,W) [x, y, z, reflectance, depth, mask], got {tuple(xyzrdm.shape)}")
    depth = lidar_utils.normalize(lidar_utils.convert_depth(xyzrdm[:, [4]].float()))
    rflct = lidar_utils.normalize(xyzrdm[:, [3]].float())
    mask = xyzrdm[:, [5]].float()
    x = torch.cat([depth, rflct], dim=1)
    x = mask * x + (1 - mask) * -1
    return F.interpolate(x, size=tuple(resolution), mode="nearest-exact")
