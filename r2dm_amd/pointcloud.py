"""Range images to point clouds as HIP kernels (r2dm_amd/csrc/pointcloud.hip): the inverse of ``projection.project_scans``.

- ``images_to_points`` turns a batch of range images -- the model's samples ``(B,2,H,W)`` or post-processed ``(B,5,H,W)`` maps --
  into the batch's valid pixels as ``[x, y, z, reflectance]`` rows in one buffer with ``offsets``, what ``load_scans`` returns and
  ``project_scans`` accepts.  It runs on the GPU; nothing falls back to the CPU.
- ``save_scans`` writes one Velodyne ``.bin`` per scan (the inverse of ``load_scans``), ``save_ply`` a binary PLY.
- ``scan_row_start`` and ``centred_ray_angles`` are the host helpers of the scan order.

The order of the rows is part of the contract.  ``order="image"`` is row-major.  ``order="scan"`` (the default) is the order a
spinning sensor writes: rings top to bottom, inside a ring increasing azimuth starting at 0, i.e. the columns fall cyclically from
``scan_row_start``'s column.  A ring then ends in the 4th quadrant and the next starts in the 1st, which is the delimiter that scan
unfolding (``project_scans(..., scan_unfolding=True)``, the reference's data/kitti_360/kitti_360.py:52-74) counts to find a point's
row: a cloud in scan order projects back to the rows it came from, a row-major cloud does not.

Rays on cell edges.  The project's default grid (``synthetic.hdl64e_ray_angles``, the reference's train.py:100-101) puts every ray on
the upper left CORNER of its cell.  A cloud exported along such rays does not re-project to its own columns, nor to its own rows
under the spherical projection, because the projection's ``floor`` falls on the cell boundary: at 64 x 1024 about 2 % of the columns
and about half of the spherical rows are off by one (the unfolding rows are right).  ``centred_ray_angles`` puts the rays at the cell
centres, where the round trip is exact.  The export still follows ``lidar_utils.ray_angles`` by default, because those are the
angles the checkpoint was trained with; pass ``ray_angles=centred_ray_angles(H, W)`` for clouds that must re-project exactly.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

LAYOUTS = {"model": 0, "sample": 1}
ORDERS = ("scan", "image")


def centred_ray_angles(H: int, W: int) -> torch.Tensor:
    """The linear HDL-64E grid with the rays at the cell CENTRES, ``(1,2,H,W)`` [elevation, azimuth] in radians:
    ``el = (1 - (h + 1/2) / H) 28 deg - 25 deg``, ``az = 180 deg - 360 deg (w + 1/2) / W``.  ``synthetic.hdl64e_ray_angles`` (the
    default of ``LiDARUtility``) is the same grid at the cell edges; see the module's note on what that does to a round trip."""
    el = (1 - (torch.arange(H, dtype=torch.float64) + 0.5) / H) * 28.0 - 25.0
    az = 180.0 - 360.0 * (torch.arange(W, dtype=torch.float64) + 0.5) / W
    el, az = torch.meshgrid(el, az, indexing="ij")
    return torch.stack([el, az])[None].deg2rad().float()


def _angles(ray_angles, H: int, W: int) -> torch.Tensor:
    """``(1,2,H,W)`` or ``(2,H,W)`` -> ``(2,H,W)`` float32 tensor (wherever it lives)"""
    a = torch.as_tensor(ray_angles)
    if a.ndim == 4 and a.shape[0] == 1:
        a = a[0]
    if a.ndim != 3 or a.shape[0] != 2 or (H and tuple(a.shape[1:]) != (H, W)):
        want = f"(2,{H},{W})" if H else "(2,H,W)"
        raise ValueError(f"ray_angles must be {want} or (1,{want[1:-1]}) [elevation, azimuth], got {tuple(torch.as_tensor(ray_angles).shape)}")
    return a.detach().float()


def scan_row_start(ray_angles) -> np.ndarray:
    """``(H,)`` int32: per row the largest column whose azimuth is >= 0, ``W - 1`` where no column is -- the column a ring's scan
    order starts from (``W/2`` on the edge grid, ``W/2 - 1`` on the centred grid).  Runs on the host."""
    az = _angles(ray_angles, 0, 0)[1].cpu().numpy()
    W = az.shape[1]
    ok = az >= 0
    last = W - 1 - np.argmax(ok[:, ::-1], axis=1)
    return np.where(ok.any(axis=1), last, W - 1).astype(np.int32)


@torch.no_grad()
def images_to_points(x, lidar_utils=None, *, layout: str = "model", order: str = "scan", keep_min: float | None = None,
                     keep_max: float | None = None, ray_angles=None, return_index: bool = False):
    """A batch of range images -> ``(points, offsets)`` or ``(points, offsets, index)``.

    ``layout="model"``: ``x`` is ``(B,2,H,W)`` in [-1,1], the sampler's output; the points are those of
    ``lidar_utils.postprocess(x)``, bit for bit, computed in the same pass.  ``layout="sample"``: ``x`` is ``(B,5,H,W)``
    [depth, x, y, z, reflectance] (``postprocess``'s output, a ``samples_*.pth`` file, ``project_scans(layout="sample")``); its
    values are copied.  A pixel is kept when ``keep_min < depth < keep_max`` (defaults: the depth window of ``lidar_utils``;
    without ``lidar_utils`` every pixel with a depth > 0) and x, y, z are finite; NaN drops out.

    ``points`` is a ``(total,4)`` float32 ROCm tensor [x, y, z, reflectance], a view of the call's ``(B H W,4)`` buffer; ``offsets``
    a ``(B+1,)`` numpy int64 array (one host read): scan k is ``points[offsets[k]:offsets[k + 1]]``.  ``index`` ``(total,)`` int32:
    the pixel ``h W + w`` of every row inside its image.  ``order``: see the module's text; ``"scan"`` takes the azimuths from
    ``ray_angles`` (``(1,2,H,W)`` or ``(2,H,W)``), by default ``lidar_utils.ray_angles``, which ``layout="model"`` also computes
    the points along.  ``layout="sample"`` with ``order="image"`` needs no ``lidar_utils``.  The same bits on every call."""
    if layout not in LAYOUTS:
        raise ValueError(f"unknown layout {layout!r}: expected one of {sorted(LAYOUTS)}")
    if order not in ORDERS:
        raise ValueError(f"unknown order {order!r}: expected one of {sorted(ORDERS)}")
    channels = 2 if layout == "model" else 5
    if len(x.shape) != 4 or x.shape[1] != channels:
        raise ValueError(f"layout {layout!r} expects (B,{channels},H,W), got {tuple(x.shape)}")
    B, _, H, W = (int(v) for v in x.shape)
    if H < 1 or W < 1:
        raise ValueError(f"images of {H}x{W}: sizes must be >= 1")
    if lidar_utils is None and layout == "model":
        raise ValueError("layout 'model' needs lidar_utils (the depth format, the depth window and the ray angles of the checkpoint)")
    if ray_angles is None and lidar_utils is not None:
        ray_angles = lidar_utils.ray_angles
    if ray_angles is None and order == "scan":
        raise ValueError("order 'scan' needs the azimuths: pass lidar_utils or ray_angles")
    ang = None if ray_angles is None else _angles(ray_angles, H, W)
    keep_min = float((lidar_utils.min_depth if lidar_utils is not None else 0.0) if keep_min is None else keep_min)
    keep_max = float((lidar_utils.max_depth if lidar_utils is not None else float("inf")) if keep_max is None else keep_max)
    if isinstance(x, np.ndarray):
        if not torch.cuda.is_available():
            raise _lib.R2DMError("images_to_points runs as HIP kernels on an MI355X and has no CPU fallback: no ROCm device found")
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to("cuda")
    _lib.require_gpu(x, "x")
    x = _lib.f32c(x)
    dev = x.device
    points = torch.empty(B * H * W, 4, dtype=torch.float32, device=dev)
    index = torch.empty(B * H * W, dtype=torch.int32, device=dev) if return_index else None
    if not B:
        out = (points, np.zeros(1, np.int64))
        return out + (index,) if return_index else out
    L = _lib.lib()
    need = L.r2dm_unproject_scratch_bytes(B, H, W)
    if not need:
        raise ValueError(f"{B} images of {H}x{W}: beyond the limits of r2dm_unproject")
    row_start = torch.from_numpy(scan_row_start(ang)).to(dev) if order == "scan" else None
    ang_dev = ang.to(dev).contiguous() if layout == "model" else None
    fmt = _lib.DEPTH_FORMATS[lidar_utils.depth_format] if lidar_utils is not None else 0
    min_depth, max_depth = (float(lidar_utils.min_depth), float(lidar_utils.max_depth)) if lidar_utils is not None else (0.0, 1.0)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
    scratch = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    base = (-scratch.data_ptr()) % 256  # 256-byte aligned start
    with torch.cuda.device(dev):
        _lib.check(L.r2dm_unproject(_lib.ptr(x), LAYOUTS[layout], _lib.ptr(ang_dev), _lib.ptr(row_start), _lib.ptr(points), _lib.ptr(index),
                                    _lib.ptr(offsets), B, H, W, min_depth, max_depth, fmt, keep_min, keep_max, scratch.data_ptr() + base,
                                    scratch.numel() - base, _lib.stream_ptr(dev)))
    off = offsets.cpu().numpy()  # the one host read
    total = int(off[-1])
    out = (points[:total], off)
    return out + (index[:total],) if return_index else out


def _host_points(points) -> np.ndarray:
    if isinstance(points, torch.Tensor):
        points = points.detach().cpu().numpy()
    points = np.asarray(points)
    if points.ndim != 2 or points.shape[1] != 4:
        raise ValueError(f"expected points (total,4), got {tuple(points.shape)}")
    return np.ascontiguousarray(points, dtype="<f4")


def save_scans(points, offsets, paths) -> None:
    """One Velodyne ``.bin`` per scan: fp32 [x, y, z, reflectance] rows, scan k = ``points[offsets[k]:offsets[k + 1]]`` to
    ``paths[k]``.  The inverse of ``projection.load_scans``."""
    from .projection import _check_offsets

    pts = _host_points(points)
    off = _check_offsets(offsets, len(pts))
    paths = list(paths)
    if len(paths) != off.size - 1:
        raise ValueError(f"{off.size - 1} scans but {len(paths)} paths")
    for k, p in enumerate(paths):
        pts[off[k]:off[k + 1]].tofile(p)


def save_ply(points, path, colors=None) -> None:
    """Binary little-endian PLY of one cloud: float ``x y z intensity`` per vertex and, with ``colors`` ``(total,3)`` uint8, uchar
    ``red green blue``."""
    pts = _host_points(points)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(pts)}"] + [f"property float {n}" for n, _ in fields]
    if colors is not None:
        if isinstance(colors, torch.Tensor):
            colors = colors.detach().cpu().numpy()
        colors = np.asarray(colors)
        if colors.shape != (len(pts), 3) or colors.dtype != np.uint8:
            raise ValueError(f"expected colors ({len(pts)},3) uint8, got {tuple(colors.shape)} {colors.dtype}")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += [f"property uchar {n}" for n in ("red", "green", "blue")]
    rows = np.empty(len(pts), dtype=np.dtype(fields))  # packed: 16 or 19 bytes a vertex
    for k, (n, _) in enumerate(fields[:4]):
        rows[n] = pts[:, k]
    if colors is not None:
        for k, n in enumerate(("red", "green", "blue")):
            rows[n] = colors[:, k]
    with open(path, "wb") as f:
        f.write(("\n".join(header + ["end_header"]) + "\n").encode("ascii"))
        f.write(rows.tobytes())


@torch.no_grad()
def height_colors(points: torch.Tensor, max_depth: float) -> torch.Tensor:
    """``(total,3)`` uint8: the viridis height map of the bird's-eye views (generate.py:51-55: z from -2 m to 0.5 m) of the rows'
    z, on the GPU."""
    from .render import colorize

    z_min, z_max = -2 / max_depth, 0.5 / max_depth
    z = (points[:, 2] / max_depth - z_min) / (z_max - z_min)
    return colorize(z.clamp(0, 1).reshape(1, 1, -1), "viridis")[0, :, 0].T.contiguous()
