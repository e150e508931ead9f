"""Rendering of the reference's ``generate.py`` (utils/render.py) as HIP kernels: colour-mapped range images and the
bird's-eye view (BEV) of a point cloud -- an oblique perspective projection, splatted bilinearly with a depth weight.

Same names and signatures as the reference module; inputs are ROCm tensors and nothing falls back to the CPU.

- ``colorize`` is bit-identical to the reference.
- ``bilinear_rasterizer`` / ``render_point_clouds`` evaluate the reference's fp32 expressions per point (one rounding per
  operation) and sum the terms in 64-bit fixed point: the image is the same bits on every call and for every order of the points,
  and closer to the exact sum than an fp32 ``scatter_add_``.  A point with a non-finite coordinate adds nothing (the reference
  adds NaN to a corner pixel).
- ``render_frames`` is generate.py's ``render()`` fused: frame in, colour image and BEV out; no xyz / colour tensor in between.
- ``make_grid`` / ``save_png`` replace torchvision's ``save_image`` with torch and the standard library.

The projection restates kornia's ``project_points`` (K = diag(f, f, 1), cx = cy = 0.5) from its documentation.
"""
from __future__ import annotations

import ctypes
import math
import struct
import zlib

import numpy as np
import torch

from . import _lib

_SCRATCH_CAP = 1 << 30  # bytes of accumulators taken at a time
_LUTS: dict = {}


# ---- colour maps ---------------------------------------------------------------------------------
def colormap_lut(cmap="turbo") -> torch.Tensor:
    """(256,3) fp32 table on the CPU: a tensor as given, ``cmap(np.linspace(0, 1, 256))[:, :3]`` of a callable (the reference's
    use), or matplotlib's colour map of that name."""
    if isinstance(cmap, torch.Tensor):
        if tuple(cmap.shape) != (256, 3):
            raise ValueError(f"a colour table is (256,3), got {tuple(cmap.shape)}")
        return cmap.detach().to(torch.float32)
    if isinstance(cmap, str):
        if cmap not in _LUTS:
            try:
                import matplotlib.cm as cm
            except ImportError as e:
                raise ImportError(f"the colour map {cmap!r} is looked up in matplotlib, which is not installed; "
                                  "pass a (256,3) tensor or a callable instead") from e
            if not hasattr(cm, cmap):
                raise ValueError(f"matplotlib has no colour map {cmap!r}")
            _LUTS[cmap] = colormap_lut(getattr(cm, cmap))
        return _LUTS[cmap]
    if callable(cmap):
        return torch.from_numpy(np.asarray(cmap(np.linspace(0, 1, 256)))[:, :3]).to(torch.float32)
    raise TypeError(f"cmap must be a (256,3) tensor, a callable or a name, got {type(cmap).__name__}")


def _device_lut(cmap, device) -> torch.Tensor:
    return colormap_lut(cmap).to(device).contiguous()


@torch.no_grad()
def colorize(tensor: torch.Tensor, cmap="turbo") -> torch.Tensor:
    """utils/render.py:239-247: ``(B,1,H,W)`` or ``(B,H,W)`` in [0,1] -> uint8 ``(B,3,H,W)``."""
    _lib.require_gpu(tensor, "tensor")
    x = tensor.squeeze(1) if tensor.ndim == 4 else tensor
    if x.ndim != 3:
        raise ValueError(f"expected (B,1,H,W) or (B,H,W), got {tuple(tensor.shape)}")
    x = _lib.f32c(x)
    B, H, W = x.shape
    out = torch.empty(B, 3, H, W, dtype=torch.uint8, device=x.device)
    if x.numel():
        lut = _device_lut(cmap, x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().r2dm_colorize(_lib.ptr(x), _lib.ptr(lut), _lib.ptr(out), B, H * W, _lib.stream_ptr(x.device)))
    return out


# SemanticKITTI's 20 training labels in RGB (the reference's make_semantickitti_cmap; 0 unlabeled, 1 car, ... 19 traffic-sign)
LABEL_COLORS = (
    (0, 0, 0), (100, 150, 245), (100, 230, 245), (30, 60, 150), (80, 30, 180), (0, 0, 255), (255, 30, 30), (255, 40, 200), (150, 30, 90),
    (255, 0, 255), (255, 150, 255), (75, 0, 75), (175, 0, 75), (255, 200, 0), (255, 120, 50), (0, 175, 0), (135, 60, 0), (150, 240, 80),
    (255, 240, 150), (255, 0, 0))


def label_lut() -> torch.Tensor:
    """The (256,3) table ``colorize`` needs for ``colorize(labels / 19, label_lut())``: the reference samples its 20-colour
    ListedColormap at ``linspace(0, 1, 256)``, entry i being colour ``floor(i / 255 * 20)`` (the last one 19)."""
    if "labels" not in _LUTS:
        index = np.minimum((np.linspace(0, 1, 256) * len(LABEL_COLORS)).astype(np.int64), len(LABEL_COLORS) - 1)
        _LUTS["labels"] = torch.tensor(LABEL_COLORS, dtype=torch.float32)[torch.from_numpy(index)] / 255
    return _LUTS["labels"]


def colorize_labels(labels: torch.Tensor) -> torch.Tensor:
    """completion_demo.py:138: int ``(B,1,H,W)`` labels 0 .. 19 -> uint8 ``(B,3,H,W)`` in SemanticKITTI's colours."""
    return colorize(labels.float() / (len(LABEL_COLORS) - 1), label_lut())


# ---- splat ---------------------------------------------------------------------------------------
def _scratch(nbytes: int, device):
    buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
    base = (-buf.data_ptr()) % 256  # 256-byte aligned start
    return buf, buf.data_ptr() + base, buf.numel() - base


def _rasterize(coords, values, H, W, ratio):
    L = _lib.lib()
    B, N, C = values.shape
    out = torch.empty(B, 3 if ratio else C, H, W, dtype=torch.float32, device=values.device)
    if not B:
        return out
    if not N:
        return out.zero_()
    per = L.r2dm_rasterize_scratch_bytes(1, C, H, W)
    step = max(1, min(B, 65535, _SCRATCH_CAP // per))
    buf, sptr, sbytes = _scratch(L.r2dm_rasterize_scratch_bytes(step, C, H, W), values.device)
    with torch.cuda.device(values.device):
        for b0 in range(0, B, step):  # (each image takes its scale from the values of its own chunk)
            nb = min(step, B - b0)
            _lib.check(L.r2dm_bilinear_rasterize(_lib.ptr(coords[b0:]), _lib.ptr(values[b0:]), _lib.ptr(out[b0:]), nb, N, C, H, W, sptr, sbytes,
                                                 int(ratio), _lib.stream_ptr(values.device)))
    return out


@torch.no_grad()
def bilinear_rasterizer(coords: torch.Tensor, values: torch.Tensor, out_shape) -> torch.Tensor:
    """utils/render.py:83-142: ``coords`` (B,N,2) as [h, w], ``values`` (B,N,C) -> (B,C,H,W)."""
    _lib.require_gpu(coords, "coords")
    _lib.require_gpu(values, "values")
    if coords.ndim != 3 or coords.shape[2] != 2 or values.ndim != 3 or values.shape[:2] != coords.shape[:2] or values.shape[2] < 1:
        raise ValueError(f"expected coords (B,N,2) and values (B,N,C), got {tuple(coords.shape)} and {tuple(values.shape)}")
    H, W = (int(v) for v in out_shape)
    if H < 1 or W < 1:
        raise ValueError(f"empty image {out_shape}")
    return _rasterize(_lib.f32c(coords), _lib.f32c(values), H, W, False)


def _view(R, t, focal_length):
    """12 host floats: R row-major (identity if None), then t (zeros if None)."""
    R = torch.eye(3) if R is None else R.detach().to("cpu", torch.float32).reshape(-1, 3, 3)
    t = torch.zeros(3) if t is None else t.detach().to("cpu", torch.float32).reshape(-1, 3)
    if R.ndim == 3:
        if R.shape[0] != 1:
            raise ValueError("one view (R of shape (1,3,3) or (3,3)) for the whole batch")
        R = R[0]
    if t.ndim == 2:
        if t.shape[0] != 1:
            raise ValueError("one view (t of shape (1,3) or (3,)) for the whole batch")
        t = t[0]
    return (ctypes.c_float * 12)(*R.flatten().tolist(), *t.tolist())


@torch.no_grad()
def render_point_clouds(points: torch.Tensor, colors: torch.Tensor | None = None, size: int = 800, R: torch.Tensor | None = None,
                        t: torch.Tensor | None = None, focal_length: float = 1.0) -> torch.Tensor:
    """utils/render.py:32-80: ``points`` (B,N,3), ``colors`` (B,N,3) or ones -> (B,3,size,size)."""
    _lib.require_gpu(points, "points")
    if points.ndim != 3 or points.shape[2] != 3:
        raise ValueError(f"expected points (B,N,3), got {tuple(points.shape)}")
    if colors is not None:
        _lib.require_gpu(colors, "colors")
        if colors.shape != points.shape:
            raise ValueError(f"colors {tuple(colors.shape)} do not match points {tuple(points.shape)}")
        colors = _lib.f32c(colors)
    size = int(size)
    if size < 1:
        raise ValueError(f"size {size}")
    points = _lib.f32c(points)
    B, N, _ = points.shape
    uv = torch.empty(B, N, 2, dtype=torch.float32, device=points.device)
    vals = torch.empty(B, N, 4, dtype=torch.float32, device=points.device)
    if B and N:
        with torch.cuda.device(points.device):
            _lib.check(_lib.lib().r2dm_project_points(_lib.ptr(points), _lib.ptr(colors), _view(R, t, focal_length), float(focal_length), size,
                                                      _lib.ptr(uv), _lib.ptr(vals), B * N, _lib.stream_ptr(points.device)))
    return _rasterize(uv, vals, size, size, True)


def make_Rt(roll: float = 0.0, pitch: float = 0.0, yaw: float = 0.0, x: float = 0.0, y: float = 0.0, z: float = 0.0, device="cpu"):
    """utils/render.py:9-29: R = A(0,0,yaw) A(0,pitch,0) A(roll,0,0) with A the rotation matrix of an axis-angle vector (Rodrigues),
    t = [[x, y, z]]; evaluated on the host in fp64, returned as fp32 (1,3,3) and (1,3)."""

    def rodrigues(v):
        v = np.asarray(v, np.float64)
        theta = float(np.linalg.norm(v))
        if theta == 0.0:
            return np.eye(3)
        k = v / theta
        K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
        return np.eye(3) + math.sin(theta) * K + (1.0 - math.cos(theta)) * (K @ K)

    R = rodrigues([0.0, 0.0, yaw]) @ rodrigues([0.0, pitch, 0.0]) @ rodrigues([roll, 0.0, 0.0])
    return (torch.from_numpy(R).to(torch.float32)[None].to(device), torch.tensor([[x, y, z]], dtype=torch.float64).to(torch.float32).to(device))


@torch.no_grad()
def render_frames(x: torch.Tensor, lidar_utils, size: int = 800, scratch_frames: int | None = None):
    """generate.py:44-59 in one pass.  ``x`` (N,2,H,W) as generate.py leaves it (both channels in [0,1], the depth divided by
    ``max_depth``) -> ``img`` (N,3,2H,W), the turbo map of the two channels stacked vertically, and ``bev`` (N,3,size,size), the
    view of generate.py (pitch pi/3, yaw pi/4, z 0.8) coloured by height.  ``scratch_frames`` bounds the frames accumulated at a
    time (default: 1 GiB of accumulators)."""
    _lib.require_gpu(x, "x")
    if x.ndim != 4 or x.shape[1] != 2 or tuple(x.shape[2:]) != tuple(lidar_utils.ray_angles.shape[2:]):
        raise ValueError(f"expected (N,2,{','.join(map(str, lidar_utils.ray_angles.shape[2:]))}) frames, got {tuple(x.shape)}")
    size = int(size)
    if size < 1:
        raise ValueError(f"size {size}")
    L = _lib.lib()
    x = _lib.f32c(x)
    N, _, H, W = x.shape
    img = torch.empty(N, 3, 2 * H, W, dtype=torch.float32, device=x.device)
    bev = torch.empty(N, 3, size, size, dtype=torch.float32, device=x.device)
    if not N:
        return img, bev
    trig = ray_trig(lidar_utils, x.device)
    turbo, viridis = _device_lut("turbo", x.device), _device_lut("viridis", x.device)
    R, t = make_Rt(pitch=math.pi / 3, yaw=math.pi / 4, z=0.8)
    per = L.r2dm_render_frames_scratch_bytes(1, size)
    frames = max(1, min(N, _SCRATCH_CAP // per)) if scratch_frames is None else int(scratch_frames)
    if frames < 1:
        raise ValueError(f"scratch_frames {scratch_frames}")
    buf, sptr, _ = _scratch(frames * per, x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.r2dm_render_frames(_lib.ptr(x), _lib.ptr(trig), _lib.ptr(turbo), _lib.ptr(viridis), _lib.ptr(img), _lib.ptr(bev), N, H, W, size,
                                        float(lidar_utils.min_depth), float(lidar_utils.max_depth), _view(R, t, 1.0), 1.0, sptr, frames * per,
                                        _lib.stream_ptr(x.device)))
    return img, bev


# ---- surface normals -----------------------------------------------------------------------------
NORMAL_MODES = {"closest": 0, "mean": 1}
_NORMAL_MAX_D = 8


def _normal_args(d, mode, W):
    if mode not in NORMAL_MODES:
        raise NotImplementedError(mode)
    d = int(d)
    if not 1 <= d <= _NORMAL_MAX_D or d > W:
        raise ValueError(f"the neighbour distance d must be in [1, min({_NORMAL_MAX_D}, width {W})], got {d}")
    return d, NORMAL_MODES[mode]


@torch.no_grad()
def estimate_surface_normal(points: torch.Tensor, d: int = 2, mode: str = "closest") -> torch.Tensor:
    """utils/render.py:145-236: coordinated points ``(B,3,H,W)`` -> unit normals ``(B,3,H,W)`` from the cross product of two
    neighbours at distance ``d`` (rows replicate, columns wrap): the pair of the eight with the smallest summed distance to the
    pixel (``"closest"``) or the mean over the eight pairs (``"mean"``).  One launch; the bits are those of the written-out fp32
    contract in include/r2dm_hip.h."""
    _lib.require_gpu(points, "points")
    if points.ndim != 4 or points.shape[1] != 3 or points.shape[2] < 1 or points.shape[3] < 1:
        raise ValueError(f"expected (B,3,H,W), got {tuple(points.shape)}")
    B, _, H, W = points.shape
    d, mode = _normal_args(d, mode, W)
    points = _lib.f32c(points)
    out = torch.empty_like(points)
    if B:
        with torch.cuda.device(points.device):
            _lib.check(_lib.lib().r2dm_surface_normals(_lib.ptr(points), _lib.ptr(out), B, H, W, d, mode, _lib.stream_ptr(points.device)))
    return out


def ray_trig(lidar_utils, device) -> torch.Tensor:
    """(4,H,W) fp32: cos / sin of the elevation, cos / sin of the azimuth of ``lidar_utils.ray_angles``, taken on ``device``."""
    ang = lidar_utils.ray_angles[0].to(device, torch.float32)
    return torch.stack([ang[0].cos(), ang[0].sin(), ang[1].cos(), ang[1].sin()]).contiguous()


@torch.no_grad()
def render_normals(metric: torch.Tensor, lidar_utils, size: int = 800, d: int = 2, mode: str = "closest", R: torch.Tensor | None = None,
                   t=(0.0, 0.0, 1.0), focal_length: float = 1.0, scratch_frames: int | None = None, trig: torch.Tensor | None = None,
                   with_colors: bool = True):
    """train.py:227-239 in one pass.  ``metric`` (B,1,H,W), the depth in metres -> ``colors`` (B,3,H,W), the surface normals of
    ``to_xyz(metric) / max_depth * mask`` as ``(-n + 1) / 2``, and ``bev`` (B,3,size,size), that cloud in those colours under the view
    ``R`` / ``t`` (default: train.py's, no rotation and t = [0, 0, 1]).  ``trig`` replaces ``ray_trig(lidar_utils)``;
    ``scratch_frames`` bounds the frames accumulated at a time; ``with_colors=False`` returns ``(None, bev)``."""
    _lib.require_gpu(metric, "metric")
    if metric.ndim != 4 or metric.shape[1] != 1 or tuple(metric.shape[2:]) != tuple(lidar_utils.ray_angles.shape[2:]):
        raise ValueError(f"expected (B,1,{','.join(map(str, lidar_utils.ray_angles.shape[2:]))}) depths, got {tuple(metric.shape)}")
    size = int(size)
    if size < 1:
        raise ValueError(f"size {size}")
    L = _lib.lib()
    metric = _lib.f32c(metric)
    B, _, H, W = metric.shape
    d, mode = _normal_args(d, mode, W)
    if trig is None:
        trig = ray_trig(lidar_utils, metric.device)
    else:
        _lib.require_gpu(trig, "trig")
        if tuple(trig.shape) != (4, H, W):
            raise ValueError(f"expected trig (4,{H},{W}), got {tuple(trig.shape)}")
        trig = _lib.f32c(trig)
    colors = torch.empty(B, 3, H, W, dtype=torch.float32, device=metric.device) if with_colors else None
    bev = torch.empty(B, 3, size, size, dtype=torch.float32, device=metric.device)
    if not B:
        return colors, bev
    if t is not None and not isinstance(t, torch.Tensor):
        t = torch.tensor(t, dtype=torch.float32)
    per = L.r2dm_normal_frames_scratch_bytes(1, size)
    frames = max(1, min(B, _SCRATCH_CAP // per)) if scratch_frames is None else int(scratch_frames)
    if frames < 1:
        raise ValueError(f"scratch_frames {scratch_frames}")
    buf, sptr, _ = _scratch(frames * per, metric.device)
    with torch.cuda.device(metric.device):
        _lib.check(L.r2dm_normal_frames(_lib.ptr(metric), _lib.ptr(trig), _lib.ptr(colors), _lib.ptr(bev), B, H, W, size,
                                        float(lidar_utils.min_depth), float(lidar_utils.max_depth), d, mode, _view(R, t, focal_length),
                                        float(focal_length), sptr, frames * per, _lib.stream_ptr(metric.device)))
    return colors, bev


@torch.no_grad()
def log_images(image: torch.Tensor, lidar_utils, channels=(1, 1), tag: str = "name", size: int = 800) -> dict:
    """train.py:221-245: the panels the reference's training monitor logs for a normalised ``(B,C,H,W)`` batch in [-1,1], ``channels``
    = (depth channels, reflectance channels), as uint8 ``(B,3,.,.)`` images: ``{tag}/depth`` (turbo), ``{tag}/depth/orig`` (turbo of the
    metric depth / max_depth), ``{tag}/bev`` (the bird's-eye view coloured by surface normal), ``{tag}/mask`` (binary_r) and
    ``{tag}/reflectance`` (plasma).  A key is present only when its channel is."""
    _lib.require_gpu(image, "image")
    channels = tuple(int(c) for c in channels)
    if image.ndim != 4 or len(channels) != 2 or min(channels) < 0 or max(channels) > 1 or image.shape[1] != sum(channels):
        raise ValueError(f"expected (B,{sum(channels)},H,W) for channels {channels} (0 or 1 each), got {tuple(image.shape)}")
    image = lidar_utils.denormalize(image)
    depth, rflct = torch.split(image, channels, dim=1)
    out = {}
    if depth.numel() > 0:
        out[f"{tag}/depth"] = colorize(depth)
        metric = lidar_utils.revert_depth(depth)
        mask = (metric > lidar_utils.min_depth) & (metric < lidar_utils.max_depth)
        out[f"{tag}/depth/orig"] = colorize(metric / lidar_utils.max_depth)
        _, bev = render_normals(metric, lidar_utils, size=size, with_colors=False)
        out[f"{tag}/bev"] = bev.mul(255).clamp(0, 255).byte()
    if rflct.numel() > 0:
        out[f"{tag}/reflectance"] = colorize(rflct, "plasma")
    if depth.numel() > 0:
        out[f"{tag}/mask"] = colorize(mask.float(), "binary_r")
    return out


# ---- image files ---------------------------------------------------------------------------------
def make_grid(images: torch.Tensor, nrow: int = 8, padding: int = 2, pad_value: float = 0.0) -> torch.Tensor:
    """torchvision.utils.make_grid for a (B,3,H,W) batch: ``nrow`` images per row, ``padding`` pixels of ``pad_value`` around every
    cell; a batch of one is returned as it is."""
    if images.ndim != 4:
        raise ValueError(f"expected (B,C,H,W), got {tuple(images.shape)}")
    B, C, H, W = images.shape
    if B == 1:
        return images[0]
    xmaps = min(int(nrow), B)
    ymaps = -(-B // xmaps)
    h, w = H + padding, W + padding
    grid = images.new_full((C, h * ymaps + padding, w * xmaps + padding), pad_value)
    for k in range(B):
        r, c = divmod(k, xmaps)
        grid[:, r * h + padding:r * h + padding + H, c * w + padding:c * w + padding + W] = images[k]
    return grid


def save_png(image: torch.Tensor, path) -> None:
    """An 8-bit RGB PNG of a (3,H,W) image: uint8 as it is, float in [0,1] as trunc(clamp(x 255 + 0.5, 0, 255)) (torchvision's
    save_image).  zlib and struct only."""
    if image.ndim != 3 or image.shape[0] != 3:
        raise ValueError(f"expected (3,H,W), got {tuple(image.shape)}")
    if image.dtype != torch.uint8:
        image = image.detach().float().mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)
    rgb = image.permute(1, 2, 0).contiguous().cpu().numpy()
    H, W, _ = rgb.shape
    rows = np.concatenate([np.zeros((H, 1), np.uint8), rgb.reshape(H, W * 3)], axis=1)  # filter type 0 in front of every row

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))
