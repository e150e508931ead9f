"""The contract of r2dm_amd.pointcloud.images_to_points restated in numpy, on post-processed images: which pixels are kept, in what
order, and what a row holds.  Nothing here computes a coordinate: the planes are gathered, so every comparison is bit for bit."""
import numpy as np


def positions(H, W, row_start=None, order="scan"):
    """(H W,) int64: the pixel ``h W + w`` at every position of a scan.  ``"image"``: row-major.  ``"scan"``: rows top to bottom,
    inside row h the columns fall cyclically from ``row_start[h]``: w = (row_start[h] - p % W) mod W."""
    h, c = np.divmod(np.arange(H * W, dtype=np.int64), W)
    if order == "image":
        return h * W + c
    assert order == "scan"
    rs = np.asarray(row_start, dtype=np.int64)
    assert rs.shape == (H,)
    return h * W + (rs[h] - c) % W


def export(planes, row_start=None, order="scan", keep_min=1.45, keep_max=80.0):
    """``planes`` (B,5,H,W) float32 [depth, x, y, z, reflectance] -> points (total,4) float32 [x, y, z, reflectance], offsets
    (B+1,) int64, index (total,) int32.  Kept: keep_min < depth < keep_max (fp32 comparisons) and x, y, z finite."""
    planes = np.ascontiguousarray(np.asarray(planes), dtype=np.float32)
    B, C, H, W = planes.shape
    assert C == 5
    pix = positions(H, W, row_start, order)
    flat = planes.reshape(B, 5, H * W)
    pts, idx, offsets = [], [], np.zeros(B + 1, np.int64)
    for b in range(B):
        v = flat[b][:, pix]  # (5, HW) in the order of the positions
        with np.errstate(invalid="ignore"):
            keep = (v[0] > np.float32(keep_min)) & (v[0] < np.float32(keep_max)) & np.isfinite(v[1:4]).all(axis=0)
        pts.append(v[1:5, keep].T)
        idx.append(pix[keep])
        offsets[b + 1] = offsets[b] + int(keep.sum())
    points = np.ascontiguousarray(np.concatenate(pts), dtype=np.float32) if B else np.zeros((0, 4), np.float32)
    index = np.concatenate(idx).astype(np.int32) if B else np.zeros(0, np.int32)
    return points, offsets, index
