#!/usr/bin/env python3
"""Generate tests/golden/pointcloud.npz: what the REAL reference's load_points_as_images makes of clouds exported in scan order.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pointcloud.py /path/to/reference

Two 8 x 64 post-processed images [depth, x, y, z, reflectance] along rays at the cell centres -- one dense, one with a random 60 %
of its pixels valid (the others all zero, as a masked image holds them) -- are exported in scan order by the contract's numpy
restatement (tests/pointcloud_oracle.py), written as Velodyne ``.bin`` files and read back by the reference (imported as
make_golden_projection.py imports it), with scan unfolding and with the spherical projection, at H = 8, W = 64.

Stored per case (``dense``, ``sparse``): ``src_<case>`` (5,8,64) the source planes, ``pts_<case>`` (N,4) the exported rows the
reference read, ``unfolding_<case>`` and ``spherical_<case>`` (6,8,64) the reference's [x, y, z, reflectance, depth, mask] images.
The tests import ``valid_mask`` and ``source_planes`` for the same images at other sizes."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_projection as GP  # noqa: E402  (import_reference)
import pointcloud_oracle as PO  # noqa: E402

OUT = os.path.join(HERE, "pointcloud.npz")
H, W = 8, 64
MIN_DEPTH, MAX_DEPTH = 1.45, 80.0
SEED = 31
CASES = {"dense": 1.0, "sparse": 0.6}


def valid_mask(H, W, fraction, seed=SEED):
    """(H,W) bool from integer PCG64 draws: a pixel is valid with probability ``fraction``."""
    g = np.random.Generator(np.random.PCG64(seed))
    return g.integers(0, 10, size=(H, W)) < round(fraction * 10)


def centred_angles(H, W):
    """Elevation and azimuth (H,W) in radians, fp64, rays at the cell centres of the linear HDL-64E grid."""
    el = np.deg2rad((1 - (np.arange(H) + 0.5) / H) * 28.0 - 25.0)
    az = np.deg2rad(180.0 - 360.0 * (np.arange(W) + 0.5) / W)
    return np.meshgrid(el, az, indexing="ij")


def source_planes(H, W, fraction, seed=SEED):
    """(5,H,W) float32 [depth, x, y, z, reflectance]: depths are multiples of 1/64 m in [2, 70), points computed in fp64 and rounded
    once; invalid pixels hold zeros."""
    g = np.random.Generator(np.random.PCG64(seed + 1))
    depth = g.integers(2 * 64, 70 * 64, size=(H, W)) / 64.0
    refl = g.integers(0, 2**12, size=(H, W)) / 2.0**12
    el, az = centred_angles(H, W)
    planes = np.stack([depth, depth * np.cos(el) * np.cos(az), depth * np.cos(el) * np.sin(az), depth * np.sin(el), refl])
    return np.where(valid_mask(H, W, fraction, seed), planes, 0.0).astype(np.float32)  # (+0: what an empty cell of the projection holds)


def row_start_of(az):
    """The contract's rule: per row the largest column whose azimuth is >= 0, W - 1 where there is none."""
    ok = az >= 0
    return np.where(ok.any(1), az.shape[1] - 1 - np.argmax(ok[:, ::-1], axis=1), az.shape[1] - 1).astype(np.int32)


def main(reference):
    mod = GP.import_reference(reference)
    out = {}
    row_start = row_start_of(centred_angles(H, W)[1])
    assert (row_start == W // 2 - 1).all()
    for name, fraction in CASES.items():
        src = source_planes(H, W, fraction)
        pts, off, idx = PO.export(src[None], row_start, "scan", MIN_DEPTH, MAX_DEPTH)
        assert off[1] == (src[0] > 0).sum() == len(pts)
        out[f"src_{name}"], out[f"pts_{name}"] = src, pts
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "scan.bin")
            pts.tofile(path)
            for mode, unfolding in (("unfolding", True), ("spherical", False)):
                img = mod.load_points_as_images(path, scan_unfolding=unfolding, H=H, W=W, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH)
                assert img.shape == (H, W, 6) and img.dtype == np.float32
                out[f"{mode}_{name}"] = np.ascontiguousarray(np.moveaxis(img, -1, 0))
                same = np.array_equal(out[f"{mode}_{name}"][:4].view(np.uint32), src[[1, 2, 3, 4]].view(np.uint32))
                rel = np.abs(out[f"{mode}_{name}"][4].astype(np.float64) - src[0]).max() / 70.0
                print(f"{name} {mode}: {len(pts)} points, x y z reflectance planes identical: {same}, depth off by at most {rel:.2e} of 70 m")
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 1_000_000


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
