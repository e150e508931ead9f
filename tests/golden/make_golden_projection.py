#!/usr/bin/env python3
"""Generate tests/golden/projection.npz by running the REAL reference's load_points_as_images on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_projection.py /path/to/reference

The reference's data/kitti_360/kitti_360.py is imported by path; ``numba`` (absent here) is replaced by a stand-in module whose
``jit`` returns the function unchanged, so its scatter runs as plain Python.

Stored per case: ``idx_<case>`` (H,W) int32, the index in the file of the point the reference left in every cell (-1: empty), and
``depth_<case>`` (H,W) float32, its depth plane.  The index is recovered by running the reference on a copy of the cloud whose
reflectance column holds the point's index (the function only carries that column).  The six planes are not stored: the tests
rebuild them from the regenerated points.  The free cloud also stores ``skip_<case>``, the cells left out of the comparison.

The clouds are regenerated from integer-only PCG64 draws by ``make_cloud`` (imported by the tests):
  - centred clouds: every point is built in fp64 from a chosen cell plus a jitter in [0.1, 0.9] of a cell on each axis and rounded
    to fp32, 4 to 8 points per cell, a tenth of the cells empty; depths are multiples of 1/64 m in 0.5 .. 90 m (plus a ring-dependent 1024th under unfolding), distinct
    within a cell; six cells hold a single point whose fp32 depth is exactly 1.45f, 80.0f or one ulp either side.  Unfolding clouds are
    ring-ordered with counter-clockwise azimuth, with H - 3, H, H + 1 or H + 3 rings, one of them starting mid-ring.
  - one free cloud: 60 k points with uniformly random directions (a little beyond the vertical field of view) and depths.
``project_numpy`` is the specification the HIP kernels implement, in numpy: the reference's expressions, the closed form of its
scan-unfolding loop, the nearest point per cell with the lowest index winning a tie.  tests/test_projection_cpu.py holds it to
this file on every case.
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "projection.npz")
MIN_DEPTH, MAX_DEPTH = 1.45, 80.0
EDGE = 1e-3       # of a cell: closer to an edge than this, two math libraries may put a point on either side
SKIP_CAP = 0.01   # of the occupied cells

# name -> (H, W, scan_unfolding, rings, start mid-ring, seed); rings None: the spherical centred cloud; "free": the free cloud
CASES = {
    "sph_8x32": (8, 32, False, None, False, 1),
    "sph_64x1024": (64, 1024, False, None, False, 2),
    "unf_8x32_r5": (8, 32, True, 5, False, 3),
    "unf_8x32_r8": (8, 32, True, 8, False, 4),
    "unf_8x32_r9": (8, 32, True, 9, False, 5),
    "unf_8x32_r11": (8, 32, True, 11, False, 6),
    "unf_8x32_r8_mid": (8, 32, True, 8, True, 7),
    "unf_64x1024_r65": (64, 1024, True, 65, False, 8),
    "free_64x1024": (64, 1024, False, "free", False, 10),
}
SPECIAL = [np.nextafter(np.float32(1.45), np.float32(0)), np.float32(1.45), np.nextafter(np.float32(1.45), np.float32(2)),
           np.nextafter(np.float32(80), np.float32(0)), np.float32(80), np.nextafter(np.float32(80), np.float32(100))]
H_UP, H_DOWN = np.deg2rad(3), np.deg2rad(-25)


def norm32(xyz):
    """np.linalg.norm(float32 (N,3), axis=1): sqrt((x x + y y) + z z), every operation rounded to fp32."""
    s = xyz.astype(np.float32) ** 2
    return np.sqrt((s[:, 0] + s[:, 1]) + s[:, 2], dtype=np.float32)


def _exact_depth_point(phi, theta, target):
    """A point near direction (phi, theta) whose fp32 depth is exactly ``target``: z is moved ulp by ulp."""
    t = np.float64(target)
    x, y = np.float32(t * np.cos(phi) * np.cos(theta)), np.float32(t * np.cos(phi) * np.sin(theta))
    z = np.float32(t * np.sin(phi))
    zs = z + np.arange(-4000, 4001, dtype=np.float64) * np.float64(np.spacing(z))
    zs = zs.astype(np.float32)
    cand = np.stack([np.full_like(zs, x), np.full_like(zs, y), zs], 1)
    hit = np.nonzero(norm32(cand) == target)[0]
    assert len(hit), ("no z gives the depth", target)
    return cand[hit[len(hit) // 2]]


def _cell_points(g, n_cells, sparse=False):
    """Per cell: the number of points (0, or 4..8; sparse: 0..2), then per point a depth (distinct within the cell), two jitters and a
    reflectance."""
    r = g.integers(0, 10, size=n_cells)
    k = r % 3 if sparse else np.where(r == 0, 0, 4 + r % 5)
    n = int(k.sum())
    cell = np.repeat(np.arange(n_cells), k)
    # depths: multiples of 1/64 m in [0.5, 90]; distinct within a cell: 8 disjoint bands per cell, one per point, in shuffled order
    first = np.cumsum(k) - k
    slot = np.arange(n) - first[cell]
    band = (slot + g.integers(0, 8, size=n_cells)[cell]) % 8
    span = (90 * 64 - 32) // 8
    depth = (32 + band * span + g.integers(0, span, size=n)) / 64.0
    jit = 0.1 + 0.8 * g.integers(0, 2**16 + 1, size=(2, n)) / 2.0**16
    refl = g.integers(0, 2**12, size=n) / 2.0**12
    return cell, depth, jit, refl


def _angles(h, jh, w, jw, H, W):
    """elevation and azimuth (fp64) of grid position (h + jh, w + jw): the inverse of kitti_360.py:76-84"""
    phi = (1.0 - (h + jh) / H) * (H_UP - H_DOWN) - abs(H_DOWN)
    theta = -(2.0 * (w + jw) / W - 1.0) * np.pi
    return phi, theta


def _to_points(depth, phi, theta, refl):
    xyz = np.stack([depth * np.cos(phi) * np.cos(theta), depth * np.cos(phi) * np.sin(theta), depth * np.sin(phi)], 1)
    return np.concatenate([xyz, refl[:, None]], 1).astype(np.float32)


def _plant_specials(g, pts, cell, n_cells, angle_of):
    """Six cells get a single point each, with the depths of SPECIAL; returns the points with those cells' other points removed."""
    cells = g.permutation(n_cells)[:len(SPECIAL)]
    keep = ~np.isin(cell, cells)
    extra = []
    for c, t in zip(cells, SPECIAL):
        phi, theta = angle_of(c)
        extra.append(np.append(_exact_depth_point(phi, theta, t), np.float32(0.5)))
    return pts, keep, cells, np.array(extra, np.float32)


def centred_spherical(H, W, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    cell, depth, jit, refl = _cell_points(g, H * W)
    phi, theta = _angles(cell // W, jit[0], cell % W, jit[1], H, W)
    pts = _to_points(depth, phi, theta, refl)
    pts, keep, cells, extra = _plant_specials(g, pts, cell, H * W, lambda c: _angles(c // W, 0.5, c % W, 0.5, H, W))
    return np.concatenate([pts[keep], extra])  # cell by cell: neighbours in the file share a cell (the tests also permute it)


def centred_unfolding(H, W, rings, mid, seed, sparse=False):
    """``rings`` rings in file order, top first; each runs counter-clockwise from azimuth 0+: columns W/2-1 .. 0, W-1 .. W/2.
    ``sparse``: about one point per cell, as a real scan has (64 x 2048: about 130 k points)."""
    g = np.random.Generator(np.random.PCG64(seed))
    cell, depth, jit, refl = _cell_points(g, rings * W, sparse)
    ring, pos = cell // W, cell % W
    w = (W // 2 - 1 - pos) % W
    # counter-clockwise inside a cell too: the column jitter falls along the file
    order = np.lexsort((-jit[1], cell))
    cell, depth, jit, refl, ring, w = cell[order], depth[order], jit[:, order], refl[order], ring[order], w[order]
    depth = depth + (ring % 7) / 1024.0  # rings that share a row (more rings than rows, a scan starting mid-ring) never share a depth
    # the row comes from the sequence, not from the elevation: any elevation will do; rings fall from +2 to -24 degrees
    phi = np.deg2rad(2.0 - 26.0 * (ring + jit[0]) / rings)
    theta = -(2.0 * (w + jit[1]) / W - 1.0) * np.pi
    pts = _to_points(depth, phi, theta, refl)

    def angle_of(c):
        return np.deg2rad(2.0 - 26.0 * (c // W + 0.5) / rings), -(2.0 * ((W // 2 - 1 - c % W) % W + 0.5) / W - 1.0) * np.pi

    pts, keep, cells, extra = _plant_specials(g, pts, cell, rings * W, angle_of)
    # a special point takes its cell's place in the sequence
    out, at = [], np.searchsorted(cell, cells)
    order = np.argsort(at)
    prev = 0
    for a, e in zip(at[order], extra[order]):
        out += [pts[prev:a][keep[prev:a]], e[None]]
        prev = a
    out.append(pts[prev:][keep[prev:]])
    pts = np.concatenate(out)
    if mid:
        s = int(g.integers(len(pts) // (3 * rings), len(pts) // (2 * rings)))  # inside the first ring
        pts = np.concatenate([pts[s:], pts[:s]])
    return pts


def free_cloud(seed, n=60_000):
    g = np.random.Generator(np.random.PCG64(seed))
    k = g.integers(0, 2**24, size=(4, n)) / 2.0**24
    phi, theta = np.deg2rad(-27.0 + 32.0 * k[0]), (2.0 * k[1] - 1.0) * np.pi
    return _to_points(0.5 + 89.5 * k[2], phi, theta, k[3])


def make_cloud(name):
    H, W, unfolding, rings, mid, seed = CASES[name]
    if rings == "free":
        return free_cloud(seed)
    return centred_unfolding(H, W, rings, mid, seed) if unfolding else centred_spherical(H, W, seed)


# ---- the specification in numpy ------------------------------------------------------------------
def unfolding_rows(points, H):
    """The closed form of kitti_360.py:52-74 (scan unfolding)."""
    x, y = points[:, 0], points[:, 1]
    quad = np.zeros(len(points), np.int32)
    quad[(x < 0) & (y >= 0)] = 1
    quad[(x < 0) & (y < 0)] = 2
    quad[(x >= 0) & (y < 0)] = 3
    delim = (np.roll(quad, 1) - quad) == 3
    seg, D = np.cumsum(delim), int(delim.sum())
    r = H - 1 - (D - seg)
    return np.where(seg == 0, 0, np.where(r >= 0, r, np.where(r == -1, H - 1, 0))).astype(np.int64)


def grid_of(points, H, W, scan_unfolding):
    """(row, column, depth, usable) per point; the reference's expressions in its precisions."""
    with np.errstate(all="ignore"):
        depth = norm32(points[:, :3])
        ok = np.isfinite(depth) & (depth > 0)
        if scan_unfolding:
            h = unfolding_rows(points, H)
        else:
            elevation = np.arcsin(points[:, 2] / depth) + abs(H_DOWN)
            gh = np.floor((1 - elevation / (H_UP - H_DOWN)) * H)
            h = np.clip(np.nan_to_num(gh, nan=0.0), 0, H - 1).astype(np.int64)
        azimuth = -np.arctan2(points[:, 1], points[:, 0])
        gw = np.floor((azimuth / np.pi + 1) / 2 % 1 * W)
        w = np.clip(np.nan_to_num(gw, nan=0.0), 0, W - 1).astype(np.int64)
    return h, w, depth, ok


def winners(h, w, depth, ok, H, W):
    """(H,W) int32: per cell the nearest usable point, the lowest index among equal depths; -1 where there is none."""
    idx = np.nonzero(ok)[0]
    cell = h[idx] * W + w[idx]
    order = np.lexsort((idx, depth[idx], cell))
    cell, idx = cell[order], idx[order]
    first = np.ones(len(cell), bool)
    first[1:] = cell[1:] != cell[:-1]
    out = np.full(H * W, -1, np.int32)
    out[cell[first]] = idx[first]
    return out.reshape(H, W)


def planes_of(points, idx, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, apply_mask=False):
    """(6,H,W) float32 [x, y, z, reflectance, depth, mask] of the winners ``idx`` (H,W)."""
    p = points[np.maximum(idx, 0)]
    depth = norm32(p.reshape(-1, 4)[:, :3]).reshape(idx.shape)
    mask = ((depth >= np.float32(min_depth)) & (depth <= np.float32(max_depth))).astype(np.float32)
    out = np.concatenate([np.moveaxis(p, -1, 0), depth[None], mask[None]]).astype(np.float32)
    out = np.where(idx >= 0, out, np.float32(0))
    if apply_mask:
        with np.errstate(invalid="ignore"):
            out *= out[[5]]
    return out


def project_numpy(points, H, W, scan_unfolding, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, apply_mask=False):
    """One scan -> (winner index (H,W), planes (6,H,W))."""
    idx = winners(*grid_of(points, H, W, scan_unfolding), H, W)
    return idx, planes_of(points, idx, min_depth, max_depth, apply_mask)


def edge_cells(points, H, W):
    """(H,W) bool: the cells a point within EDGE of a cell edge falls in, and the cells across that edge (fp64 evaluation of the
    spherical formulas)."""
    p = points.astype(np.float64)
    d = np.sqrt((p[:, :3] ** 2).sum(1))
    gh = (1 - (np.arcsin(p[:, 2] / d) + abs(H_DOWN)) / (H_UP - H_DOWN)) * H
    gw = ((-np.arctan2(p[:, 1], p[:, 0])) / np.pi + 1) / 2 % 1 * W
    h, w = np.floor(gh), np.floor(gw)
    dh = np.where(gh - h < EDGE, -1, np.where(h + 1 - gh < EDGE, 1, 0))
    dw = np.where(gw - w < EDGE, -1, np.where(w + 1 - gw < EDGE, 1, 0))
    near = np.nonzero((dh != 0) | (dw != 0))[0]
    skip = np.zeros((H, W), bool)
    for a in (0, 1):
        for b in (0, 1):
            hh = np.clip(h[near] + a * dh[near], 0, H - 1).astype(np.int64)
            ww = ((w[near] + b * dw[near]) % W).astype(np.int64)
            skip[hh, np.clip(ww, 0, W - 1)] = True
    return skip, (np.clip(h, 0, H - 1).astype(np.int64), np.clip(w, 0, W - 1).astype(np.int64))


# ---- the reference -------------------------------------------------------------------------------
def import_reference(reference):
    import importlib.util

    if "numba" not in sys.modules:
        stub = types.ModuleType("numba")
        stub.jit = lambda *a, **k: (lambda f: f)
        sys.modules["numba"] = stub
    spec = importlib.util.spec_from_file_location("ref_kitti_360", os.path.join(reference, "data", "kitti_360", "kitti_360.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_reference(mod, points, H, W, scan_unfolding):
    """(winner index, depth plane) of the reference on ``points``, the index carried through the reflectance column."""
    assert len(points) < 2**24
    tagged = points.copy()
    tagged[:, 3] = np.arange(len(points), dtype=np.float32)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "scan.bin")
        tagged.tofile(path)
        img = mod.load_points_as_images(path, scan_unfolding=scan_unfolding, H=H, W=W)
    assert img.shape == (H, W, 6) and img.dtype == np.float32
    occupied = img[..., 4] > 0
    idx = np.where(occupied, img[..., 3], -1).astype(np.int32)
    # the whole payload is the winner's row
    want = planes_of(tagged, idx)
    assert np.array_equal(np.moveaxis(img, -1, 0).view(np.uint32), want.view(np.uint32))
    return idx, img[..., 4].copy()


def main(reference):
    mod = import_reference(reference)
    out = {}
    for name, (H, W, unfolding, rings, mid, seed) in CASES.items():
        pts = make_cloud(name)
        idx, depth = run_reference(mod, pts, H, W, unfolding)
        h, w, d32, ok = grid_of(pts, H, W, unfolding)
        assert ok.all()
        # no two points of one cell share a depth: the reference's result does not depend on its unstable argsort
        cd = np.stack([h * W + w, d32.view(np.uint32).astype(np.int64)], 1)
        assert len(np.unique(cd, axis=0)) == len(pts), name
        mine = winners(h, w, d32, ok, H, W)
        occupied = idx >= 0
        if rings == "free":
            skip, (h64, w64) = edge_cells(pts, H, W)
            ideal = winners(h64, w64, d32, ok, H, W)
            assert not ((ideal != idx) & ~skip).any(), "the reference leaves the fp64 grid outside the left-out cells"
            assert not ((mine != idx) & ~skip).any()
            frac = (skip & (occupied | (ideal >= 0))).sum() / occupied.sum()
            print(f"{name}: {len(pts)} points, {occupied.sum()} occupied cells, {skip.sum()} cells left out ({frac:.2%} of the occupied), "
                  f"reference != fp64 grid in {(ideal != idx).sum()} cells")
            assert frac <= SKIP_CAP, frac
            out[f"skip_{name}"] = np.packbits(skip)
        else:
            assert np.array_equal(mine, idx), name
            dmask = (depth >= np.float32(MIN_DEPTH)) & (depth <= np.float32(MAX_DEPTH))
            got = {float(t): int(((depth == t) & occupied).sum()) for t in SPECIAL}
            if not unfolding or (rings <= H and not mid):  # (where rings share a row a planted point may lose its cell to another ring)
                assert all(v >= 1 for v in got.values()), got
            D = int(((np.roll(pts[:, 0] >= 0, 1) & np.roll(pts[:, 1] < 0, 1)) & (pts[:, 0] >= 0) & (pts[:, 1] >= 0)).sum()) if unfolding else 0
            print(f"{name}: {len(pts)} points, {occupied.sum()} of {H * W} cells occupied, {int((occupied & ~dmask).sum())} winners outside "
                  f"the depth window, {D} delimiters")
        out[f"idx_{name}"], out[f"depth_{name}"] = idx, depth
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 1_000_000


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
