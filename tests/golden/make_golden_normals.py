#!/usr/bin/env python3
"""Generate tests/golden/normals.npz by running the REAL reference's ``estimate_surface_normal`` (utils/render.py) and the BEV of its
training monitor (train.py:227-239) on the CPU, in fp32 and in fp64.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_normals.py /path/to/reference

The reference module imports kornia at the top: the stand-in of make_golden_render.py is installed first (only the BEV uses it).  The
reference's rasteriser allocates its image in the default dtype: the fp64 BEV runs under ``torch.set_default_dtype(torch.float64)``.

Scenes (``depth_scene``, integer draws only): per row, segments of 8 - 47 columns with a base depth in [3, 60) m on a 2^-10 grid and a
slope of at most 2^-6 m per column; a row is the row above with probability 3/4; noise integers(-41, 42) / 2^12 (about +-1 cm); 10 % of
the pixels are 0.  The points are ``LiDARUtility.to_xyz(depth) / 80 * mask`` of the reference (1.45 m .. 80 m).

Contents (data only), for every case of ``CASES``, mode in ("closest", "mean") and d in (1, 2):
  - stored cases: ``depth_*`` (B,1,H,W), ``trig_*`` (4,H,W) = cos / sin of the reference's ray angles as its to_xyz takes them,
    ``xyz_*`` (B,3,H,W), and the reference's normals ``n32_*_{mode}_{d}`` (fp32 run) and ``n64_*_{mode}_{d}`` (fp64 run of the same fp32 points);
  - the 64 x 1024 case (its fields would be 9 MB): the depth is regenerated from the integer draws, the trig planes from ``trigrows_full``
    (2,64) and ``trigcols_full`` (2,1024) (asserted here to rebuild the reference's planes and points bit for bit); of the normals every
    ``SAMPLE_STRIDE``-th pixel is kept (``n32_full_*`` / ``n64_full_*``, (3,n)), and ``stat_full_{mode}_{d}`` records, over the whole image,
    [rms, 99th percentile of |n32 - n64| over the kept pixels, max |n32 - n64|, fraction of pixels left out, max |fp64 restatement - n64|];
  - ``bev64_small``: the fp64 run of train.py:227-239 on the case "small" at size 64, (B,3,64,64) float64.
Asserted here, on every case: the bars (a) and (b) of tests/test_normals_cpu.py."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "normals.npz")

MIN_DEPTH, MAX_DEPTH = 1.45, 80.0
MODES, DS = ("closest", "mean"), (1, 2)
MAX_EXCLUDED = 0.01
SAMPLE_STRIDE = 37
BEV_SIZE = 64
# name, seed, shape (B,H,W), kind, stored.  The 1 % cap on the pixels left out is a condition on the INPUTS, asserted in main: of the 80 pixels of
# "wrap" not one may go, and the seed 303 (one pixel, 1.25 %) was passed over for it.
CASES = [
    ("small", 301, (2, 6, 40), "scene", True),
    ("flat", 302, (1, 3, 33), "scene", True),    # H below the window
    ("wrap", 313, (2, 5, 8), "scene", True),     # the wrap reaches across most of the row
    ("tie", 304, (1, 1, 4), "valid", True),      # d = 2: (0,d) and (0,-d) are one pixel, the vertical neighbours the anchor's row: exact ties
    ("zero", 305, (1, 4, 40), "zero", True),
    ("full", 306, (1, 64, 1024), "scene", False),
]


def depth_scene(seed, shape, kind="scene"):
    """(B,1,H,W) fp32 depths in metres from integer draws (kind "valid": no pixel is 0; "zero": all are)."""
    g = np.random.Generator(np.random.PCG64(seed))
    B, H, W = shape
    if kind == "zero":
        return np.zeros((B, 1, H, W), np.float32)
    base = np.empty((B, H, W), np.float64)
    for b in range(B):
        for h in range(H):
            if h > 0 and g.integers(0, 4) != 0:
                base[b, h] = base[b, h - 1]
                continue
            w = 0
            while w < W:
                n = min(int(g.integers(8, 48)), W - w)
                start, slope = g.integers(3 * 2**10, 60 * 2**10) / 2**10, g.integers(-16, 17) / 2**10
                base[b, h, w:w + n] = start + slope * np.arange(n)
                w += n
    depth = base + g.integers(-41, 42, size=(B, H, W)) / 2**12
    holes = g.integers(0, 10, size=(B, H, W)) == 0
    if kind != "valid":
        depth[holes] = 0.0
    return depth.astype(np.float32)[:, None]


def error_stats(err, keep):
    """err (B,3,H,W) >= 0, keep (B,H,W) bool -> (rms, 99th percentile) over the components of the kept pixels."""
    import torch

    e = err.permute(0, 2, 3, 1)[keep].flatten().double()
    return e.pow(2).mean().sqrt().item(), torch.quantile(e, 0.99).item()


def order_bound(err32_max):
    """Bar (a): fp64 carries 29 more bits than fp32; 9 of them are left to the order of the operations."""
    return 2.0**-20 * err32_max + 1e-12


def main(reference):
    sys.path.insert(0, reference)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import torch
    from make_golden_render import install_kornia_stand_in

    install_kornia_stand_in()
    from utils import render as ref  # (reference)
    from utils.lidar import LiDARUtility  # (reference)

    import normals_oracle as O

    out = {}
    for name, seed, shape, kind, stored in CASES:
        B, H, W = shape
        lu = LiDARUtility((H, W), "log_depth", MIN_DEPTH, MAX_DEPTH)
        depth = torch.from_numpy(depth_scene(seed, shape, kind))
        mask = (depth > lu.min_depth) & (depth < lu.max_depth)
        xyz = lu.to_xyz(depth) / lu.max_depth * mask  # train.py:232
        trig = O.ray_trig(lu.ray_angles)
        assert torch.equal(O.frame_xyz(depth, trig, MIN_DEPTH, MAX_DEPTH).view(torch.int32), xyz.view(torch.int32)), name
        if stored:
            out[f"depth_{name}"], out[f"trig_{name}"], out[f"xyz_{name}"] = depth.numpy(), trig.numpy(), xyz.numpy()
        else:
            rows, cols = trig[:2, :, 0], trig[2:, 0, :]
            assert torch.equal(trig[:2], rows[:, :, None].expand(-1, -1, W)) and torch.equal(trig[2:], cols[:, None, :].expand(-1, H, -1))
            out[f"trigrows_{name}"], out[f"trigcols_{name}"] = rows.numpy(), cols.numpy()
        for mode in MODES:
            for d in DS:
                if d > W:
                    continue
                n32, n64 = ref.estimate_surface_normal(xyz, d, mode), ref.estimate_surface_normal(xyz.double(), d, mode)
                assert n32.dtype == torch.float32 and n64.dtype == torch.float64
                o32, i32 = O.estimate_surface_normal(xyz, d, mode, torch.float32, return_index=True)
                o64, i64 = O.estimate_surface_normal(xyz, d, mode, torch.float64, return_index=True)
                e_ref, e_o = (n32.double() - n64).abs(), (o32.double() - n64).abs()
                order = (o64 - n64).abs().max().item()
                assert order <= order_bound(e_ref.max().item()), (name, mode, d, order, e_ref.max().item())
                keep = (i32 == i64) if mode == "closest" else torch.ones(B, H, W, dtype=torch.bool)
                excluded = 1 - keep.double().mean().item()
                assert excluded <= MAX_EXCLUDED, (name, mode, d, excluded)
                (rms_r, q_r), (rms_o, q_o) = error_stats(e_ref, keep), error_stats(e_o, keep)
                assert rms_o <= 2 * rms_r and q_o <= 2 * q_r, (name, mode, d, rms_o, rms_r, q_o, q_r)
                print(f"{name} {tuple(shape)} {mode} d {d}: reference fp32 against fp64 rms {rms_r:.3e} q99 {q_r:.3e} max {e_ref.max().item():.3e}; "
                      f"restatement fp32 rms {rms_o:.3e} q99 {q_o:.3e}; fp64 restatement against the reference's fp64 {order:.3e}; left out "
                      f"{excluded:.4%}; restatement fp32 == reference fp32 bits on {(o32 == n32).all(1).double().mean().item():.2%} of the pixels")
                key = f"{name}_{mode}_{d}"
                if stored:
                    out[f"n32_{key}"], out[f"n64_{key}"] = n32.numpy(), n64.numpy()
                else:
                    pick = torch.arange(0, H * W, SAMPLE_STRIDE)
                    out[f"n32_{key}"], out[f"n64_{key}"] = n32[0].reshape(3, -1)[:, pick].numpy(), n64[0].reshape(3, -1)[:, pick].numpy()
                    out[f"stat_{key}"] = np.array([rms_r, q_r, e_ref.max().item(), excluded, order])
        if name == "small":  # train.py:227-239 in fp64
            torch.set_default_dtype(torch.float64)
            try:
                m64 = depth.double()
                x64 = lu.to_xyz(m64) / lu.max_depth * mask
                normal = lu.denormalize(-ref.estimate_surface_normal(x64))
                flat = lambda a: a.reshape(B, 3, H * W).permute(0, 2, 1)
                bev = ref.render_point_clouds(points=flat(x64), colors=flat(normal), size=BEV_SIZE, t=torch.tensor([0, 0, 1.0]).to(x64))
            finally:
                torch.set_default_dtype(torch.float32)
            assert bev.dtype == torch.float64 and (bev != 0).any() and torch.isfinite(bev).all()
            _, o_bev = O.render_normals(depth, trig, MIN_DEPTH, MAX_DEPTH, BEV_SIZE, dtype=torch.float64)
            print(f"small: fp64 BEV at size {BEV_SIZE}, {int((bev != 0).any(1).sum())} pixels hit; restatement against it {(o_bev - bev).abs().max().item():.3e}")
            out["bev64_small"] = bev.numpy()
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
