#!/usr/bin/env python3
"""Scores a directory of generated ``samples_*.pth`` files ((5,H,W) [depth, x, y, z, reflectance], what sample_and_save.py writes and
evaluate.py reads) against a real set in 3-D, on the GPU: coverage (COV), minimum matching distance (MMD) and 1-nearest-neighbour accuracy
(1-NNA) under the squared Chamfer distance between point clouds (the PointFlow / LiDM definitions; r2dm_amd.geometry, DESIGN.md section 4,
"Geometry metrics") or, with ``--distance emd``, under the earth mover's distance (the protocol's second column: Chamfer is blind to
density, a one-to-one matching is not).  There every scan must have ``--points`` points inside the window, and the document also carries
``emd_eps`` and ``emd_max_gap``, the largest certified distance of an entry from its exact value.

The real set comes from either
  - ``--real_dir DIR``: a directory of ``*.pth`` scans in the sample layout; or
  - ``--real_scans DIR`` with ``--ckpt``: a directory tree of raw Velodyne ``*.bin`` scans, projected here with the checkpoint's
    ``cfg.data.projection`` and resized to ``cfg.data.resolution`` as evaluate.py does.
A pixel is a point when its depth lies inside LiDARGen's window (0.5 m, 63 m), as in evaluate.py.  Every cloud is subsampled to
``--points`` points, cloud i of a set by a generator seeded from ``(--seed, i)``; the first ``--limit`` files of each set are used, because
the cost is quadratic in the set size ((G + R)^2 / 2 cloud pairs).  Writes one JSON document to ``--out``."""
import json
from argparse import ArgumentParser
from pathlib import Path

import torch

from evaluate import MAX_DEPTH, MIN_DEPTH, load_batches, sample_files, scan_files


def clouds_of_files(files, points, seed, batch_size, num_workers, device):
    """(N,points,4) subsampled clouds and (N,) counts of sample files"""
    from r2dm_amd import geometry

    clouds, counts, done = [], [], 0
    for imgs in load_batches(files, batch_size, num_workers):
        c, n = geometry.subsample(*geometry.clouds_of_samples(imgs.to(device), MIN_DEPTH, MAX_DEPTH), points, seed, first_index=done)
        clouds.append(c)
        counts.append(n)
        done += c.shape[0]
    return torch.cat(clouds), torch.cat(counts)


def clouds_of_scans(files, cfg, points, seed, batch_size, device):
    """The same of raw scans: the dataset builder's projection, evaluate.py's resize to the model's resolution (nearest-exact)."""
    import torch.nn.functional as F

    from r2dm_amd import geometry, projection

    unfolding, width = projection.parse_projection(cfg.data.projection)
    H, W = cfg.data.resolution
    clouds, counts = [], []
    for k in range(0, len(files), batch_size):
        pts, offsets = projection.load_scans(files[k:k + batch_size])
        imgs = projection.project_scans(pts, offsets, H=64, W=width, scan_unfolding=unfolding, apply_mask=True,
                                        out_width=W if W <= width else None, layout="sample", device=device)
        if tuple(imgs.shape[-2:]) != (H, W):
            imgs = F.interpolate(imgs, size=(H, W), mode="nearest-exact")
        c, n = geometry.subsample(*geometry.clouds_of_samples(imgs, MIN_DEPTH, MAX_DEPTH), points, seed, first_index=k)
        clouds.append(c)
        counts.append(n)
    return torch.cat(clouds), torch.cat(counts)


@torch.no_grad()
def main(argv=None):
    from r2dm_amd import geometry

    args = build_parser().parse_args(argv)
    if (args.real_scans is None) == (args.real_dir is None):
        raise SystemExit("give one of --real_scans DIR (with --ckpt) / --real_dir DIR")
    if args.points < 1 or args.limit < 1:
        raise SystemExit("--points and --limit must be >= 1")
    device = torch.device("cuda")
    gen_files = sample_files(args.sample_dir, limit=args.limit)
    if not gen_files:
        raise SystemExit("no *.pth files in --sample_dir")
    if args.real_scans is not None:
        if args.ckpt is None:
            raise SystemExit("--real_scans needs --ckpt (the projection and the resolution of the real scans)")
        from r2dm_amd.option import Config

        cfg = Config(**torch.load(args.ckpt, map_location="cpu")["cfg"])
        real_files = scan_files(args.real_scans)[:args.limit]
        if not real_files:
            raise SystemExit("no *.bin files below --real_scans")
        R, nR = clouds_of_scans(real_files, cfg, args.points, args.seed, args.batch_size, device)
    else:
        real_files = sample_files(args.real_dir, limit=args.limit)
        if not real_files:
            raise SystemExit("no *.pth files in --real_dir")
        R, nR = clouds_of_files(real_files, args.points, args.seed, args.batch_size, args.num_workers, device)
    G, nG = clouds_of_files(gen_files, args.points, args.seed, args.batch_size, args.num_workers, device)
    empty = int((nG == 0).sum().item()), int((nR == 0).sum().item())
    if any(empty):
        raise SystemExit(f"{empty[0]} generated and {empty[1]} real scans have no point inside ({MIN_DEPTH} m, {MAX_DEPTH} m): the set metrics "
                         "are defined for clouds with points")
    extra = {}
    if args.distance == "emd":
        short = int((nG < args.points).sum().item()), int((nR < args.points).sum().item())
        if any(short):
            raise SystemExit(f"{short[0]} generated and {short[1]} real scans have fewer than --points = {args.points} points inside ({MIN_DEPTH} m, "
                             f"{MAX_DEPTH} m): the earth mover's distance is defined between clouds of the same size")
        (D_gr, gap_gr), (D_gg, gap_gg), (D_rr, gap_rr) = (geometry.pairwise_emd(X, nX, Y, nY, eps=args.emd_eps, max_rounds=args.emd_max_rounds)
                                                          for X, nX, Y, nY in ((G, nG, R, nR), (G, nG, None, None), (R, nR, None, None)))
        # the largest certified emd - lower over all pairs: how far from the exact distance any entry can be
        extra = {"emd_eps": args.emd_eps, "emd_max_gap": max(g.max().item() for g in (gap_gr, gap_gg, gap_rr))}
    else:
        D_gr = geometry.pairwise_chamfer(G, nG, R, nR)
        D_gg = geometry.pairwise_chamfer(G, nG, G, nG)
        D_rr = geometry.pairwise_chamfer(R, nR, R, nR)
    doc = dict(geometry.set_metrics(D_gg, D_gr, D_rr))
    doc.update({"#fake": len(gen_files), "#real": len(real_files), "points": args.points, "seed": args.seed, "distance": args.distance,
                "min_depth": MIN_DEPTH, "max_depth": MAX_DEPTH, "directory": str(args.sample_dir),
                "real": str(args.real_scans if args.real_scans is not None else args.real_dir)})
    doc.update(extra)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=4)
    print(f"COV {doc['cov']:.4f}  MMD {doc['mmd']:.6f}  1-NNA {doc['1-nna']:.4f}  ({len(gen_files)} generated, {len(real_files)} real) -> {args.out}")
    return doc


def build_parser():
    parser = ArgumentParser()
    parser.add_argument("--sample_dir", type=str, required=True, help="a directory of generated samples_*.pth files")
    parser.add_argument("--real_dir", type=str, default=None, help="a directory of (5,H,W) real scans in the sample layout (*.pth)")
    parser.add_argument("--real_scans", type=str, default=None, help="a directory tree of raw Velodyne *.bin scans, projected here (needs --ckpt)")
    parser.add_argument("--ckpt", type=Path, default=None)
    parser.add_argument("--points", type=int, default=2048, help="points per cloud after subsampling")
    parser.add_argument("--limit", type=int, default=2000, help="the first so many files of each set: the cost is quadratic")
    parser.add_argument("--seed", type=int, default=0, help="cloud i of a set is subsampled by a generator seeded from (seed, i)")
    parser.add_argument("--batch_size", type=int, default=64)
    parser.add_argument("--num_workers", type=int, default=4)
    parser.add_argument("--out", type=str, default="geometry.json")
    parser.add_argument("--distance", choices=("cd_sq", "emd"), default="cd_sq",
                        help="the distance between two clouds: squared Chamfer, or the earth mover's distance (every scan needs --points points)")
    parser.add_argument("--emd_eps", type=float, default=0.01, help="--distance emd: accuracy of a distance, metres per point")
    parser.add_argument("--emd_max_rounds", type=int, default=1 << 20, help="--distance emd: bidding rounds of the auction per cloud pair")
    return parser


if __name__ == "__main__":
    main()
