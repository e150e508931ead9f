#!/usr/bin/env python3
"""The held-out denoising loss of a checkpoint and its split over noise levels, on the GPU: ``ddpm(x_0)`` of the reference
(models/diffusion/base.py:122-149) evaluated forward-only on real scans, at every level of a fixed grid (r2dm_amd.loss.loss_curve) --
one U-Net call per scan and level, no sampling.

The scans come from either
  - ``--real_scans DIR``: a directory tree of raw Velodyne ``*.bin`` scans, projected here with the checkpoint's ``cfg.data.projection``
    and coded as the training loop codes its batches (train.py:201-214: depth in the checkpoint's coding and reflectance in [-1,1],
    -1 where nothing was measured, nearest-exact resize to ``cfg.data.resolution``); or
  - ``--real_dir DIR``: a directory of ``*.pth`` files with (5,H,W) [depth, x, y, z, reflectance] scans, what ``evaluate.py --real_dir``
    reads.
``--mask_loss`` passes the measured-pixel mask as ``loss_mask``; the default passes none, as the training loop does (train.py:265).
``--weights ema|raw`` picks the checkpoint's averaged or raw weights.  Image i draws its noise from a generator seeded ``--seed + i``.

Writes one JSON document to ``--out``: the curve (per level: t, mean log-SNR, mean unweighted loss, mean weighted loss, mean loss per
channel), the mean of the weighted loss over the levels, the checkpoint's configuration, the number of scans and the seed."""
import json
from argparse import ArgumentParser
from pathlib import Path

import torch
import torch.nn.functional as F

from evaluate import sample_files, scan_files


def _channels(cfg):
    """(channel names, their indices in [depth, reflectance]) of the checkpoint's images (train.py:201-207)."""
    picks = [(name, k) for k, (name, on) in enumerate((("depth", cfg.data.train_depth), ("reflectance", cfg.data.train_reflectance))) if on]
    return [name for name, _ in picks], [k for _, k in picks]


def images_of_scans(files, cfg, lidar_utils, batch_size, device):
    """(x_0 (N,C,H,W), measured-pixel mask (N,1,H,W)) of raw scans: the dataset builder's projection (64 rows, the projection's own
    width, masked by its depth window), then ``projection.known_from_scan``."""
    from r2dm_amd import projection

    unfolding, width = projection.parse_projection(cfg.data.projection)
    xs, ms = [], []
    for k in range(0, len(files), batch_size):
        points, offsets = projection.load_scans(files[k:k + batch_size])
        xyzrdm = projection.project_scans(points, offsets, H=64, W=width, scan_unfolding=unfolding, min_depth=lidar_utils.min_depth,
                                          max_depth=lidar_utils.max_depth, apply_mask=True, device=device)
        xs.append(projection.known_from_scan(xyzrdm, lidar_utils, cfg.data.resolution))
        ms.append(F.interpolate(xyzrdm[:, [5]].float(), size=tuple(cfg.data.resolution), mode="nearest-exact"))
    return torch.cat(xs), torch.cat(ms)


def images_of_samples(files, cfg, lidar_utils, device):
    """The same pair from (5,H,W) [depth, x, y, z, reflectance] files: a pixel counts as measured when its metric depth lies inside
    the checkpoint's depth window."""
    from r2dm_amd import projection

    imgs = torch.stack([torch.load(f, map_location="cpu").float() for f in files]).to(device)
    if imgs.dim() != 4 or imgs.shape[1] != 5:
        raise SystemExit(f"--real_dir: expected (5,H,W) scans, got {tuple(imgs.shape[1:])}")
    depth = imgs[:, [0]]
    mask = ((depth > lidar_utils.min_depth) & (depth < lidar_utils.max_depth)).float()
    xyzrdm = torch.cat([imgs[:, 1:4], imgs[:, [4]], depth, mask], dim=1) * mask
    return (projection.known_from_scan(xyzrdm, lidar_utils, cfg.data.resolution),
            F.interpolate(mask, size=tuple(cfg.data.resolution), mode="nearest-exact"))


@torch.no_grad()
def main(argv=None):
    import r2dm_amd
    from r2dm_amd import loss as loss_mod

    args = build_parser().parse_args(argv)
    if (args.real_scans is None) == (args.real_dir is None):
        raise SystemExit("give one of --real_scans DIR / --real_dir DIR")
    device = torch.device("cuda")
    ddpm, lidar_utils, cfg = r2dm_amd.setup_model(args.ckpt, device=device, ema=args.weights == "ema", show_info=False, max_batch=args.batch_size)
    if args.real_scans is not None:
        files = scan_files(args.real_scans)[:args.limit]
        if not files:
            raise SystemExit("no *.bin files below --real_scans")
        x_0, measured = images_of_scans(files, cfg, lidar_utils, args.batch_size, device)
    else:
        files = sample_files(args.real_dir, limit=args.limit)
        if not files:
            raise SystemExit("no *.pth files in --real_dir")
        x_0, measured = images_of_samples(files, cfg, lidar_utils, device)
    names, picks = _channels(cfg)
    x_0 = x_0[:, picks].contiguous()
    rng = r2dm_amd.setup_rng([args.seed + i for i in range(len(files))], device)
    curve = loss_mod.loss_curve(ddpm, x_0, loss_mask=measured if args.mask_loss else None, levels=args.levels, rng=rng,
                                batch_size=args.batch_size)
    for level in curve["levels"]:
        level["per_channel"] = dict(zip(names, level["per_channel"]))
    doc = {"curve": curve["levels"], "mean_weighted_loss": curve["mean_weighted_loss"], "num_scans": len(files), "seed": args.seed,
           "levels": args.levels, "weights": args.weights, "mask_loss": bool(args.mask_loss),
           "source": str(args.real_scans if args.real_scans is not None else args.real_dir), "config": json.loads(json.dumps(cfg_dict(cfg), default=list))}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=4)
    print(f"{len(files)} scans x {args.levels} levels: mean weighted loss {doc['mean_weighted_loss']:.6f} -> {args.out}")
    return doc


def cfg_dict(cfg):
    from dataclasses import asdict, is_dataclass

    return asdict(cfg) if is_dataclass(cfg) else dict(cfg)


def build_parser():
    parser = ArgumentParser()
    parser.add_argument("--ckpt", type=Path, required=True)
    parser.add_argument("--real_scans", type=str, default=None, help="a directory tree of raw Velodyne *.bin scans, projected here")
    parser.add_argument("--real_dir", type=str, default=None, help="a directory of (5,H,W) scans in the sample layout (*.pth)")
    parser.add_argument("--levels", type=int, default=16, help="noise levels of the curve")
    parser.add_argument("--batch_size", type=int, default=8, help="U-Net rows per call")
    parser.add_argument("--limit", type=int, default=None, help="the first so many scans (sorted)")
    parser.add_argument("--seed", type=int, default=0, help="scan i draws its noise from a generator seeded seed + i")
    parser.add_argument("--weights", choices=["ema", "raw"], default="ema")
    parser.add_argument("--mask_loss", action="store_true", help="the measured-pixel mask as loss_mask (default: none, as train.py:265)")
    parser.add_argument("--out", type=str, default="loss.json")
    return parser


if __name__ == "__main__":
    main()
