#!/usr/bin/env python3
"""Latent interpolation between two LiDAR scans, or between two noise draws (the latent-interpolation figure of the R2DM paper; the
reference has no script for it).

``--scan_a A.bin --scan_b B.bin``: two raw Velodyne scans, projected on the GPU with the checkpoint's ``cfg.data.projection`` (as
``completion_demo.py`` does), are encoded by DDIM inversion up to ``--t_end`` (``ddpm.invert``, ``--steps`` steps), their latents are
interpolated spherically at ``--frames`` weights from 0 to 1 (``r2dm_amd.latent.slerp``) and every frame is decoded by the DDIM sampler
from there (``ddpm.sample_from(..., clip=False)``): ``r2dm_amd.latent.interpolate``.  ``--seed_a S --seed_b T``: the two latents are the
draws at t = 1 that ``setup_rng([S])`` and ``setup_rng([T])`` give ``ddpm.sample``; nothing is inverted.  ``--decoder dpmpp`` decodes the
interpolated latents with the DPM-Solver++(2M) sampler instead (``ddpm.sample_dpm(x_t=..., clip=False)``).

Written to ``--out_dir``: ``interpolation.png``, one column per frame -- the colour-mapped range image over the reflectance image over the
bird's-eye view (r2dm_amd.render) -- and ``interpolation.pt`` with ``latents`` and ``frames`` (F,1,2,H,W), for scans also ``x_a`` and
``x_b``.  ``--points_dir DIR``: every frame as a Velodyne file ``DIR/frame_%04d.bin`` (r2dm_amd.pointcloud).  For scans one JSON line on
stdout: the angle ``omega`` between the two latents and, for each end, the round-trip error of the model -- frame 0 against scan A, the
last frame against scan B: MAE and RMSE of the metric range and of the reflectance over the whole image
(``r2dm_amd.completion_errors`` with nothing known)."""
import json
import math
from argparse import ArgumentParser
from pathlib import Path

import torch

import r2dm_amd
from completion_demo import known_of_scan


def display(x, lidar_utils):
    """(N,2,H,W) in [-1,1] -> both channels in [0,1], the depth in metres over ``max_depth`` (what generate.py renders)"""
    x = lidar_utils.denormalize(x.clamp(-1, 1))
    x[:, [0]] = lidar_utils.revert_depth(x[:, [0]]) / lidar_utils.max_depth
    return x


def round_trip(frame, x_ref, lidar_utils):
    """range / reflectance MAE and RMSE of a decoded frame against the scan it should reproduce, over every pixel with a return"""
    pred, target = lidar_utils.postprocess(frame.clamp(-1, 1)), lidar_utils.postprocess(x_ref)
    known = torch.zeros(pred.shape[0], 1, *pred.shape[2:], device=pred.device)
    err = r2dm_amd.completion_errors(pred, target, known, lidar_utils.min_depth, lidar_utils.max_depth)
    return {k: [float(f"{v:.6g}") for v in err[k].tolist()] for k in ("mae_depth", "rmse_depth", "mae_reflectance", "rmse_reflectance")}


def main(args):
    from r2dm_amd import latent
    from r2dm_amd.render import make_grid, render_frames, save_png

    torch.set_grad_enabled(False)
    device = torch.device("cuda")
    scans = args.scan_a is not None
    if scans != (args.scan_b is not None) or scans == (args.seed_a is not None) or (args.seed_a is None) != (args.seed_b is None):
        raise SystemExit("give either --scan_a and --scan_b, or --seed_a and --seed_b")
    ddpm, lidar_utils, cfg = r2dm_amd.setup_model(args.ckpt, device=device, show_info=False)
    saved, row = {}, None
    if scans:
        x_a, x_b = (known_of_scan(p, lidar_utils, cfg, device) for p in (args.scan_a, args.scan_b))
        frames, latents = latent.interpolate(ddpm, x_a, x_b, args.frames, args.steps, t_end=args.t_end, return_latents=True, decoder=args.decoder)
        saved.update(x_a=x_a.cpu(), x_b=x_b.cpu())
        cos = torch.nn.functional.cosine_similarity(latents[0].flatten(1).double(), latents[-1].flatten(1).double()).clamp(-1, 1)
        row = {"frames": args.frames, "steps": args.steps, "t_end": args.t_end, "omega": [float(f"{v:.6g}") for v in cos.acos().tolist()],
               "scan_a": round_trip(frames[0], x_a, lidar_utils), "scan_b": round_trip(frames[-1], x_b, lidar_utils)}
    else:
        z = [ddpm.randn(1, *ddpm.sampling_shape, rng=r2dm_amd.setup_rng([s], device), device=device) for s in (args.seed_a, args.seed_b)]
        latents = latent.slerp(z[0], z[1], torch.linspace(0.0, 1.0, args.frames).tolist())
        cap = ddpm.model.max_batch
        if args.decoder == "dpmpp":
            decode = lambda z: ddpm.sample_dpm(z.shape[0], args.steps, x_t=z, clip=False, progress=False)
        else:
            decode = lambda z: ddpm.sample_from(z, args.steps, progress=False, mode="ddim")
        frames = torch.cat([decode(latents[k:k + cap, 0]) for k in range(0, args.frames, cap)])[:, None]
    saved.update(latents=latents.cpu(), frames=frames.cpu())

    args.out_dir.mkdir(parents=True, exist_ok=True)
    W = frames.shape[-1]
    img, bev = render_frames(display(frames[:, 0], lidar_utils), lidar_utils, size=W)
    save_png(make_grid(torch.cat([img, bev], dim=2), nrow=args.frames, pad_value=1.0), args.out_dir / "interpolation.png")
    torch.save(saved, args.out_dir / "interpolation.pt")
    print(f'Saved to "{args.out_dir / "interpolation.png"}" and "{args.out_dir / "interpolation.pt"}"')
    if args.points_dir is not None:
        args.points_dir.mkdir(parents=True, exist_ok=True)
        points, offsets = r2dm_amd.images_to_points(frames[:, 0].clamp(-1, 1), lidar_utils, layout="model", order="scan")
        r2dm_amd.save_scans(points, offsets, [args.points_dir / f"frame_{k:04d}.bin" for k in range(args.frames)])
        print(f'Saved {int(offsets[-1])} points of {args.frames} frames to "{args.points_dir}"')
    if row is not None:
        print(json.dumps(row))


def parser():
    p = ArgumentParser()
    p.add_argument("--ckpt", type=Path, required=True)
    p.add_argument("--scan_a", type=Path, default=None, help="a raw Velodyne scan (*.bin: float32 x, y, z, reflectance)")
    p.add_argument("--scan_b", type=Path, default=None)
    p.add_argument("--seed_a", type=int, default=None, help="instead of two scans: the seeds of two noise draws at t = 1")
    p.add_argument("--seed_b", type=int, default=None)
    p.add_argument("--frames", type=int, default=8, help="frames from A to B, both ends included")
    p.add_argument("--steps", type=int, default=32, help="steps of the inversion and of the decoding")
    p.add_argument("--t_end", type=float, default=1.0, help="the noise level the scans are inverted to, in (0, 1]")
    p.add_argument("--decoder", choices=["ddim", "dpmpp"], default="ddim",
                   help="how the interpolated latents are decoded: the DDIM sampler, or dpmpp: DPM-Solver++(2M), ddpm.sample_dpm(x_t=..., clip=False)")
    p.add_argument("--out_dir", type=Path, default=Path("interpolation"))
    p.add_argument("--points_dir", type=Path, default=None, help="also write every frame as a Velodyne .bin file there")
    return p


if __name__ == "__main__":
    args = parser().parse_args()
    if args.frames < 2 or args.steps < 1 or not 0.0 < args.t_end <= 1.0:
        raise SystemExit("--frames must be at least 2, --steps at least 1 and --t_end in (0, 1]")
    main(args)
