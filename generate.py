#!/usr/bin/env python3
"""Drop-in for the reference's generate.py: same CLI, same sampling call, same post-processing of
the returned (S+1,B,2,H,W) stack, which is saved as tensors.  With ``--render_dir DIR`` the last frame is also rendered as the
reference renders it (generate.py:44-63, r2dm_amd/render.py): ``samples_img.png``, the turbo-coloured range / reflectance
images, and ``samples_bev.png``, the bird's-eye views; ``--render_frames`` adds ``frames/bev_%04d.png`` for every frame of the
stack, ``--render_normals`` the view of the reference's training monitor (train.py:227-239): ``samples_normal.png``, the surface normals
as colours, and ``samples_bev_normal.png``, the bird's-eye views coloured by them.  With ``--points_dir DIR`` the final samples are also written as Velodyne scans ``DIR/samples_%04d.bin`` (fp32 [x, y, z,
reflectance] rows in scan order, r2dm_amd.pointcloud), with ``--points_ply`` also as ``.ply`` coloured by the bird's-eye views' viridis
height map.  ``--mode dpmpp`` (extension) samples with DPM-Solver++(2M), ``ddpm.sample_dpm``, meant for ``--sampling_steps`` 16 to 32 (``--dpm_eta 1``: its stochastic member, SDE-DPM-Solver++(2M)).  Still missing from the reference's script: the mp4 (no encoder here) and the antialiased 512-pixel resize of its frames."""
import argparse
import json
from pathlib import Path

import torch

import r2dm_amd


def main(args):
    torch.set_grad_enabled(False)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    ddpm, lidar_utils, _ = r2dm_amd.setup_model(args.ckpt, device=args.device, max_batch=args.batch_size)
    # (extension: the feature cache -- only every cache_interval-th step runs the whole U-Net; the defaults are the sampler without it)
    cache = dict(cache_interval=args.cache_interval, cache_depth=args.cache_depth, cache_drift=args.cache_drift)
    if args.mode == "dpmpp":  # (extension: DPM-Solver++(2M), meant for 16-32 steps)
        xs = ddpm.sample_dpm(batch_size=args.batch_size, num_steps=args.sampling_steps, return_all=True, eta=args.dpm_eta, **cache).clamp(-1, 1)
    else:
        xs = ddpm.sample(batch_size=args.batch_size, num_steps=args.sampling_steps, mode=args.mode, return_all=True, **cache).clamp(-1, 1)
    if args.cache_drift and args.cache_interval > 1:  # one more JSON line: how far the cached features moved between full steps, per full step and sample
        print(json.dumps({"cache_interval": args.cache_interval, "cache_depth": args.cache_depth, "cache_drift": [[None if v != v else v for v in row] for row in ddpm.last_cache_drift.tolist()]}))
    xs = lidar_utils.denormalize(xs)
    xs[:, :, [0]] = lidar_utils.revert_depth(xs[:, :, [0]]) / lidar_utils.max_depth
    points = lidar_utils.postprocess(_last_sample_normalized(xs, lidar_utils))
    torch.save({"frames": xs.cpu(), "points": points.cpu()}, args.output)
    print(f"saved {tuple(xs.shape)} frames and {tuple(points.shape)} [depth,x,y,z,reflectance] maps to {args.output}")
    if args.render_dir is not None:
        render(xs, lidar_utils, args)
    if args.points_dir is not None:
        save_points(points, lidar_utils, args)


def save_points(samples, lidar_utils, args):
    """The final samples (B,5,H,W) as one Velodyne scan each, in scan order; with --points_ply the same cloud as a coloured PLY."""
    from r2dm_amd.pointcloud import height_colors

    args.points_dir.mkdir(parents=True, exist_ok=True)
    cloud, offsets = r2dm_amd.images_to_points(samples, lidar_utils, layout="sample", order="scan")
    names = [args.points_dir / f"samples_{k:04d}" for k in range(len(samples))]
    r2dm_amd.save_scans(cloud, offsets, [n.with_suffix(".bin") for n in names])
    if args.points_ply:
        colors = height_colors(cloud, lidar_utils.max_depth)
        for k, n in enumerate(names):
            r2dm_amd.save_ply(cloud[offsets[k]:offsets[k + 1]], n.with_suffix(".ply"), colors[offsets[k]:offsets[k + 1]])
    print(f"wrote {len(names)} scans ({int(offsets[-1])} points) to {args.points_dir}")


def render(xs, lidar_utils, args):
    """generate.py:61-63 on the last frame; with --render_frames the BEV of every frame, a few sampling steps per launch."""
    from r2dm_amd.render import make_grid, render_frames, render_normals, save_png

    args.render_dir.mkdir(parents=True, exist_ok=True)
    img, bev = render_frames(xs[-1], lidar_utils, size=args.bev_size)
    save_png(make_grid(img, nrow=1), args.render_dir / "samples_img.png")
    save_png(make_grid(bev, nrow=4), args.render_dir / "samples_bev.png")
    written = 2
    if args.render_normals:
        colors, bev = render_normals(xs[-1][:, [0]] * lidar_utils.max_depth, lidar_utils, size=args.bev_size)
        save_png(make_grid(colors, nrow=1), args.render_dir / "samples_normal.png")
        save_png(make_grid(bev, nrow=4), args.render_dir / "samples_bev_normal.png")
        written += 2
    if args.render_frames:
        (args.render_dir / "frames").mkdir(exist_ok=True)
        S1, B = xs.shape[:2]
        steps = max(1, 64 // B)
        for s0 in range(0, S1, steps):
            _, bev = render_frames(xs[s0:s0 + steps].flatten(0, 1), lidar_utils, size=args.bev_size)
            for k, frame in enumerate(bev.unflatten(0, (-1, B))):
                save_png(make_grid(frame, nrow=B, pad_value=1.0), args.render_dir / "frames" / f"bev_{s0 + k:04d}.png")
                written += 1
    print(f"rendered {written} images to {args.render_dir}")


def _last_sample_normalized(xs, lidar_utils):
    """Undo the display scaling of the final frame to feed the fused xyz post-processing kernel."""
    last = xs[-1].clone()
    last[:, [0]] = lidar_utils.convert_depth(last[:, [0]] * lidar_utils.max_depth)
    return lidar_utils.normalize(last)


def parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--ckpt", type=Path, required=True)
    parser.add_argument("--device", choices=["cuda"], default="cuda")
    parser.add_argument("--mode", choices=["ddpm", "ddim", "dpmpp"], default="ddpm",
                        help="dpmpp (extension): the DPM-Solver++(2M) sampler, ddpm.sample_dpm; use it with --sampling_steps 16 to 32")
    parser.add_argument("--dpm_eta", type=float, default=0.0, help="--mode dpmpp: the share of fresh noise per step (0: deterministic, 1: SDE-DPM-Solver++(2M))")
    parser.add_argument("--cache_interval", type=int, default=1, help="feature cache (DeepCache): run the whole U-Net only every N-th step (1: no cache)")
    parser.add_argument("--cache_depth", type=int, default=1, choices=[1, 2, 3], help="--cache_interval: the outermost U-Net levels a shallow step runs")
    parser.add_argument("--cache_drift", action="store_true", help="--cache_interval: print the drift of the cached features as one more JSON line")
    parser.add_argument("--batch_size", type=int, default=1)
    parser.add_argument("--sampling_steps", type=int, default=256)
    parser.add_argument("--output", type=Path, default=Path("samples.pt"))
    parser.add_argument("--seed", type=int, default=None, help="seed of torch's global generators (default: not seeded, as the reference)")
    parser.add_argument("--render_dir", type=Path, default=None, help="also write samples_img.png and samples_bev.png there")
    parser.add_argument("--bev_size", type=int, default=800, help="side of a bird's-eye view in pixels")
    parser.add_argument("--render_frames", action="store_true", help="with --render_dir: frames/bev_%%04d.png for every frame of the stack")
    parser.add_argument("--render_normals", action="store_true",
                        help="with --render_dir: also samples_normal.png and samples_bev_normal.png, the surface normals and the bird's-eye views coloured by them")
    parser.add_argument("--points_dir", type=Path, default=None, help="also write the final samples as Velodyne scans samples_%%04d.bin there")
    parser.add_argument("--points_ply", action="store_true", help="with --points_dir: also samples_%%04d.ply, coloured by height")
    return parser


if __name__ == "__main__":
    args = parser().parse_args()
    args.device = torch.device(args.device)
    main(args)
