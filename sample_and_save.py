#!/usr/bin/env python3
"""Drop-in for the reference's bulk sampler (/root/reference/sample_and_save.py): same CLI, same per-seed output
files ``samples_{seed:010d}.pth`` holding a (5,H,W) [depth, x, y, z, reflectance] tensor.

Multi-GPU: launch with ``python -m torch.distributed.run --nproc-per-node N sample_and_save.py ...`` -- one process
per MI355X, seeds sharded contiguously (what Accelerate's split_batches DataLoader does in the reference,
:25-46), weights packed once on rank 0 and broadcast over RCCL/xGMI, no collective in the sampling loop.
Precision: fp32 parity by default (``--precision fp32``: 22-bit split fp16 operands, three MFMA products per fp32 product;
``fp32-bf16x3``: three bf16 pieces, fp32 operand range).  The reference runs this script under fp16 autocast (:70,
utils/option.py:49); ``--precision fp16`` is that bulk mode here: one fp16 product per MAC, fp32 accumulation and tensors,
its own tolerance class (tests/test_hip_fp16_mode.py).
``--max-batch`` / the batch size fix the layer tilings: per-seed results are bit-reproducible for a fixed batch size only.
``--mode dpmpp`` (extension) samples with DPM-Solver++(2M), ``ddpm.sample_dpm``: use it with ``--num_steps`` 16 to 32 (``--dpm_eta 1``: its stochastic member).
``--points_dir DIR`` (extension) also writes every sample as a Velodyne scan ``DIR/samples_{seed:010d}.bin``: the pixels inside the
checkpoint's depth window as fp32 [x, y, z, reflectance] rows in scan order (r2dm_amd.pointcloud)."""
import json
import os
from argparse import ArgumentParser
from pathlib import Path

import torch

import r2dm_amd
from r2dm_amd.distributed import broadcast_packed_weights, shard_seeds


def sample(args):
    torch.set_grad_enabled(False)
    world, rank, local = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", 1), ("RANK", 0), ("LOCAL_RANK", 0)))
    local = local % max(torch.cuda.device_count(), 1)  # (tests: several ranks share one GPU)
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        import torch.distributed as td

        # RCCL over xGMI ("nccl" IS RCCL on ROCm); R2DM_DIST_BACKEND=gloo lets two ranks share one GPU in tests (as bench.py)
        backend = os.environ.get("R2DM_DIST_BACKEND", "nccl")
        td.init_process_group(backend, **({"device_id": device} if backend == "nccl" else {}))

    ddpm, lidar_utils, cfg = r2dm_amd.setup_model(args.ckpt, show_info=rank == 0, max_batch=args.max_batch or args.batch_size,
                                                  precision=args.precision)
    ddpm.to(device)
    lidar_utils.to(device)
    broadcast_packed_weights(ddpm.model, device, src=0)

    save_dir = Path(args.output_dir)
    points_dir = None if args.points_dir is None else Path(args.points_dir)
    if rank == 0:
        save_dir.mkdir(parents=True, exist_ok=True)
        if points_dir is not None:
            points_dir.mkdir(parents=True, exist_ok=True)
    if world > 1:
        td.barrier()

    mine = shard_seeds(list(range(args.num_samples)), rank, world)
    for i in range(0, len(mine), args.batch_size):
        seeds = mine[i: i + args.batch_size]
        rng = r2dm_amd.setup_rng(seeds, device=device)
        # (extension: the feature cache -- only every cache_interval-th step runs the whole U-Net; the defaults are the sampler without it)
        cache = dict(cache_interval=args.cache_interval, cache_depth=args.cache_depth, cache_drift=args.cache_drift)
        if args.mode == "dpmpp":  # (extension: DPM-Solver++(2M), meant for 16-32 steps)
            samples = ddpm.sample_dpm(batch_size=len(seeds), num_steps=args.num_steps, rng=rng, progress=False, eta=args.dpm_eta, **cache).clamp(-1, 1)
        else:
            samples = ddpm.sample(batch_size=len(seeds), num_steps=args.num_steps, mode=args.mode, rng=rng, progress=False, **cache).clamp(-1, 1)
        if args.cache_drift and args.cache_interval > 1:  # per batch: (full steps, samples), the drift of the cached features between full steps
            with open(save_dir / f"cache_drift_{seeds[0]:010d}.json", "w") as f:
                json.dump({"seeds": list(seeds), "cache_interval": args.cache_interval, "cache_depth": args.cache_depth,
                           "cache_drift": [[None if v != v else v for v in row] for row in ddpm.last_cache_drift.tolist()]}, f)
        samples = lidar_utils.postprocess(samples)  # denormalize -> revert_depth -> to_xyz -> concat, one kernel
        for seed, s in zip(seeds, samples):
            torch.save(s.clone(), save_dir / f"samples_{seed:010d}.pth")
        if points_dir is not None:
            points, offsets = r2dm_amd.images_to_points(samples, lidar_utils, layout="sample", order="scan")
            r2dm_amd.save_scans(points, offsets, [points_dir / f"samples_{seed:010d}.bin" for seed in seeds])
    if world > 1:
        td.barrier()
        td.destroy_process_group()


def parser():
    parser = ArgumentParser()
    parser.add_argument("--ckpt", type=str)
    parser.add_argument("--output_dir", type=str)
    parser.add_argument("--batch_size", type=int, default=64)
    parser.add_argument("--num_samples", type=int, default=10_000)
    parser.add_argument("--num_steps", type=int, default=256)
    parser.add_argument("--mode", choices=["ddpm", "ddim", "dpmpp"], default="ddpm",
                        help="dpmpp (extension): the DPM-Solver++(2M) sampler, ddpm.sample_dpm; use it with --num_steps 16 to 32")
    parser.add_argument("--dpm_eta", type=float, default=0.0, help="--mode dpmpp: the share of fresh noise per step (0: deterministic, 1: SDE-DPM-Solver++(2M))")
    parser.add_argument("--precision", choices=["fp32", "fp32-bf16x3", "fp16"], default="fp32")
    parser.add_argument("--cache_interval", type=int, default=1, help="extension: feature cache (DeepCache): run the whole U-Net only every N-th step (1: no cache)")
    parser.add_argument("--cache_depth", type=int, default=1, choices=[1, 2, 3], help="extension: --cache_interval: the outermost U-Net levels a shallow step runs")
    parser.add_argument("--cache_drift", action="store_true", help="extension: --cache_interval: also write cache_drift_<first seed>.json per batch")
    parser.add_argument("--max-batch", type=int, default=0, help="extension: the batch size the layer tilings are planned for (default: --batch_size)")
    parser.add_argument("--points_dir", type=str, default=None, help="extension: also write every sample as a Velodyne scan samples_<seed>.bin there")
    return parser


if __name__ == "__main__":
    sample(parser().parse_args())
