#!/usr/bin/env python3
"""Drop-in for the reference's completion_demo.py: RePaint completion of one real scan under four simulated corruptions (the full
scan, every 4th beam, a random half of the beams, a random 10 % of the points).

Same options (``--ckpt --num_steps --num_resample_steps --jump_length --seed``); ``--method ddnm`` (extension) completes with the
data-consistent sampler ``ddpm.complete`` instead, ``--num_resample_steps`` then being its resampling count, ``--method dpmpp`` with ``ddpm.complete_dpm`` (the same projection on DPM-Solver++(2M), ``--dpmpp_eta``; no resampling; its image is named ``dpmpp_completion_...``); the scan comes from ``--scan FILE.bin`` (a raw
Velodyne file, projected on the GPU by r2dm_amd.projection with the checkpoint's ``cfg.data.projection``) instead of the
HuggingFace dataset lookup, and ``--out`` names the image.  The corruption masks are drawn as the reference draws them
(completion_demo.py:81-87: the same CPU draws after ``torch.manual_seed(seed)``), the completion is the same
``ddpm.repaint(..., rng=setup_rng(range(4)))`` call, clamped.

Written: one PNG with a column per corruption -- input image (depth over reflectance), input bird's-eye view, completed image,
completed bird's-eye view (r2dm_amd.render; the views coloured by height) -- and, next to it, ``completion.pt`` with ``x_in``,
``mask`` and ``x_out``.  ``--rangenet_weights PATH`` (the official ``darknet53-1024.tar.gz`` archive or a ``.pth`` state dict; a local
file, nothing is downloaded) adds the reference's segmentation: RangeNet-53 labels of the completed samples (r2dm_amd.rangenet), a
row of label-coloured images under the completed ones, the completed bird's-eye views coloured by label instead of height, and
``labels`` in ``completion.pt``.  Without it there is no segmentation row.  ``--semseg_postprocess {none,knn,crf,crf_knn}`` refines those
labels with the reference's post-processors at their defaults (r2dm_amd.postproc: the CRF-RNN on the logits, the kNN vote on the labels);
the refined labels are the ones drawn and saved.  ``--out_scan FILE.bin`` (extension) also writes the completed scan -- the completion of
the full input, the first column -- as a Velodyne file in scan order (r2dm_amd.pointcloud).  ``--ensemble K`` (extension) completes every
corruption K times (member 0 is the image's completion) and adds two rows, the fraction of members with a return at each pixel and the
standard deviation of their depth (0 to 5 m), turbo-coloured; ``completion.pt`` gains ``maps`` (4,8,H,W), r2dm_amd.ensemble_scores' maps."""
import math
from argparse import SUPPRESS, ArgumentParser
from pathlib import Path

import torch

import r2dm_amd

BATCH = 4


def corruption_masks(x_orig, seed):
    """completion_demo.py:19,81-87: four masks (4,2,H,W) on the CPU -- full, 25 % beams, random 50 % beams, random 10 % points."""
    torch.manual_seed(seed)
    H, W = x_orig.shape[-2:]
    mask = torch.zeros(1, *x_orig.shape[1:]).repeat_interleave(BATCH, dim=0)
    mask[0, ...] = 1
    mask[1, :, ::4] = 1
    mask[2, :] = torch.empty(H, 1).bernoulli_(0.5)
    mask[3, :] = torch.empty(H, W).bernoulli_(0.1)
    return mask


def known_of_scan(path, lidar_utils, cfg, device):
    """The scan as the dataset serves it (64 rows, the projection's width, masked), then completion_demo.py:66-75."""
    unfolding, width = r2dm_amd.parse_projection(cfg.data.projection)
    points, offsets = r2dm_amd.load_scans([path])
    xyzrdm = r2dm_amd.project_scans(points, offsets, H=64, W=width, scan_unfolding=unfolding, min_depth=lidar_utils.min_depth,
                                    max_depth=lidar_utils.max_depth, apply_mask=True, device=device)
    return r2dm_amd.known_from_scan(xyzrdm, lidar_utils, cfg.data.resolution)


def to_img(x, lidar_utils):
    """completion_demo.py:112-115,135: (B,2,H,W) in [-1,1] -> turbo-coloured (B,3,2H,W) in [0,1], depth over reflectance"""
    from r2dm_amd.render import colorize

    img = lidar_utils.denormalize(x)
    img[:, [0]] = lidar_utils.revert_depth(img[:, [0]]) / lidar_utils.max_depth
    return colorize(img.clamp(0, 1).flatten(1, 2), "turbo").float() / 255


def semseg_inputs(x, lidar_utils):
    """completion_demo.py:40-49 up to the normalisation, which the extractor's kernel applies: (B,2,H,W) in [-1,1] -> the (B,5,H,W)
    [depth, x, y, z, reflectance] input of RangeNet and its (B,1,H,W) mask"""
    sample = lidar_utils.denormalize(x)
    depth = lidar_utils.revert_depth(sample[:, [0]])
    mask = (depth > lidar_utils.min_depth).float()
    mask *= (depth < lidar_utils.max_depth).float()
    return torch.cat([depth, lidar_utils.to_xyz(depth), sample[:, [1]]], dim=1), mask


def semseg_postprocess(name, num_classes):
    """``--semseg_postprocess``: None, or the post-processors of ``RangeNetExtractor.segment`` at the reference's defaults"""
    from r2dm_amd.postproc import CRFRNN, KNN

    if name not in ("none", "knn", "crf", "crf_knn"):
        raise ValueError(f"--semseg_postprocess must be none, knn, crf or crf_knn, got {name!r}")
    steps = tuple(cls(num_classes) for key, cls in (("crf", CRFRNN), ("knn", KNN)) if key in name.split("_"))
    return steps or None


def to_bev(x, lidar_utils, size, colors=None):
    """completion_demo.py:117-133: (B,2,H,W) -> (B,3,size,size), coloured by height or by the given (B,3,H,W) colours in [0,1]"""
    from r2dm_amd.render import colorize, make_Rt, render_point_clouds

    R, t = make_Rt(pitch=math.pi / 4, yaw=math.pi / 4, z=0.6)
    depth = lidar_utils.revert_depth(lidar_utils.denormalize(x)[:, [0]])
    xyz = lidar_utils.to_xyz(depth) / lidar_utils.max_depth
    z_min, z_max = -2 / lidar_utils.max_depth, 0.5 / lidar_utils.max_depth
    z = (xyz[:, [2]] - z_min) / (z_max - z_min)
    if colors is None:
        colors = colorize(z.clamp(0, 1), "viridis").float() / 255
    points = xyz.flatten(2).transpose(1, 2)
    colors = 1 - colors.flatten(2).transpose(1, 2)
    return (1 - render_point_clouds(points, colors, size=size, R=R, t=t)).clamp(0, 1)


STD_SCALE = 5.0  # metres: the depth std that gets the colour map's last colour


def complete(args, ddpm, x_in, mask, rng):
    """the chosen method's completion of the four corrupted inputs from the generators ``rng``, clamped"""
    if getattr(args, "method", "repaint") == "dpmpp":  # (no resampling on the multistep solver: --num_resample_steps, --jump_length are not read)
        return ddpm.complete_dpm(known=x_in, mask=mask, num_steps=args.num_steps, eta=getattr(args, "dpmpp_eta", 1.0), rng=rng).clamp(-1, 1)
    completer = ddpm.complete if getattr(args, "method", "repaint") == "ddnm" else ddpm.repaint
    return completer(known=x_in, mask=mask, num_steps=args.num_steps, num_resample_steps=args.num_resample_steps,
                     jump_length=args.jump_length, rng=rng).clamp(-1, 1)


def ensemble_maps(args, ddpm, lidar_utils, x_orig, x_in, mask, x_out):
    """``--ensemble K``: K - 1 further completions of every corruption (member k of corruption c seeded by ``member_seed(seed, c, k)``;
    member 0 is ``x_out``) -> the (4,8,H,W) per-pixel maps of ``r2dm_amd.ensemble_scores`` against the scan itself"""
    from r2dm_amd.completion import member_seed

    if not 1 <= args.ensemble <= 64:
        raise ValueError(f"--ensemble must be in [1, 64], got {args.ensemble}")
    members = [x_out] + [complete(args, ddpm, x_in, mask, r2dm_amd.setup_rng([member_seed(args.seed, c, k) for c in range(BATCH)], device=x_in.device))
                         for k in range(1, args.ensemble)]
    samples = torch.stack([lidar_utils.postprocess(m) for m in members], dim=1)
    target = lidar_utils.postprocess(x_orig.clamp(-1, 1)).expand(BATCH, -1, -1, -1)
    return r2dm_amd.ensemble_scores(samples, target, mask[:, :1], lidar_utils.min_depth, lidar_utils.max_depth)["maps"]


def uncertainty_rows(maps):
    """two image rows (B,3,H,W) in [0,1]: the members' return probability and their depth std (0 to STD_SCALE metres), turbo-coloured"""
    from r2dm_amd.render import colorize

    return [colorize(maps[:, [0]].clamp(0, 1), "turbo").float() / 255, colorize((maps[:, [2]] / STD_SCALE).clamp(0, 1), "turbo").float() / 255]


def main(args):
    from r2dm_amd.render import make_grid, save_png

    torch.set_grad_enabled(False)
    device = torch.device("cuda")
    ddpm, lidar_utils, cfg = r2dm_amd.setup_model(args.ckpt, device=device, max_batch=BATCH, show_info=False)
    x_orig = known_of_scan(args.scan, lidar_utils, cfg, device)

    mask = corruption_masks(x_orig, args.seed).to(device)
    x_in = mask * x_orig + (1 - mask) * -1
    x_out = complete(args, ddpm, x_in, mask, r2dm_amd.setup_rng(range(BATCH), device=device))

    W = x_in.shape[-1]
    saved = {"x_in": x_in.cpu(), "mask": mask.cpu(), "x_out": x_out.cpu()}
    rows = [to_img(x_in, lidar_utils), to_bev(x_in, lidar_utils, W), to_img(x_out, lidar_utils)]
    if getattr(args, "ensemble", None) is not None:
        maps = ensemble_maps(args, ddpm, lidar_utils, x_orig, x_in, mask, x_out)
        rows += uncertainty_rows(maps)
        saved["maps"] = maps.cpu()
    if getattr(args, "rangenet_weights", None) is not None:  # completion_demo.py:105-106,138-140
        from r2dm_amd.render import colorize_labels

        semseg = r2dm_amd.rangenet.pretrained_rangenet(args.rangenet_weights, device=device)
        labels = semseg.segment(*semseg_inputs(x_out, lidar_utils), postprocess=semseg_postprocess(getattr(args, "semseg_postprocess", "none"),
                                                                                                  semseg.num_classes))
        colors = colorize_labels(labels).float() / 255
        rows += [colors, to_bev(x_out, lidar_utils, W, colors)]
        saved["labels"] = labels.cpu()
    else:
        rows.append(to_bev(x_out, lidar_utils, W))
    columns = torch.cat(rows, dim=2)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    save_png(make_grid(columns, nrow=BATCH, pad_value=1.0), args.out)
    state = args.out.parent / "completion.pt"
    torch.save(saved, state)
    print(f'Saved to "{args.out}" and "{state}"')
    if args.out_scan is not None:
        points, offsets = r2dm_amd.images_to_points(x_out[:1], lidar_utils, layout="model", order="scan")
        args.out_scan.parent.mkdir(parents=True, exist_ok=True)
        r2dm_amd.save_scans(points, offsets, [args.out_scan])
        print(f'Saved {int(offsets[-1])} points to "{args.out_scan}"')


def parser():
    p = ArgumentParser()
    p.add_argument("--ckpt", type=Path, required=True)
    p.add_argument("--num_steps", type=int, default=32)
    p.add_argument("--method", choices=("repaint", "ddnm", "dpmpp"), default="repaint",
                   help="repaint: the reference's sampler; ddnm: the data-consistent sampler (ddpm.complete), one denoiser call per step; "
                        "dpmpp: the same projection on DPM-Solver++(2M) (ddpm.complete_dpm), use it with --num_steps 16 to 32")
    p.add_argument("--dpmpp_eta", type=float, default=SUPPRESS,  # (an attribute of the parsed arguments only when given)
                   help="the dpmpp method's share of fresh noise per step (default 1: SDE-DPM-Solver++(2M); 0: deterministic)")
    p.add_argument("--num_resample_steps", type=int, default=16, help="the chosen method's resampling count")
    p.add_argument("--jump_length", type=int, default=1)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--scan", type=Path, required=True, help="a raw Velodyne scan (*.bin: float32 x, y, z, reflectance), instead of --sample_id")
    p.add_argument("--out", type=Path, default=None, help="the image (default: the reference's completion_T-..._r-..._j-....png)")
    p.add_argument("--rangenet_weights", type=str, default=None,
                   help="the official darknet53-1024.tar.gz archive or a .pth state dict (a local file): adds the segmentation row and label colours")
    p.add_argument("--semseg_postprocess", choices=("none", "knn", "crf", "crf_knn"), default="none",
                   help="refine the labels of --rangenet_weights: the kNN vote of RangeNet++, the CRF-RNN of SqueezeSeg, or the CRF-RNN and then the vote")
    p.add_argument("--ensemble", type=int, default=SUPPRESS, metavar="K",  # (an attribute of the parsed arguments only when given)
                   help="complete every corruption K times and add two image rows, the members' return probability and depth std "
                        "(the per-pixel maps go into completion.pt)")
    p.add_argument("--out_scan", type=Path, default=None, help="also write the completed scan (of the full input) as a Velodyne .bin file")
    return p


if __name__ == "__main__":
    args = parser().parse_args()
    if args.out is None:
        args.out = Path({"ddnm": "ddnm_", "dpmpp": "dpmpp_"}.get(args.method, "") + f"completion_T-{args.num_steps:04d}_r-{args.num_resample_steps:04d}_j-{args.jump_length:04d}.png")
    print(vars(args))
    main(args)
