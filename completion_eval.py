#!/usr/bin/env python3
"""Scores scan completion on held-out scans, on the GPU: every scan is corrupted (``--corruption``: ``full``, ``beams:K``,
``random_beams:P``, ``random_points:P``; repeatable), completed by RePaint, by the data-consistent sampler (``ddnm``: ``ddpm.complete``, one
denoiser call per step; ``--ddnm_resample_steps``, and ``--ddnm_init linear --ddnm_t_start 0.5`` to start it from the interpolated scan), by
the same projection on DPM-Solver++(2M) (``dpmpp``: ``ddpm.complete_dpm``, meant for ``--num_steps`` 16 to 32; ``--dpmpp_eta``, ``--dpmpp_order``,
``--dpmpp_init``, ``--dpmpp_t_start``)
and / or by nearest / linear interpolation of the known beams (``--methods``), and compared with the scan itself -- mean absolute and root-mean-square error of range and reflectance over the pixels
that had to be filled in, the recall of returns, the rate of false returns and, with ``--rangenet_weights``, the IoU of the RangeNet-53
labels of the completed image against the labels of the real scan (r2dm_amd.completion.evaluate_completion; DESIGN.md section 4,
"Completion metrics").  ``--chamfer`` also scores the completion in 3-D: Chamfer distance and the F-score at ``--fscore_threshold`` metres
of the prediction's returns against the scan's, over the whole image and over the inpainted pixels (``results[kind][method]["geometry"]``;
DESIGN.md section 4, "Geometry metrics").

The scans come from either
  - ``--real_scans DIR``: a directory tree of raw Velodyne ``*.bin`` scans, projected here with the checkpoint's ``cfg.data.projection``
    (64 rows, the projection's width, masked by the depth window) and resized to ``cfg.data.resolution`` (nearest-exact); or
  - ``--real_dir DIR``: a directory of ``*.pth`` files with (5,H,W) [depth, x, y, z, reflectance] scans at the model's resolution, what
    ``evaluate.py --real_dir`` reads.
``--rangenet_weights PATH`` is the official ``darknet53-1024.tar.gz`` archive or a ``.pth`` state dict (a local file; nothing is
downloaded); ``--semseg_postprocess`` refines the labels of both images with the reference's post-processors.  Scan i draws its masks and
its RePaint noise from generators seeded from ``(--seed, i)`` (r2dm_amd.completion.scan_seed), whatever ``--batch_size``.

Writes one JSON document to ``--out``: ``info`` (checkpoint, number of scans, settings) and ``results[kind][method]`` (counts, error
sums, micro and macro averages, per-class IoU and mIoU, or ``skipped``); an undefined value is ``null``.  ``--save_dir DIR`` also writes
the tensors behind the numbers, one ``.pt`` file per corruption.

``--ensemble K`` draws K completions per scan with every stochastic method (member k of scan i seeded by
r2dm_amd.completion.member_seed; member 0 is the single draw, on which everything above is still scored) and adds
``results[kind][method]["ensemble"]``: the continuous ranked probability score of range and reflectance (the mean absolute error at K = 1,
so the interpolation baselines share the column), the rank histogram and the spread / skill ratio (calibration), the Brier score of ray
drop, best-of-K and the errors of the consensus scan ("Ensemble scores"); ``--save_dir`` then also keeps the per-pixel
return-probability, mean, std and median maps.

``--ensemble_coherence`` (with ``--ensemble``) also scores the members across pixels, which none of the above does: the energy score and
the variogram score of order 0.5 over ``--coherence_offsets`` (pairs "dh,dw"; default r2dm_amd.completion.DEFAULT_OFFSETS), which tell a
coherent draw from per-pixel noise with the same marginals (``results[kind][method]["ensemble"]["coherence"]``; DESIGN.md section 4,
"Ensemble coherence").

``--voxel_iou S [S ...]`` also scores the same clouds by voxel occupancy at the voxel sizes S in metres (the literature's column is 0.1):
IoU, precision, recall and F1 of the occupied voxels, whole image and inpainted pixels (``results[kind][method]["voxel"]``); with
``--ensemble K`` (at most 63 then) the K members also vote on every voxel -- the members' IoU, the "any" and "consensus" occupancy against
the scan's, the Brier score of the occupancy probability and its reliability curve (``results[kind][method]["ensemble"]["occupancy"]``;
DESIGN.md section 4, "Voxel occupancy")."""
import json
from argparse import SUPPRESS, ArgumentParser
from pathlib import Path

import torch
import torch.nn.functional as F

from evaluate import sample_files, scan_files


def planes_of_scans(files, cfg, lidar_utils, batch_size, device):
    """(N,6,H,W) masked [x, y, z, reflectance, depth, mask] planes of raw scans at ``cfg.data.resolution``"""
    from r2dm_amd import projection

    unfolding, width = projection.parse_projection(cfg.data.projection)
    out = []
    for k in range(0, len(files), batch_size):
        points, offsets = projection.load_scans(files[k:k + batch_size])
        xyzrdm = projection.project_scans(points, offsets, H=64, W=width, scan_unfolding=unfolding, min_depth=lidar_utils.min_depth,
                                          max_depth=lidar_utils.max_depth, apply_mask=True, device=device)
        out.append(F.interpolate(xyzrdm, size=tuple(cfg.data.resolution), mode="nearest-exact"))
    return torch.cat(out)


def planes_of_samples(files, cfg, lidar_utils, device):
    """The same planes from (5,H,W) [depth, x, y, z, reflectance] files: a pixel counts as measured when its depth lies inside the
    checkpoint's depth window."""
    imgs = torch.stack([torch.load(f, map_location="cpu").float() for f in files]).to(device)
    if imgs.dim() != 4 or imgs.shape[1] != 5:
        raise SystemExit(f"--real_dir: expected (5,H,W) scans, got {tuple(imgs.shape[1:])}")
    if tuple(imgs.shape[-2:]) != tuple(cfg.data.resolution):
        imgs = F.interpolate(imgs, size=tuple(cfg.data.resolution), mode="nearest-exact")
    depth = imgs[:, [0]]
    mask = ((depth > lidar_utils.min_depth) & (depth < lidar_utils.max_depth)).float()
    planes = torch.cat([imgs[:, 1:4], imgs[:, [4]], depth, mask], dim=1)
    return torch.where(mask != 0, planes, torch.zeros_like(planes))


@torch.no_grad()
def main(argv=None):
    import r2dm_amd
    from completion_demo import semseg_postprocess
    from r2dm_amd import completion

    parser = build_parser()
    args = parser.parse_args(argv)
    coherence = coherence_settings(parser, args)
    if (args.real_scans is None) == (args.real_dir is None):
        raise SystemExit("give one of --real_scans DIR / --real_dir DIR")
    kinds = list(dict.fromkeys(args.corruption or ["beams:4"]))
    for kind in kinds:
        completion.parse_kind(kind)
    device = torch.device("cuda")
    ddpm, lidar_utils, cfg = r2dm_amd.setup_model(args.ckpt, device=device, show_info=False, max_batch=args.batch_size)
    if args.real_scans is not None:
        files = scan_files(args.real_scans)[:args.limit]
        if not files:
            raise SystemExit("no *.bin files below --real_scans")
        planes = planes_of_scans(files, cfg, lidar_utils, args.batch_size, device)
    else:
        files = sample_files(args.real_dir, limit=args.limit)
        if not files:
            raise SystemExit("no *.pth files in --real_dir")
        planes = planes_of_samples(files, cfg, lidar_utils, device)
    semseg, post = None, None
    if args.rangenet_weights is not None:
        semseg = r2dm_amd.rangenet.pretrained_rangenet(args.rangenet_weights, device=device)
        post = semseg_postprocess(args.semseg_postprocess, semseg.num_classes)
    dpmpp = dpmpp_settings(args)
    out = completion.evaluate_completion(ddpm, lidar_utils, planes, kinds, methods=tuple(args.methods), num_steps=args.num_steps,
                                         num_resample_steps=args.num_resample_steps, jump_length=args.jump_length, seed=args.seed,
                                         batch_size=args.batch_size, semseg=semseg, semseg_postprocess=post, keep=args.save_dir is not None,
                                         chamfer=args.chamfer, fscore_threshold=args.fscore_threshold, ddnm_resample_steps=args.ddnm_resample_steps,
                                         ddnm_init=None if args.ddnm_init == "none" else args.ddnm_init, ddnm_t_start=args.ddnm_t_start,
                                         **{**dpmpp, "dpmpp_init": None if dpmpp["dpmpp_init"] == "none" else dpmpp["dpmpp_init"]},
                                         **({"ensemble": args.ensemble} if hasattr(args, "ensemble") else {}), **coherence,
                                         **({"voxel_sizes": args.voxel_iou} if hasattr(args, "voxel_iou") else {}))
    results, kept = out if args.save_dir is not None else (out, None)
    info = {"ckpt": str(args.ckpt), "source": str(args.real_scans if args.real_scans is not None else args.real_dir), "num_scans": len(files),
            "resolution": list(cfg.data.resolution), "corruptions": kinds, "methods": list(args.methods), "num_steps": args.num_steps,
            "num_resample_steps": args.num_resample_steps, "jump_length": args.jump_length, "batch_size": args.batch_size, "seed": args.seed,
            "lo": float(lidar_utils.min_depth), "hi": float(lidar_utils.max_depth), "rangenet_weights": args.rangenet_weights,
            "semseg_postprocess": args.semseg_postprocess if semseg is not None else None}
    if args.chamfer:
        info["fscore_threshold"] = args.fscore_threshold
    if "ddnm" in args.methods:
        info.update(ddnm_resample_steps=args.ddnm_resample_steps, ddnm_init=args.ddnm_init, ddnm_t_start=args.ddnm_t_start)
    if "dpmpp" in args.methods:
        info.update(dpmpp)
    if hasattr(args, "ensemble"):
        info["ensemble"] = args.ensemble
    if coherence:
        info["ensemble_coherence"] = True
    if hasattr(args, "voxel_iou"):
        info["voxel_sizes"] = args.voxel_iou
    doc = completion.jsonable({"info": info, "results": results})
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=4, allow_nan=False)
    if kept is not None:
        args.save_dir.mkdir(parents=True, exist_ok=True)
        for kind, tensors in kept.items():
            torch.save(tensors, args.save_dir / (kind.replace(":", "_") + ".pt"))
    for kind in kinds:
        for method, entry in results[kind].items():
            if "skipped" in entry:
                print(f"{kind:>20} {method:>8}: skipped")
                continue
            m, iou = entry["micro"], entry.get("iou", {}).get("miou")
            print(f"{kind:>20} {method:>8}: MAE depth {m['mae_depth']:.4f} m, reflectance {m['mae_reflectance']:.4f}, recall {m['return_recall']:.4f}"
                  + ("" if iou is None else f", mIoU {iou:.4f}")
                  + (f", inpainted CD {entry['geometry']['inpainted']['micro']['cd']:.4f} m, F-score {entry['geometry']['inpainted']['micro']['fscore']:.4f}"
                     if "geometry" in entry else "")
                  + (f", inpainted voxel IoU {entry['voxel']['inpainted']['micro']['iou'][0]:.4f} at {entry['voxel']['sizes'][0]:g} m"
                     if "voxel" in entry else ""))
            if "ensemble" in entry:
                e = entry["ensemble"]
                print(f"{'':>20} {'':>8}  {e['members']} members: CRPS depth {e['micro']['crps_depth']:.4f} m, spread / skill "
                      f"{e['micro']['spread_skill_depth']:.3f}, Brier {e['micro']['brier_return']:.4f}, best-of-K MAE {e['micro']['best_mae_depth']:.4f} m, "
                      f"consensus MAE {e['consensus']['micro']['mae_depth']:.4f} m"
                      + (f", energy depth {e['coherence']['macro']['energy_depth']:.4f} m, variogram depth "
                         f"{e['coherence']['micro']['variogram_total_depth']:.4f} m" if "coherence" in e else "")
                      + (f", occupancy Brier {e['occupancy']['all']['micro']['brier'][0]:.4f}, consensus voxel IoU "
                         f"{e['occupancy']['all']['micro']['consensus_iou'][0]:.4f} at {e['occupancy']['sizes'][0]:g} m" if "occupancy" in e else ""))
    print(f"{len(files)} scans -> {args.out}")
    return doc


DPMPP_DEFAULTS = {"dpmpp_eta": 1.0, "dpmpp_order": 2, "dpmpp_init": "none", "dpmpp_t_start": 1.0}


def dpmpp_settings(args):
    """the dpmpp method's settings of parsed arguments, the defaults where an option was not given"""
    return {name: getattr(args, name, default) for name, default in DPMPP_DEFAULTS.items()}


def parse_offsets(text):
    """``"0,1 0,2 1,0"`` -> ((0, 1), (0, 2), (1, 0)); ValueError for anything else"""
    out = []
    for item in str(text).split():
        parts = item.split(",")
        if len(parts) != 2:
            raise ValueError(f"an offset is dh,dw, got {item!r}")
        out.append((int(parts[0]), int(parts[1])))
    return tuple(out)


def coherence_settings(parser, args):
    """the keyword arguments of ``evaluate_completion`` behind --ensemble_coherence / --coherence_offsets: none when the option is not given"""
    on, offsets = hasattr(args, "ensemble_coherence"), getattr(args, "coherence_offsets", None)
    if (on or offsets is not None) and not hasattr(args, "ensemble"):
        parser.error("--ensemble_coherence scores the members of an ensemble: give --ensemble K as well")
    if offsets is not None and not on:
        parser.error("--coherence_offsets goes with --ensemble_coherence")
    if not on:
        return {}
    try:
        return {"ensemble_coherence": True, "coherence_offsets": None if offsets is None else parse_offsets(offsets)}
    except ValueError as e:
        parser.error(f"--coherence_offsets: {e}")


def build_parser():
    parser = ArgumentParser()
    parser.add_argument("--ckpt", type=Path, required=True)
    parser.add_argument("--real_scans", type=str, default=None, help="a directory tree of raw Velodyne *.bin scans, projected here")
    parser.add_argument("--real_dir", type=str, default=None, help="a directory of (5,H,W) scans in the sample layout (*.pth)")
    parser.add_argument("--limit", type=int, default=None, help="the first so many scans (sorted)")
    parser.add_argument("--corruption", action="append", default=None, metavar="KIND",
                        help="full, beams:K, random_beams:P or random_points:P; repeatable (default: beams:4)")
    parser.add_argument("--methods", nargs="+", choices=["repaint", "ddnm", "dpmpp", "nearest", "linear"], default=["repaint"],
                        help="ddnm: the data-consistent sampler (ddpm.complete), one denoiser call per step; dpmpp: the same projection on "
                             "DPM-Solver++(2M) (ddpm.complete_dpm), use it with --num_steps 16 to 32")
    parser.add_argument("--num_steps", type=int, default=32)
    parser.add_argument("--num_resample_steps", type=int, default=10)
    parser.add_argument("--jump_length", type=int, default=1)
    parser.add_argument("--ddnm_resample_steps", type=int, default=1, help="resamplings per step of the ddnm method (1: none)")
    parser.add_argument("--ddnm_init", choices=("none", "nearest", "linear"), default="none",
                        help="start the ddnm method from this interpolation of the known beams, noised to --ddnm_t_start (masks of whole rows)")
    parser.add_argument("--ddnm_t_start", type=float, default=1.0, help="the noise level the ddnm method starts at (< 1 needs --ddnm_init)")
    # (the dpmpp method's settings are attributes of the parsed arguments only when given: ``dpmpp_settings`` fills in DPMPP_DEFAULTS)
    parser.add_argument("--dpmpp_eta", type=float, default=SUPPRESS,
                        help="the dpmpp method's share of fresh noise per step (default 1: SDE-DPM-Solver++(2M); 0: deterministic)")
    parser.add_argument("--dpmpp_order", type=int, choices=(1, 2), default=SUPPRESS, help="the dpmpp method's solver order (default 2)")
    parser.add_argument("--dpmpp_init", choices=("none", "nearest", "linear"), default=SUPPRESS,
                        help="start the dpmpp method from this interpolation of the known beams, noised to --dpmpp_t_start (masks of whole rows; default none)")
    parser.add_argument("--dpmpp_t_start", type=float, default=SUPPRESS,
                        help="the noise level the dpmpp method starts at (default 1; < 1 needs --dpmpp_init)")
    parser.add_argument("--batch_size", type=int, default=8, help="scans per RePaint call")
    parser.add_argument("--seed", type=int, default=0, help="scan i draws its masks and its noise from generators seeded from (seed, i)")
    parser.add_argument("--rangenet_weights", type=str, default=None,
                        help="the official darknet53-1024.tar.gz archive or a .pth state dict (a local file): adds per-class IoU and mIoU")
    parser.add_argument("--semseg_postprocess", choices=("none", "knn", "crf", "crf_knn"), default="none",
                        help="refine the labels of both images: the kNN vote of RangeNet++, the CRF-RNN of SqueezeSeg, or the CRF-RNN and then the vote")
    parser.add_argument("--chamfer", action="store_true",
                        help="also Chamfer distance and F-score of the completed scan's points against the real scan's, whole image and inpainted pixels")
    parser.add_argument("--fscore_threshold", type=float, default=0.2, help="the F-score's distance threshold in metres (with --chamfer)")
    parser.add_argument("--voxel_iou", type=float, nargs="+", default=SUPPRESS, metavar="S",  # (an attribute of the parsed arguments only when given)
                        help="also the voxel occupancy IoU, precision, recall and F1 of the same clouds at these voxel sizes in metres (1 to 8, e.g. 0.1 0.2); "
                             "with --ensemble K (at most 63 then) also the members' occupancy vote: Brier score, consensus IoU, reliability curve")
    parser.add_argument("--ensemble", type=int, default=SUPPRESS, metavar="K",  # (an attribute of the parsed arguments only when given)
                        help="draw K members per scan with every stochastic method and score them as an ensemble: CRPS, rank histogram, "
                             "spread against skill, Brier score of ray drop, best-of-K, the consensus scan (--save_dir keeps the per-pixel maps)")
    parser.add_argument("--ensemble_coherence", action="store_true", default=SUPPRESS,  # (attributes only when given, as --ensemble)
                        help="with --ensemble: also the energy score and the variogram score of the members across pixels (a draw's spatial coherence)")
    parser.add_argument("--coherence_offsets", type=str, default=SUPPRESS, metavar='"DH,DW ..."',
                        help='the pixel offsets of the variogram score, e.g. "0,1 0,2 1,0" (default: r2dm_amd.completion.DEFAULT_OFFSETS)')
    parser.add_argument("--save_dir", type=Path, default=None, help="also write the tensors behind the numbers, one .pt file per corruption")
    parser.add_argument("--out", type=str, default="completion.json")
    return parser


if __name__ == "__main__":
    main()
