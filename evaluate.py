#!/usr/bin/env python3
"""Drop-in for the reference's evaluation script (evaluate.py): scores a directory of generated
``samples_*.pth`` files (sample_and_save.py's (5,H,W) [depth, x, y, z, reflectance] tensors) against a real set with the
bird's-eye-view JSD and MMD of metrics/bev.py and, given the PointNet / RangeNet-53 weights, the FPD / FRD (Frechet distance and
squared MMD of PointNet / RangeNet features, metrics/distribution.py), on the GPU (r2dm_amd.metrics, r2dm_amd.pointnet,
r2dm_amd.rangenet).

Same CLI (``--ckpt``, ``--sample_dir``, ``--dataset``, ``--batch_size``, ``--num_workers``) and the same output file,
``{sample_dir}_{timestamp}.json``.  The real set comes from either
  - the reference's own cache pickle ``real_set_{dataset}_{projection}_{H}x{W}_{split}.pkl`` (its ``bev_hists``), looked for
    in the working directory under that name as the reference writes it, or given with ``--real_set PATH``; or
  - ``--real_dir DIR``: a directory of (5,H,W) scans in the sample layout, histogrammed here; or
  - ``--real_scans DIR``: a directory tree of raw Velodyne ``*.bin`` scans (KITTI-360's ``data_3d_raw``, say), projected here on the
    GPU (r2dm_amd.projection) with the checkpoint's ``cfg.data.projection`` and resized to ``cfg.data.resolution`` as the reference's
    dataset and evaluate.py do, ``--batch_size`` scans at a time.
The HuggingFace dataset builders are not used.

``--pointnet_weights PATH`` (SpareNet's ``cls_model_39.pth``, the file the reference downloads; nothing is downloaded here) adds
``pts.frechet_distance`` and ``pts.squared_mmd``: the generated features come from the batches that feed the BEV histograms, the real
ones from the cache pickle's ``pts_feats`` or from the ``--real_dir`` / ``--real_scans`` batches; all real features are used.  The
subsets of the squared MMD are drawn from numpy's global state as in the reference, or from ``--mmd_seed``.

``--rangenet_weights PATH`` (the official ``darknet53-1024.tar.gz`` archive the reference downloads, or a ``.pth`` state dict in its
module layout; a local file, nothing is downloaded here) adds ``img.frechet_distance`` and ``img.squared_mmd`` when the checkpoint
was trained with reflectance, as in the reference: the "lidargen" features of RangeNet-53 over the same batches, the real ones from
the cache pickle's ``img_feats`` or from the ``--real_dir`` / ``--real_scans`` batches."""
import datetime
import json
import pickle
import random
from argparse import ArgumentParser
from pathlib import Path

import numpy as np
import torch

# from LiDARGen (reference evaluate.py:19-22)
MAX_DEPTH = 63.0
MIN_DEPTH = 0.5
MAX_SAMPLES = 10_000


def sample_files(root, limit=MAX_SAMPLES):
    """The first ``limit`` sorted ``*.pth`` files of ``root`` (the reference's Samples dataset)."""
    return sorted(Path(root).glob("*.pth"))[:limit]


def load_batches(files, batch_size, num_workers):
    """(B,5,H,W) fp32 batches of the files, read by a DataLoader as the reference does."""

    class Files(torch.utils.data.Dataset):
        def __len__(self):
            return len(files)

        def __getitem__(self, i):
            img = torch.load(files[i], map_location="cpu")
            assert img.shape[0] == 5, img.shape
            return img.float()

    return torch.utils.data.DataLoader(Files(), batch_size=batch_size, num_workers=num_workers)


def _measure(imgs, extractor, hists, feats, img_extractor=None, img_feats=None):
    """One (B,5,H,W) batch on the GPU: its BEV histograms and, with the extractors, its PointNet and RangeNet features
    (evaluate.py:142-160)."""
    from r2dm_amd import metrics, pointnet

    hists.append(metrics.bev_histograms(imgs, image_min_depth=MIN_DEPTH, image_max_depth=MAX_DEPTH))
    if extractor is not None:
        feats.append(pointnet.pointnet_features(extractor, imgs))
    if img_extractor is not None:
        img_feats.append(img_extractor.extract(imgs, feature="lidargen", image_min_depth=MIN_DEPTH, image_max_depth=MAX_DEPTH))


def _measured(hists, feats, img_feats, extractor, img_extractor):
    """(histograms, PointNet features or None), and as a third value the RangeNet features when there is an ``img_extractor``."""
    out = (torch.cat(hists), torch.cat(feats) if extractor is not None else None)
    return out if img_extractor is None else out + (torch.cat(img_feats),)


def _split(measured):
    """(histograms, PointNet features or None, RangeNet features or None) of what ``histograms_of`` / ``histograms_of_scans`` returned"""
    return measured if len(measured) == 3 else (*measured, None)


def histograms_of(files, batch_size, num_workers, device, extractor=None, img_extractor=None):
    """int32 (N,100,100) BEV histograms of the sample files: depth mask, then point_cloud_to_histogram (evaluate.py:22-41,145-155);
    with ``extractor`` also the (N,1808) PointNet features of the same batches (else None); with ``img_extractor`` a third value, the
    (N,4096) RangeNet features."""
    if not files:
        raise SystemExit("no *.pth files to evaluate")
    hists, feats, img_feats = [], [], []
    for imgs in load_batches(files, batch_size, num_workers):
        _measure(imgs.to(device, non_blocking=True), extractor, hists, feats, img_extractor, img_feats)
    return _measured(hists, feats, img_feats, extractor, img_extractor)


def scan_files(root):
    """All ``*.bin`` files below ``root``, sorted."""
    return sorted(Path(root).rglob("*.bin"))


def histograms_of_scans(files, cfg, batch_size, device, extractor=None, img_extractor=None):
    """int32 (N,100,100) BEV histograms of raw scans: the dataset builder's projection (64 rows, the projection's own width, masked by
    its depth window), evaluate.py's resize to the model's resolution (nearest-exact), then the depth mask and histogram as above;
    with ``extractor`` also the PointNet features of the same images (else None); with ``img_extractor`` a third value, their RangeNet
    features."""
    import torch.nn.functional as F

    from r2dm_amd import projection

    if not files:
        raise SystemExit("no *.bin files below --real_scans")
    unfolding, width = projection.parse_projection(cfg.data.projection)
    H, W = cfg.data.resolution
    hists, feats, img_feats = [], [], []
    for k in range(0, len(files), batch_size):
        points, offsets = projection.load_scans(files[k:k + batch_size])
        imgs = projection.project_scans(points, offsets, H=64, W=width, scan_unfolding=unfolding, apply_mask=True,
                                        out_width=W if W <= width else None, layout="sample", device=device)
        if tuple(imgs.shape[-2:]) != (H, W):
            imgs = F.interpolate(imgs, size=(H, W), mode="nearest-exact")
        _measure(imgs, extractor, hists, feats, img_extractor, img_feats)
    return _measured(hists, feats, img_feats, extractor, img_extractor)


def real_cache_name(cfg, split):
    H, W = cfg.data.resolution
    return f"real_set_{cfg.data.dataset}_{cfg.data.projection}_{H}x{W}_{split}.pkl"


@torch.no_grad()
def evaluate(args):
    from r2dm_amd import metrics
    from r2dm_amd.option import Config

    device = torch.device("cuda")
    ckpt = torch.load(args.ckpt, map_location="cpu")
    cfg = Config(**ckpt["cfg"])

    extractor = None
    if getattr(args, "pointnet_weights", None) is not None:
        from r2dm_amd import pointnet

        extractor = pointnet.pretrained_pointnet(args.pointnet_weights, device=device)

    img_extractor = None  # (the reference computes the FRD only for a model with reflectance: evaluate.py:108,145)
    frd_asked = getattr(args, "rangenet_weights", None) is not None
    if frd_asked and cfg.data.train_reflectance:
        from r2dm_amd import rangenet

        img_extractor = rangenet.pretrained_rangenet(args.rangenet_weights, device=device)
    more = () if img_extractor is None else (img_extractor,)
    real_img = None

    results = dict(img=dict(), pts=dict(), bev=dict(), info=dict())
    results["info"]["phase"] = args.dataset
    results["info"]["directory"] = args.sample_dir

    # real set: the reference's cache, or a directory of scans
    if args.real_scans is not None:
        real_hists, real_feats, real_img = _split(histograms_of_scans(scan_files(args.real_scans), cfg, args.batch_size, device, extractor, *more))
        results["info"]["real"] = str(args.real_scans)
    elif args.real_dir is not None:
        real_hists, real_feats, real_img = _split(histograms_of(sample_files(args.real_dir, limit=None), args.batch_size, args.num_workers, device,
                                                                extractor, *more))
        results["info"]["real"] = str(args.real_dir)
    else:
        path = Path(args.real_set) if args.real_set is not None else Path(real_cache_name(cfg, args.dataset))
        if not path.exists():
            raise SystemExit(f"no real set: {path} not found (run the reference's evaluate.py once to cache it, or give "
                             "--real_set PATH / --real_dir DIR / --real_scans DIR)")
        print(f"found cached {path}")
        with open(path, "rb") as f:
            real_set = pickle.load(f)
        real_hists = torch.from_numpy(np.ascontiguousarray(real_set["bev_hists"])).to(device)
        real_feats = None
        if extractor is not None:  # the reference's own PointNet features of the real set
            real_feats = torch.from_numpy(np.ascontiguousarray(real_set["pts_feats"], dtype=np.float32)).to(device)
        if img_extractor is not None:  # ... and its RangeNet features
            real_img = torch.from_numpy(np.ascontiguousarray(real_set["img_feats"], dtype=np.float32)).to(device)
        results["info"]["real"] = str(path)
    results["info"]["#real"] = len(real_hists)

    # generated set
    gen_hists, gen_feats, gen_img = _split(histograms_of(sample_files(args.sample_dir), args.batch_size, args.num_workers, device, extractor, *more))
    results["info"]["#fake"] = len(gen_hists)

    # the real subset as the reference takes it (evaluate.py:185-187)
    perm = list(range(len(real_hists)))
    random.Random(0).shuffle(perm)
    perm = perm[:MAX_SAMPLES]
    real_sub = real_hists[torch.tensor(perm, device=device)]

    results["bev"]["jsd"] = metrics.compute_jsd_2d(real_sub, gen_hists)
    results["bev"]["mmd"] = metrics.compute_mmd_2d(real_sub, gen_hists)
    seed = getattr(args, "mmd_seed", None)
    rng = lambda: None if seed is None else np.random.RandomState(seed)
    if img_extractor is not None:  # all real features, as the reference (evaluate.py:174-180)
        results["img"]["frechet_distance"] = metrics.compute_frechet_distance(real_img, gen_img)
        results["img"]["squared_mmd"] = metrics.compute_squared_mmd(real_img, gen_img, rng=rng())
    if extractor is not None:  # (evaluate.py:182-187)
        results["pts"]["frechet_distance"] = metrics.compute_frechet_distance(real_feats, gen_feats)
        results["pts"]["squared_mmd"] = metrics.compute_squared_mmd(real_feats, gen_feats, rng=rng())
    prdc_k = getattr(args, "prdc_k", None)
    if prdc_k is not None:  # extension: the k-NN manifold metrics of each computed feature group, the real side bounded like the BEV subset
        sub = torch.tensor(perm, device=device)
        for group, real_f, gen_f in (("img", real_img, gen_img), ("pts", real_feats, gen_feats)):
            if real_f is not None and gen_f is not None:
                results[group].update(metrics.manifold_metrics(real_f[sub], gen_f, k=prdc_k))
        results["info"]["prdc_k"] = prdc_k
        results["info"]["prdc_#real"] = len(perm)
    if frd_asked and img_extractor is None:  # (as in the reference, which skips the FRD for such a model)
        no_frd = "img (FRD) is not computed: the checkpoint was trained without reflectance"
        results["info"]["note"] = no_frd if extractor is not None else no_frd + "; pts (FPD) is not computed: it needs the PointNet weights"
    elif extractor is None and img_extractor is None:
        results["info"]["note"] = ("img (FRD) and pts (FPD) are not computed: they need the RangeNet-53 and PointNet weights")
    elif img_extractor is None:
        results["info"]["note"] = "img (FRD) is not computed: it needs the RangeNet-53 weights"
    elif extractor is None:
        results["info"]["note"] = "pts (FPD) is not computed: it needs the PointNet weights"

    print(results)
    save_path = args.sample_dir + f"_{datetime.datetime.now().strftime('%Y%m%dT%H%M%S')}.json"
    with open(save_path, "w") as f:
        json.dump(results, f, indent=4)
    return save_path


def build_parser():
    parser = ArgumentParser()
    parser.add_argument("--ckpt", type=Path, required=True)
    parser.add_argument("--sample_dir", type=str, required=True)
    parser.add_argument("--dataset", choices=["train", "test", "all"], default="all")
    parser.add_argument("--batch_size", type=int, default=64)
    parser.add_argument("--num_workers", type=int, default=4)
    parser.add_argument("--real_set", type=str, default=None,
                        help="extension: the reference's real-set cache pickle (default: its own name in the working directory)")
    parser.add_argument("--real_dir", type=str, default=None,
                        help="extension: a directory of (5,H,W) real scans in the sample layout, instead of the cache")
    parser.add_argument("--real_scans", type=str, default=None,
                        help="extension: a directory tree of raw Velodyne *.bin scans, projected here with the checkpoint's projection")
    parser.add_argument("--pointnet_weights", type=str, default=None,
                        help="extension: SpareNet's cls_model_39.pth (the PointNet of the FPD); adds pts.frechet_distance / pts.squared_mmd")
    parser.add_argument("--rangenet_weights", type=str, default=None,
                        help="extension: the official darknet53-1024.tar.gz archive or a .pth state dict (the RangeNet-53 of the FRD), a local "
                             "file; adds img.frechet_distance / img.squared_mmd for a model trained with reflectance")
    parser.add_argument("--mmd_seed", type=int, default=None,
                        help="extension: seed of the squared MMD's subset draws (default: numpy's global state, as the reference)")
    parser.add_argument("--prdc_k", type=int, default=None,
                        help="extension: adds precision / recall / density / coverage (k-NN manifolds, k-th nearest other sample) to each "
                             "computed feature group, against the real subset the BEV metrics take")
    return parser


if __name__ == "__main__":
    evaluate(build_parser().parse_args())
