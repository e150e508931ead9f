"""r2dm_amd -- MI355X-native R2DM sampler (DDPM/DDIM reverse process over the Efficient U-Net).

Drop-in for the sampling API of kazuto1011/r2dm; the per-step hot path runs as hand-written HIP
kernels (``libr2dm_hip.so``, C ABI in ``include/r2dm_hip.h``).  There is no CPU fallback.
"""
from .diffusion import ContinuousTimeGaussianDiffusion, DiscreteTimeGaussianDiffusion, GaussianDiffusion
from .inference import setup_model, setup_rng
from .lidar import LiDARUtility
from .option import Config
from .unet import EfficientUNet
from . import metrics  # noqa: E402  (BEV metrics of evaluate.py)
from . import projection  # noqa: E402  (raw scans -> range images)
from .projection import known_from_scan, load_points_as_images, load_scans, parse_projection, project_scans
from . import pointcloud  # noqa: E402  (range images -> point clouds)
from .pointcloud import centred_ray_angles, images_to_points, save_ply, save_scans, scan_row_start
from . import pointnet  # noqa: E402  (PointNet features of the FPD)
from .pointnet import pointnet_features, pretrained_pointnet
from . import rangenet  # noqa: E402  (RangeNet features of the FRD, segmentation labels)
from .rangenet import pretrained_rangenet
from . import postproc  # noqa: E402  (kNN vote and CRF-RNN refinement of the labels)
from .postproc import CRFRNN, KNN
from . import loss  # noqa: E402  (the denoising loss over noise levels)
from .loss import loss_curve
from . import completion  # noqa: E402  (completion metrics: range / reflectance error, IoU, interpolation baselines)
from .completion import (aggregate_coherence, aggregate_ensemble, completion_errors, confusion_matrix, corruption_mask, ensemble_coherence,
                         ensemble_consensus, ensemble_scores, evaluate_completion, fill_beams, iou_from_confusion, member_seed)
from . import geometry  # noqa: E402  (Chamfer distance, F-score, COV / MMD / 1-NNA on a HIP nearest-neighbour search)
from .geometry import chamfer_from_sums, chamfer_sums, emd_pairs, nearest_neighbors, pairwise_chamfer, pairwise_emd, set_metrics
from .geometry import occupancy_from_counts, voxel_from_counts, voxel_iou, voxel_occupancy_counts
from . import latent  # noqa: E402  (DDIM inversion's transfer kernel, slerp, latent interpolation and reconstruction)
from .latent import ddim_transfer, interpolate, reconstruct, slerp

__all__ = [
    "ContinuousTimeGaussianDiffusion", "DiscreteTimeGaussianDiffusion", "GaussianDiffusion", "EfficientUNet",
    "LiDARUtility", "Config", "setup_model", "setup_rng",
    "load_scans", "project_scans", "load_points_as_images", "parse_projection", "known_from_scan",
    "images_to_points", "save_scans", "save_ply", "scan_row_start", "centred_ray_angles",
    "pretrained_pointnet", "pointnet_features", "pretrained_rangenet",
    "KNN", "CRFRNN", "loss_curve",
    "corruption_mask", "completion_errors", "confusion_matrix", "iou_from_confusion", "fill_beams", "evaluate_completion",
    "ensemble_scores", "ensemble_consensus", "aggregate_ensemble", "member_seed",
    "ensemble_coherence", "aggregate_coherence",
    "nearest_neighbors", "chamfer_sums", "chamfer_from_sums", "pairwise_chamfer", "set_metrics",
    "emd_pairs", "pairwise_emd",
    "voxel_iou", "voxel_occupancy_counts", "voxel_from_counts", "occupancy_from_counts",
    "ddim_transfer", "slerp", "interpolate", "reconstruct",
]
__version__ = "0.4.0"
