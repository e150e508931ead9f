"""ctypes binding of libr2dm_hip.so (C ABI: include/r2dm_hip.h).

There is NO fallback: if the shared library is missing, or a tensor is not on a ROCm device,
every entry point raises.  PyTorch only owns memory and streams here.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int32, c_int64, c_size_t, c_void_p
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("R2DM_HIP_LIB", os.path.join(_HERE, "libr2dm_hip.so"))


class R2DMError(RuntimeError):
    pass


class R2DMRangeError(R2DMError):
    """The fp16-operand paths' range guard tripped (r2dm_check_range): results of the forwards since the last check are not valid."""


class R2DMRangeFallback(R2DMRangeError):
    """The guard tripped at the end of a loop that cannot replay itself (a hand-written ``p_step`` loop under
    ``deferred_range_check``): the denoiser has switched to the wide-range operand split, the loop's results are not valid, and
    repeating the call gives them (``repaint`` does that itself, from the saved generator states)."""


class Config(Structure):
    _fields_ = [
        ("in_channels", c_int32),
        ("out_channels", c_int32),
        ("height", c_int32),
        ("width", c_int32),
        ("base_channels", c_int32),
        ("temb_channels", c_int32),
        ("channel_multiplier", c_int32 * 4),
        ("num_residual_blocks", c_int32 * 4),
        ("gn_num_groups", c_int32),
        ("gn_eps", c_float),
        ("attn_num_heads", c_int32),
        ("coord_channels", c_int32),
        ("max_batch", c_int32),
    ]


class TensorInfo(Structure):
    _fields_ = [("key", c_char_p), ("numel", c_int64)]


# name -> (restype, argtypes); exactly the symbols include/r2dm_hip.h declares
_P = c_void_p
SIGNATURES = {
    "r2dm_last_error": (c_char_p, []),
    "r2dm_version": (c_char_p, []),
    "r2dm_create": (c_int32, [POINTER(c_void_p), POINTER(Config)]),
    "r2dm_destroy": (None, [_P]),
    "r2dm_num_tensors": (c_int64, [_P]),
    "r2dm_tensor_at": (c_int32, [_P, c_int64, POINTER(TensorInfo)]),
    "r2dm_blob_bytes": (c_size_t, [_P]),
    "r2dm_blob_flag_region": (c_int32, [_P, POINTER(c_size_t), POINTER(c_size_t)]),
    "r2dm_blob_cmap_region": (c_int32, [_P, POINTER(c_size_t), POINTER(c_size_t)]),
    "r2dm_blob_layout_hash": (ctypes.c_uint64, [_P]),
    "r2dm_bind_blob": (c_int32, [_P, _P, c_size_t]),
    "r2dm_load_tensor": (c_int32, [_P, c_int64, _P, c_int64, _P]),
    "r2dm_workspace_bytes": (c_size_t, [_P, c_int32]),
    "r2dm_unet_forward": (c_int32, [_P, _P, _P, _P, c_int32, _P, c_size_t, _P]),
    "r2dm_forward_listing": (c_int32, [_P, c_int32, _P, c_size_t, POINTER(c_size_t)]),
    "r2dm_cache_bytes": (c_size_t, [_P, c_int32, c_int32]),
    "r2dm_unet_forward_cached": (c_int32, [_P, _P, _P, _P, c_int32, _P, c_size_t, _P, _P, c_size_t, c_int32, c_int32, _P]),
    "r2dm_forward_listing_cached": (c_int32, [_P, c_int32, c_int32, c_int32, _P, c_size_t, POINTER(c_size_t)]),
    "r2dm_cache_store": (c_int32, [_P, _P, c_int32, c_int64, c_int32, _P, _P, _P]),
    "r2dm_set_conv_pieces": (c_int32, [_P, c_int32]),
    "r2dm_check_range": (c_int32, [_P, _P]),
    "r2dm_test_raise_range_bound": (c_int32, [_P, c_float, _P]),
    "r2dm_range_sites": (c_int32, [_P, POINTER(c_float), c_int32, POINTER(c_int32)]),
    "r2dm_range_site_name": (c_char_p, [_P, c_int32]),
    "r2dm_profile_enable": (c_int32, [_P, c_int32]),
    "r2dm_profile_read": (c_int32, [_P, POINTER(ctypes.c_double), POINTER(ctypes.c_double), POINTER(c_int64)]),
    "r2dm_profile_read_classes": (c_int32, [_P, POINTER(ctypes.c_double), POINTER(ctypes.c_double), POINTER(c_int64)]),
    "r2dm_profile_event_overhead": (c_int32, [_P, _P, POINTER(ctypes.c_double), POINTER(ctypes.c_double)]),
    "r2dm_posterior_step": (c_int32, [_P, _P, _P, _P, _P, c_int32, c_int64, c_int32, c_int32, c_float, _P]),
    "r2dm_posterior_step_known": (c_int32, [_P, _P, _P, _P, _P, _P, _P, c_int32, c_int64, c_int32, c_int32, c_int32, c_int32, c_float, _P]),
    "r2dm_dpm_step": (c_int32, [_P, _P, _P, _P, _P, _P, c_int32, c_int64, c_int32, c_float, _P]),
    "r2dm_dpm_step_known": (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, _P, c_int32, c_int64, c_int32, c_int32, c_int32, c_float, _P]),
    "r2dm_repaint_blend": (c_int32, [_P, _P, _P, _P, _P, _P, c_int32, c_int64, c_int32, c_int32, _P]),
    "r2dm_q_step": (c_int32, [_P, _P, _P, _P, c_int32, c_int64, _P]),
    "r2dm_diffusion_loss_scratch_bytes": (c_size_t, [c_int32, c_int32, c_int64]),
    "r2dm_diffusion_loss": (c_int32, [_P, _P, _P, _P, c_int32, _P, c_int32, c_int32, c_int32, c_int32, c_int64, _P, _P, _P, _P]),
    "r2dm_ddim_transfer": (c_int32, [_P, _P, _P, _P, c_int32, c_int64, c_int32, _P]),
    "r2dm_slerp_scratch_bytes": (c_size_t, [c_int32, c_int64]),
    "r2dm_slerp": (c_int32, [_P, _P, POINTER(c_float), c_int32, _P, _P, c_int32, c_int64, _P, _P]),
    "r2dm_lidar_postprocess": (c_int32, [_P, _P, _P, c_int32, c_int32, c_int32, c_float, c_float, _P]),
    "r2dm_lidar_postprocess_fmt": (c_int32, [_P, _P, _P, c_int32, c_int32, c_int32, c_float, c_float, c_int32, _P]),
    "r2dm_conv_packed_elems": (c_int64, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32]),
    "r2dm_conv2d_ring": (c_int32, [_P, _P, _P, _P, _P, c_int32, _P, _P, _P, c_int32, c_int32, c_int32, c_int32,
                                   c_int32, c_int32, _P]),
    "r2dm_conv_stat_slots": (c_int32, [c_int32, c_int32]),
    "r2dm_conv2d_ring_ex": (c_int32, [_P, _P, c_int32, _P, _P, _P, _P, c_int32, _P, c_int32, _P, _P, _P, c_int32, c_int32, c_int32, _P, c_int32,
                                      _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P]),
    "r2dm_group_norm_scratch_bytes": (c_size_t, [c_int32, c_int32]),
    "r2dm_group_norm_affine": (c_int32, [_P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32,
                                         c_float, _P]),
    "r2dm_affine_act": (c_int32, [_P, _P, _P, c_int32, c_int32, c_int64, c_int32, _P]),
    "r2dm_group_norm_from_stats": (c_int32, [_P, c_int32, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_float, _P]),
    "r2dm_fir_down2": (c_int32, [_P, _P, c_int32, c_int32, c_int32, c_int32, _P]),
    "r2dm_fir_down2_stat_slots": (c_int32, [c_int32, c_int32, c_int32, c_int32]),
    "r2dm_fir_down2_stats": (c_int32, [_P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, _P]),
    "r2dm_fir_up2": (c_int32, [_P, _P, c_int32, c_int32, c_int32, c_int32, _P]),
    "r2dm_down_planes": (c_int32, [_P, _P, c_int32, c_int32, c_int32, c_int32, _P]),
    "r2dm_down_gemm_stat_slots": (c_int32, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    "r2dm_down_gemm": (c_int32, [_P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P]),
    "r2dm_down_gemm_nine": (c_int32, [_P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P]),
    "r2dm_down_phase_planes": (c_int32, [_P, _P, c_int32, c_int32, c_int32, c_int32, _P]),
    "r2dm_down_phase_planes_floats": (c_int64, [c_int32, c_int32, c_int32]),
    "r2dm_group_norm_affine_ex": (c_int32, [_P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_float, _P, _P]),
    "r2dm_group_norm_from_stats_ex": (c_int32, [_P, c_int32, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_float, _P, _P]),
    "r2dm_group_norm_from_stats_strided": (c_int32, [_P, c_int32, _P, _P, _P, c_int64, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_float, _P, _P]),
    "r2dm_fir_up2_ex": (c_int32, [_P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "r2dm_down_planes_ex": (c_int32, [_P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "r2dm_down_phase_planes_ex": (c_int32, [_P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "r2dm_attention": (c_int32, [_P, _P, c_int32, c_int32, c_int32, c_int32, _P]),
    "r2dm_time_embedding": (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, _P]),
    "r2dm_ada_proj": (c_int32, [_P, _P, _P, _P, c_int32, c_int32, c_int32, _P]),
    "r2dm_bev_histogram": (c_int32, [_P, c_int32, _P, _P, _P, c_int32, c_int64, c_int32, c_float, c_float, c_float, c_float,
                                     _P]),
    "r2dm_bev_hist_sum": (c_int32, [_P, c_int32, _P, c_int64, c_int64, _P]),
    "r2dm_bev_mmd_scratch_bytes": (c_size_t, [c_int32, c_int32]),
    "r2dm_bev_mmd": (c_int32, [_P, _P, c_int32, c_int32, c_int64, ctypes.c_double, _P, c_size_t, _P, _P]),
    "r2dm_pointnet_packed_bytes": (c_size_t, [c_int32, c_int32]),
    "r2dm_pointnet_pack": (c_int32, [_P, c_int32, c_int32, _P, _P, _P, _P]),
    "r2dm_pointnet_scratch_bytes": (c_size_t, [c_int32]),
    "r2dm_pointnet_trunk": (c_int32, [_P, c_int32, c_int32, c_int64, _P, c_float, c_float, c_float, _P, _P, _P, _P, _P, _P, c_size_t, _P, _P]),
    "r2dm_pointnet_head": (c_int32, [_P, _P, _P, c_int32, _P, _P, _P, _P, _P, _P, c_int32, _P, c_int32, _P]),
    "r2dm_rangenet_packed_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "r2dm_rangenet_pack": (c_int32, [_P, c_int32, c_int32, c_int32, _P, _P, _P, _P]),
    "r2dm_rangenet_conv": (c_int32, [_P, _P, _P, c_float, c_float, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                     c_float, _P, _P]),
    "r2dm_rangenet_argmax": (c_int32, [_P, _P, c_int32, c_int32, c_int64, _P]),
    "r2dm_feature_moments": (c_int32, [_P, c_int64, c_int32, _P, _P, _P]),
    "r2dm_poly_mmd_scratch_bytes": (c_size_t, [c_int32, c_int32]),
    "r2dm_poly_mmd": (c_int32, [_P, _P, _P, _P, c_int32, c_int32, c_int32, _P, c_size_t, _P, _P]),
    "r2dm_feature_knn_scratch_bytes": (c_size_t, [c_int64, c_int64, c_int32, c_int32]),
    "r2dm_feature_knn": (c_int32, [_P, c_int64, _P, c_int64, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, _P, c_size_t, _P, POINTER(c_int32), _P]),
    "r2dm_colorize": (c_int32, [_P, _P, _P, c_int64, c_int64, _P]),
    "r2dm_rasterize_scratch_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "r2dm_bilinear_rasterize": (c_int32, [_P, _P, _P, c_int32, c_int64, c_int32, c_int32, c_int32, _P, c_size_t, c_int32, _P]),
    "r2dm_project_points": (c_int32, [_P, _P, POINTER(c_float), c_float, c_int32, _P, _P, c_int64, _P]),
    "r2dm_render_frames_scratch_bytes": (c_size_t, [c_int32, c_int32]),
    "r2dm_render_frames": (c_int32, [_P, _P, _P, _P, _P, _P, c_int64, c_int32, c_int32, c_int32, c_float, c_float, POINTER(c_float), c_float,
                                     _P, c_size_t, _P]),
    "r2dm_surface_normals": (c_int32, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, _P]),
    "r2dm_normal_frames_scratch_bytes": (c_size_t, [c_int32, c_int32]),
    "r2dm_normal_frames": (c_int32, [_P, _P, _P, _P, c_int64, c_int32, c_int32, c_int32, c_float, c_float, c_int32, c_int32, POINTER(c_float), c_float,
                                     _P, c_size_t, _P]),
    "r2dm_project_scratch_bytes": (c_size_t, [c_int64, c_int32, c_int32, c_int32, c_int32]),
    "r2dm_project_scans": (c_int32, [_P, POINTER(c_int64), _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_float, c_float, c_int32, c_int32,
                                     _P, c_size_t, _P]),
    "r2dm_unproject_scratch_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "r2dm_unproject": (c_int32, [_P, c_int32, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_float, c_float, c_int32, c_float, c_float,
                                 _P, c_size_t, _P]),
    "r2dm_knn_vote": (c_int32, [_P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_float, _P, _P]),
    "r2dm_crf_iter": (c_int32, [_P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P]),
    "r2dm_completion_error_scratch_bytes": (c_size_t, [c_int32, c_int64]),
    "r2dm_completion_error": (c_int32, [_P, _P, _P, c_float, c_float, c_int32, c_int64, _P, _P, _P]),
    "r2dm_ensemble_score_scratch_bytes": (c_size_t, [c_int32, c_int32, c_int64]),
    "r2dm_ensemble_score": (c_int32, [_P, _P, _P, c_float, c_float, c_int32, c_int32, c_int64, _P, _P, _P, _P, _P, _P]),
    "r2dm_ensemble_coherence_scratch_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    "r2dm_ensemble_coherence": (c_int32, [_P, _P, _P, c_float, c_float, c_int32, c_int32, c_int32, c_int32, _P, c_int32, _P, _P, _P, _P, _P]),
    "r2dm_confusion_matrix": (c_int32, [_P, _P, _P, c_int32, c_int64, c_int32, _P, _P, _P]),
    "r2dm_fill_beams": (c_int32, [_P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_float, c_int32, _P]),
    "r2dm_nn_pairs_scratch_bytes": (c_size_t, [c_int64, c_int64]),
    "r2dm_nn_pairs": (c_int32, [_P, _P, c_int64, c_int64, _P, _P, c_int64, c_int64, _P, c_int64, c_int64, ctypes.c_double, _P, _P, _P, _P, _P, _P, _P,
                                _P, _P, _P]),
    "r2dm_voxel_occupancy_scratch_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "r2dm_voxel_occupancy": (c_int32, [_P, _P, c_int64, c_int64, _P, _P, c_int64, c_int64, _P, _P, c_int64, c_int64, POINTER(c_float), c_int64, c_int64,
                                       _P, _P, _P, _P, _P]),
    "r2dm_emd_max_points": (c_int64, []),
    "r2dm_emd_pairs_scratch_bytes": (c_size_t, [c_int64, c_int64]),
    "r2dm_emd_pairs": (c_int32, [_P, _P, c_int64, c_int64, _P, _P, c_int64, c_int64, _P, c_int64, c_int64, ctypes.c_double, c_int64, _P, _P, _P, _P, _P,
                                 _P]),
}

_lib: Optional[ctypes.CDLL] = None


def lib() -> ctypes.CDLL:
    """Load (once) and type the shared library.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise R2DMError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or r2dm_amd/csrc/build.sh). r2dm_amd has no CPU / PyTorch fallback.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise R2DMError(lib().r2dm_last_error().decode(errors="replace"))


def require_gpu(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise R2DMError(
            f"{what} is on {t.device}: r2dm_amd runs the sampling path only as HIP kernels on an MI355X "
            "(device 'cuda' under PyTorch-ROCm) and has no CPU fallback")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def f32c(t: torch.Tensor) -> torch.Tensor:
    """fp32 + contiguous (no copy when already so)."""
    return t.detach().to(torch.float32).contiguous()


# ---- thin functional wrappers -----------------------------------------------------------------
def posterior_step(x_t, pred, noise, coef, mode: int, objective: int, clip: float) -> torch.Tensor:
    require_gpu(x_t, "x_t")
    x_t, pred, coef = f32c(x_t), f32c(pred), f32c(coef)
    noise = None if noise is None else f32c(noise)
    out = torch.empty_like(x_t)
    B = x_t.shape[0]
    with torch.cuda.device(x_t.device):
        check(lib().r2dm_posterior_step(ptr(x_t), ptr(pred), ptr(noise), ptr(coef), ptr(out), B,
                                        x_t.numel() // B, mode, objective, float(clip), stream_ptr(x_t.device)))
    return out


def posterior_step_known(x_t, pred, noise, known, mask, coef, mode: int, objective: int, clip: float) -> torch.Tensor:
    """``posterior_step`` with the measurement written over the x_0 estimate, ``x0 = mask * known + (1 - mask) * x0``, in one launch;
    ``mask`` (B | 1, 1 | C, H, W) is expanded over the batch as in ``repaint_blend``."""
    require_gpu(x_t, "x_t")
    x_t, pred, noise, known, coef = f32c(x_t), f32c(pred), f32c(noise), f32c(known), f32c(coef)
    if x_t.dim() < 3 or any(t.shape != x_t.shape or t.device != x_t.device for t in (pred, noise, known)) or coef.shape != (x_t.shape[0], 8) \
            or coef.device != x_t.device:
        raise ValueError(f"x_t {tuple(x_t.shape)}, prediction {tuple(pred.shape)}, noise {tuple(noise.shape)} and known {tuple(known.shape)} must have "
                         f"one (B,C,...) shape on one device, coef {tuple(coef.shape)} must be (B,8)")
    B, C = x_t.shape[0], x_t.shape[1]
    mask = f32c(mask.to(x_t.device).expand(B, -1, *x_t.shape[2:]))
    out = torch.empty_like(x_t)
    with torch.cuda.device(x_t.device):
        check(lib().r2dm_posterior_step_known(ptr(x_t), ptr(pred), ptr(noise), ptr(known), ptr(mask), ptr(coef), ptr(out), B,
                                              x_t.numel() // B, C, mask.shape[1], mode, objective, float(clip), stream_ptr(x_t.device)))
    return out


def dpm_step(x_t, pred, x0_prev, coef, objective: int, clip: float, x0_out: Optional[torch.Tensor] = None):
    """One DPM-Solver++(2M) update (``r2dm_dpm_step``) -> ``(x_s, x0)``: ``x0`` the clamped estimate of x_0 (``posterior_step``'s), ``x_s =
    c_x x_t + c_0 x0`` with ``x0_prev=None`` (a first-order row), else ``(c_x x_t + c_0 x0) + c_1 x0_prev``; ``coef`` (B,8) = (alpha_t, sigma_t,
    c_x, c_0, c_1, 0, 0, 0).  ``x0_out``: a float32 contiguous buffer of ``x_t``'s shape to write ``x0`` into (it may be ``x0_prev`` itself); None: a new one.
    Operands of any (B,...) shape: without a measurement there are no channels to speak of."""
    return dpm_step_known(x_t, pred, x0_prev, None, None, None, coef, objective, clip, x0_out, _entry="r2dm_dpm_step")


def dpm_step_known(x_t, pred, x0_prev, noise, known, mask, coef, objective: int, clip: float, x0_out: Optional[torch.Tensor] = None,
                   _entry: str = "r2dm_dpm_step_known"):
    """``dpm_step`` with a measurement and a noise operand (``r2dm_dpm_step_known``) -> ``(x_s, x0)``: the clamped estimate gets ``x0 = mask *
    known + (1 - mask) * x0`` (``known`` and ``mask`` both given or both None; ``mask`` (B | 1, 1 | C, ...) is expanded over the batch as in
    ``repaint_blend``), ``x_s = c_x x_t + c_0 x0 [+ c_1 x0_prev] [+ c_z noise]``; ``coef`` (B,8) = (alpha_t, sigma_t, c_x, c_0, c_1, c_z, 0, 0).
    ``x0`` is the estimate after the projection.  ``x0_out`` as in ``dpm_step``.  (``_entry``: ``dpm_step``'s own, which takes neither.)"""
    measured = _entry == "r2dm_dpm_step_known"
    require_gpu(x_t, "x_t")
    x_t, pred, coef = f32c(x_t), f32c(pred), f32c(coef)
    x0_prev, noise, known = (None if t is None else f32c(t) for t in (x0_prev, noise, known))
    if (known is None) != (mask is None):
        raise ValueError("known and mask are given together or not at all")
    if x_t.dim() < (3 if measured else 2) or any(t is not None and (t.shape != x_t.shape or t.device != x_t.device) for t in (pred, x0_prev, noise, known, x0_out)) \
            or coef.shape != (x_t.shape[0], 8) or coef.device != x_t.device:
        raise ValueError(f"x_t {tuple(x_t.shape)}, prediction {tuple(pred.shape)}, x0_prev, noise, known and x0_out must have one "
                         f"{'(B,C,...)' if measured else '(B,...)'} shape on one device, coef {tuple(coef.shape)} must be (B,8)")
    B = x_t.shape[0]
    if mask is not None:
        mask = f32c(mask.to(x_t.device).expand(B, -1, *x_t.shape[2:]))
    if x0_out is None:
        x0_out = torch.empty_like(x_t)
    elif x0_out.dtype != torch.float32 or not x0_out.is_contiguous():
        raise ValueError("x0_out must be a contiguous float32 tensor")
    out = torch.empty_like(x_t)
    args = [ptr(x_t), ptr(pred), ptr(x0_prev), ptr(coef), ptr(out), ptr(x0_out), B, x_t.numel() // B, objective, float(clip), stream_ptr(x_t.device)]
    if measured:  # r2dm_dpm_step_known's further operands, where its signature has them
        args[3:3] = [ptr(noise), ptr(known), ptr(mask)]
        args[11:11] = [x_t.shape[1], 1 if mask is None else mask.shape[1]]
    with torch.cuda.device(x_t.device):
        check(getattr(lib(), _entry)(*args))
    return out, x0_out


def repaint_blend(known, noise, unknown, mask, coef) -> torch.Tensor:
    """mask * (known*alpha + noise*sigma) + (1 - mask) * unknown; coef (B,2) = (alpha, sigma)."""
    require_gpu(known, "known")
    known, noise, unknown, coef = f32c(known), f32c(noise), f32c(unknown), f32c(coef)
    B, C = known.shape[0], known.shape[1]
    mask = f32c(mask.to(known.device).expand(B, -1, *known.shape[2:]))
    out = torch.empty_like(known)
    with torch.cuda.device(known.device):
        check(lib().r2dm_repaint_blend(ptr(known), ptr(noise), ptr(unknown), ptr(mask), ptr(coef), ptr(out), B,
                                       known.numel() // B, C, mask.shape[1], stream_ptr(known.device)))
    return out


def q_step(x_s, noise, coef) -> torch.Tensor:
    """x_s * a_ts + std * noise; coef (B,2) = (a_ts, std)."""
    require_gpu(x_s, "x_s")
    x_s, noise, coef = f32c(x_s), f32c(noise), f32c(coef)
    out = torch.empty_like(x_s)
    B = x_s.shape[0]
    with torch.cuda.device(x_s.device):
        check(lib().r2dm_q_step(ptr(x_s), ptr(noise), ptr(coef), ptr(out), B, x_s.numel() // B, stream_ptr(x_s.device)))
    return out


OBJECTIVES = {"eps": 0, "v": 1, "x_0": 2}  # what the denoiser predicts (csrc/common.h OBJ_*): the one table, for samplers and loss alike
LOSS_CRITERIA = {"l2": 0, "l1": 1, "huber": 2}


def diffusion_loss(prediction, x_0, noise, mask, coef, objective: str, criterion: str):
    """``(num (B,C), den (B,))`` in float64: per sample and channel the sum of ``criterion(prediction - target) * mask``, and the sum of
    the mask over its own elements (``C*H*W`` for ``mask=None``) -- base.py:133-136 in one pass.  ``mask``: None, (B,1,H,W) or (B,C,H,W);
    ``coef`` (B,2) = (alpha, sigma), read for the ``v`` objective only."""
    require_gpu(prediction, "prediction")
    if objective not in OBJECTIVES:
        raise ValueError(f"invalid objective {objective}")
    if criterion not in LOSS_CRITERIA:
        raise ValueError(f"invalid criterion: {criterion}")
    if prediction.dim() < 2 or x_0.shape != prediction.shape or noise.shape != prediction.shape:
        raise ValueError(f"prediction {tuple(prediction.shape)}, x_0 {tuple(x_0.shape)} and noise {tuple(noise.shape)} must have one (B,C,...) shape")
    dev = prediction.device
    prediction, x_0, noise = f32c(prediction), f32c(x_0.to(dev)), f32c(noise.to(dev))
    B, C = prediction.shape[:2]
    plane = prediction.numel() // max(B * C, 1)
    mask_c = 0
    if mask is not None:
        if mask.dim() != prediction.dim() or mask.shape[0] != B or mask.shape[1] not in (1, C) or mask.shape[2:] != prediction.shape[2:]:
            raise ValueError(f"loss_mask {tuple(mask.shape)} must be (B,1,...) or (B,C,...) of prediction {tuple(prediction.shape)}")
        mask, mask_c = f32c(mask.to(dev)), mask.shape[1]
    coef = None if coef is None else f32c(coef.to(dev))
    if objective == "v" and (coef is None or coef.shape != (B, 2)):
        raise ValueError("the v objective needs coef (B,2) = (alpha, sigma)")
    nbytes = lib().r2dm_diffusion_loss_scratch_bytes(B, C, plane)
    if nbytes == 0:
        raise R2DMError(f"diffusion_loss: empty or oversized problem (B={B}, C={C}, plane={plane})")
    scratch = torch.empty(nbytes // 8, device=dev, dtype=torch.float64)
    num = torch.empty(B, C, device=dev, dtype=torch.float64)
    den = torch.empty(B, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        check(lib().r2dm_diffusion_loss(ptr(prediction), ptr(x_0), ptr(noise), ptr(mask), mask_c, ptr(coef), OBJECTIVES[objective],
                                        LOSS_CRITERIA[criterion], B, C, plane, ptr(scratch), ptr(num), ptr(den), stream_ptr(dev)))
    return num, den


DEPTH_FORMATS = {"log_depth": 0, "inverse_depth": 1, "depth": 2}


def lidar_postprocess(x, ray_angles, min_depth: float, max_depth: float, depth_format: str = "log_depth") -> torch.Tensor:
    require_gpu(x, "x")
    if depth_format not in DEPTH_FORMATS:
        raise ValueError(f"unknown depth_format {depth_format!r}")
    x, ang = f32c(x), f32c(ray_angles).reshape(2, *x.shape[-2:])
    B, _, H, W = x.shape
    out = torch.empty(B, 5, H, W, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        check(lib().r2dm_lidar_postprocess_fmt(ptr(x), ptr(ang), ptr(out), B, H, W, float(min_depth), float(max_depth),
                                               DEPTH_FORMATS[depth_format], stream_ptr(x.device)))
    return out
