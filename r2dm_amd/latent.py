"""The model's latent space: DDIM inversion, decoding from a given latent, spherical interpolation.

``ContinuousTimeGaussianDiffusion.invert`` encodes a scan deterministically (the DDIM update with eta = 0 run towards more noise) and
``sample_from`` runs the reverse loop from any tensor at any noise level; here are the two HIP operators they and the interpolation
stand on (``r2dm_amd/csrc/latent.hip``) and the compositions: ``interpolate`` (the latent-interpolation figure of the R2DM paper) and
``reconstruct`` (a scan through the model and back).  There is no CPU fallback."""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence

import torch

from . import _lib

_MAX_WEIGHTS = 64  # weights of one r2dm_slerp call (csrc/common.h: kSlerpMaxWeights)


def ddim_transfer(x_t: torch.Tensor, prediction: torch.Tensor, coef: torch.Tensor, objective) -> torch.Tensor:
    """``x_u`` from ``x_t`` (B,...) and the denoiser's ``prediction`` at level t, along the deterministic DDIM line to level u (either
    direction, unclipped); ``coef`` (B,4) = (alpha_t, sigma_t, alpha_u, sigma_u); ``objective``: "eps", "v", "x_0" or its id.  One launch of
    ``r2dm_ddim_transfer``: float32, not contracted, x_0 and eps in the direct form of the objective."""
    _lib.require_gpu(x_t, "x_t")
    if isinstance(objective, str):
        if objective not in _lib.OBJECTIVES:
            raise ValueError(f"invalid objective {objective}")
        objective = _lib.OBJECTIVES[objective]
    if prediction.shape != x_t.shape or x_t.dim() < 2:
        raise ValueError(f"x_t {tuple(x_t.shape)} and prediction {tuple(prediction.shape)} must have one (B,...) shape")
    B = x_t.shape[0]
    if tuple(coef.shape) != (B, 4):
        raise ValueError(f"coef must be ({B},4) = (alpha_t, sigma_t, alpha_u, sigma_u), got {tuple(coef.shape)}")
    dev = x_t.device
    x_t, prediction, coef = _lib.f32c(x_t), _lib.f32c(prediction.to(dev)), _lib.f32c(coef.to(dev))
    out = torch.empty_like(x_t)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().r2dm_ddim_transfer(_lib.ptr(x_t), _lib.ptr(prediction), _lib.ptr(coef), _lib.ptr(out), B, x_t.numel() // max(B, 1),
                                                 int(objective), _lib.stream_ptr(dev)))
    return out


def _weights(weights) -> list:
    w = [float(v) for v in (weights.detach().cpu().reshape(-1).tolist() if isinstance(weights, torch.Tensor) else list(weights))]
    if not w:
        raise ValueError("slerp needs at least one weight")
    if not all(math.isfinite(v) for v in w):
        raise ValueError(f"slerp weights must be finite, got {w}")
    return w


def slerp(a: torch.Tensor, b: torch.Tensor, weights: Sequence[float], return_coefficients: bool = False):
    """Spherical interpolation of two latent batches ``a``, ``b`` (B,...) at the K ``weights`` (0 -> ``a``, 1 -> ``b``; any finite value,
    outside [0,1] it extrapolates) -> (K,B,...) float32; with ``return_coefficients`` also ``coef64`` (K,B,2) float64 = (c_a, c_b), the
    coefficients whose float32 roundings the output was formed with.  The angle is taken per sample over all its elements
    (``r2dm_slerp``: float64 sums in a fixed order, so a sample's frames do not depend on the batch it is in; (anti)parallel or zero
    inputs fall back to the lerp pair (1-w, w))."""
    w = _weights(weights)
    _lib.require_gpu(a, "a")
    if b.shape != a.shape or a.dim() < 2 or a.shape[0] < 1:
        raise ValueError(f"a {tuple(a.shape)} and b {tuple(b.shape)} must have one (B,...) shape with B >= 1")
    dev, B, K = a.device, a.shape[0], len(w)
    a, b = _lib.f32c(a), _lib.f32c(b.to(dev))
    per_sample = a.numel() // B
    L = _lib.lib()
    nbytes = L.r2dm_slerp_scratch_bytes(B, per_sample)
    if nbytes == 0:
        raise _lib.R2DMError(f"slerp: batch must be in [1, 65535] and the elements per sample a multiple of 4 (B={B}, per_sample={per_sample})")
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    out = torch.empty(K, *a.shape, dtype=torch.float32, device=dev)
    coef64 = torch.empty(K, B, 2, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        for k0 in range(0, K, _MAX_WEIGHTS):  # (the sums are formed again per chunk of 64 weights: the same bits)
            chunk = w[k0:k0 + _MAX_WEIGHTS]
            host = (ctypes.c_float * len(chunk))(*chunk)
            _lib.check(L.r2dm_slerp(_lib.ptr(a), _lib.ptr(b), host, len(chunk), _lib.ptr(out[k0:]), _lib.ptr(coef64[k0:]), B, per_sample,
                                    _lib.ptr(scratch), _lib.stream_ptr(dev)))
    return (out, coef64) if return_coefficients else out


def _decode(ddpm, latents: torch.Tensor, num_steps: int, t_start: float, mode: str, ddim_eta: float, rng, decoder: str = "ddim") -> torch.Tensor:
    """``sample_from(..., clip=False)`` over (N,C,H,W) latents in chunks of at most the model's ``max_batch``; ``rng`` (None, one generator,
    or a list with one generator per latent) follows the chunks.  ``decoder="dpmpp"``: ``sample_dpm(x_t=..., clip=False)`` instead, which draws
    nothing (``mode``, ``ddim_eta`` and ``rng`` are not read)."""
    if decoder not in ("ddim", "dpmpp"):
        raise ValueError(f"decoder must be 'ddim' or 'dpmpp', got {decoder!r}")
    cap = int(getattr(getattr(ddpm.model, "_orig_mod", ddpm.model), "max_batch", 0)) or latents.shape[0]
    frames = []
    for i in range(0, latents.shape[0], cap):
        part = latents[i:i + cap]
        r = rng[i:i + cap] if isinstance(rng, list) else rng
        if decoder == "dpmpp":
            frames.append(ddpm.sample_dpm(part.shape[0], num_steps, x_t=part, t_start=t_start, clip=False, progress=False))
            continue
        frames.append(ddpm.sample_from(part, num_steps, t_start=t_start, progress=False, rng=r, mode=mode, ddim_eta=ddim_eta, clip=False))
    return torch.cat(frames)


def _invert(ddpm, x: torch.Tensor, num_steps: int, t_end: float) -> torch.Tensor:
    cap = int(getattr(getattr(ddpm.model, "_orig_mod", ddpm.model), "max_batch", 0)) or x.shape[0]
    return torch.cat([ddpm.invert(x[i:i + cap], num_steps, t_end=t_end, progress=False) for i in range(0, x.shape[0], cap)])


def interpolate(ddpm, x_a: torch.Tensor, x_b: torch.Tensor, num_frames: int, num_steps: int, t_end: float = 1.0, mode: str = "ddim",
                ddim_eta: float = 0.0, rng=None, return_latents: bool = False, decoder: str = "ddim"):
    """Latent interpolation between two image batches ``x_a``, ``x_b`` (B,C,H,W) in [-1,1]: both are inverted to ``t_end`` in one batch
    (``ddpm.invert``, ``num_steps`` steps), the latents are slerped at ``linspace(0, 1, num_frames)`` and every frame is decoded with
    ``ddpm.sample_from(..., t_start=t_end, clip=False)`` in chunks of at most the model's ``max_batch`` -> (num_frames,B,C,H,W), frame 0
    the reconstruction of ``x_a`` and the last one that of ``x_b``.  ``rng`` is ``sample_from``'s: None, one generator, or a list of
    ``num_frames * B`` generators in frame-major order (read for ``mode="ddpm"`` and for DDIM with ``ddim_eta > 0`` only in effect).
    ``return_latents``: also the (num_frames,B,C,H,W) interpolated latents.  ``decoder="dpmpp"``: the frames are decoded by
    ``ddpm.sample_dpm(x_t=..., t_start=t_end, clip=False)`` (DPM-Solver++(2M), ``num_steps`` steps; the inversion stays DDIM's)."""
    if x_a.shape != x_b.shape or x_a.dim() != 4:
        raise ValueError(f"x_a {tuple(x_a.shape)} and x_b {tuple(x_b.shape)} must have one (B,C,H,W) shape")
    if int(num_frames) < 2:
        raise ValueError(f"num_frames must be at least 2, got {num_frames}")
    B = x_a.shape[0]
    z = _invert(ddpm, torch.cat([x_a, x_b.to(x_a.device)]), num_steps, t_end)
    latents = slerp(z[:B], z[B:], torch.linspace(0.0, 1.0, int(num_frames)).tolist())
    frames = _decode(ddpm, latents.flatten(0, 1), num_steps, t_end, mode, ddim_eta, rng, decoder).reshape(latents.shape)
    return (frames, latents) if return_latents else frames


def reconstruct(ddpm, x_0: torch.Tensor, num_steps: int, t_end: float = 1.0) -> torch.Tensor:
    """``x_0`` (B,C,H,W) through the model and back: ``invert`` to ``t_end``, then ``sample_from(mode="ddim", clip=False)`` from there."""
    return _decode(ddpm, _invert(ddpm, x_0, num_steps, t_end), num_steps, t_end, "ddim", 0.0, None)
