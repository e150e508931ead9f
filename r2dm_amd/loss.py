"""The held-out denoising loss of a checkpoint and how it splits over noise levels.

``loss_curve`` evaluates every image at every level of a fixed grid with ``GaussianDiffusion.loss_terms`` -- one noising
(``r2dm_q_step``), one U-Net call and one fused reduction (``r2dm_diffusion_loss``) per image and level; no sampling, no gradient.
``denoising_loss.py`` at the repository root is its command line."""
from __future__ import annotations

from typing import List, Optional

import torch

from .diffusion import DiscreteTimeGaussianDiffusion, GaussianDiffusion


def level_grid(ddpm: GaussianDiffusion, levels: int) -> torch.Tensor:
    """The ``levels`` steps a curve is evaluated at, on the host.  Continuous time: the midpoints ``t_k = (k + 0.5) / levels`` of
    ``levels`` equal cells of [0, 1] (float32).  Discrete time: ``levels`` evenly spaced integer steps from 0 to ``T - 1``, both included
    (int64; ``levels`` = 1 gives step 0)."""
    levels = int(levels)
    if levels < 1:
        raise ValueError(f"levels must be >= 1, got {levels}")
    if isinstance(ddpm, DiscreteTimeGaussianDiffusion):
        T = int(ddpm.num_training_steps)
        if levels > T:
            raise ValueError(f"{levels} levels of {T} training steps: at most one level per step")
        return torch.linspace(0, T - 1, levels, dtype=torch.float64).round().long()
    return ((torch.arange(levels, dtype=torch.float64) + 0.5) / levels).float()


@torch.inference_mode()
def loss_curve(ddpm: GaussianDiffusion, x_0: torch.Tensor, loss_mask: Optional[torch.Tensor] = None, levels: int = 16, rng=None,
               batch_size: Optional[int] = None) -> dict:
    """Every image of ``x_0`` (N,C,H,W) at every level of ``level_grid(ddpm, levels)``.

    The N x levels (level, image) rows are walked level by level, ``batch_size`` U-Net rows at a time (default: the denoiser's
    ``max_batch``); a row's numbers do not depend on the rows it shares a call with.  ``rng``: a list of N generators (one per image:
    image i takes its noise for level 0, 1, ... from generator i in that order, whatever ``batch_size``), one generator, or None
    (the device's global generator) -- the last two draw one block of noise per call, so their draws depend on ``batch_size``.
    ``loss_mask``: None, (N,1,H,W) or (N,C,H,W), used at every level.

    -> ``{"levels": [{"t", "log_snr", "loss", "weighted_loss", "per_channel"} per level], "mean_weighted_loss", "num_images"}``: per
    level the means over the images of the log-SNR, of the unweighted per-sample loss, of that loss times the level's loss weight,
    and of the per-channel losses (depth, reflectance in a two-channel model).  ``mean_weighted_loss`` is the mean over the levels of
    ``weighted_loss``: for continuous time the midpoint Riemann sum of E_t[w(t) L(t)] over t ~ U(0,1), the expectation of the
    training objective with every loss paired with its own weight; for discrete time the mean over the evenly spaced subset of the
    T steps, an estimate of the same expectation over the uniform step distribution."""
    if x_0.dim() != 4:
        raise ValueError(f"expected x_0 (N,C,H,W), got {tuple(x_0.shape)}")
    N = x_0.shape[0]
    if N < 1:
        raise ValueError("loss_curve needs at least one image")
    if isinstance(rng, list) and len(rng) != N:
        raise ValueError(f"{len(rng)} generators for {N} images")
    if batch_size is None:
        batch_size = int(getattr(getattr(ddpm.model, "_orig_mod", ddpm.model), "max_batch", 8))
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    grid = level_grid(ddpm, levels)
    K = grid.numel()
    rows = [(k, i) for k in range(K) for i in range(N)]
    keys = ("log_snr", "per_sample", "weighted", "per_channel")
    parts = {key: [] for key in keys}
    for r in range(0, len(rows), batch_size):
        chunk = rows[r:r + batch_size]
        img = torch.tensor([i for _, i in chunk], device=x_0.device)
        steps = grid[torch.tensor([k for k, _ in chunk])].to(x_0.device)
        terms = ddpm.loss_terms(x_0[img], steps, None if loss_mask is None else loss_mask.to(x_0.device)[img],
                                rng=[rng[i] for _, i in chunk] if isinstance(rng, list) else rng)
        for key in keys:
            parts[key].append(terms[key])
    table = {key: torch.cat(parts[key]).double().cpu() for key in keys}  # float64 on the host: the means over the images
    per_level = lambda key: table[key].reshape(K, N, *table[key].shape[1:]).mean(1)
    log_snr, loss, weighted, per_channel = (per_level(key) for key in keys)
    out_levels: List[dict] = []
    for k in range(K):
        out_levels.append({"t": grid[k].item(), "log_snr": log_snr[k].item(), "loss": loss[k].item(), "weighted_loss": weighted[k].item(),
                           "per_channel": per_channel[k].tolist()})
    return {"levels": out_levels, "mean_weighted_loss": weighted.mean().item(), "num_images": N}
