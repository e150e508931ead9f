"""Completion metrics: how good an inpainted scan is.

The R2DM paper scores beam-level upsampling of held-out scans by the mean absolute error of range and reflectance over the pixels the
model had to fill in, and by the IoU of RangeNet labels of the completed image against the labels of the real scan, next to nearest and
linear interpolation of the known beams.  The reference has no code for it.  Here the scoring is three HIP kernels
(``r2dm_amd/csrc/completion.hip``) and this module:

- ``corruption_mask``      the corruptions, by name: ``full``, ``beams:K``, ``random_beams:P``, ``random_points:P``.
- ``completion_errors``    per sample the four counts and six error sums of ``r2dm_completion_error`` and the values derived from them.
- ``confusion_matrix`` / ``iou_from_confusion``   label agreement.
- ``fill_beams``           the interpolation baselines.
- ``ensemble_scores``      K completions per scan scored as an ensemble (``r2dm_ensemble_score``): CRPS, the rank histogram, spread against
  skill, the Brier score of ray drop, best-of-K and per-pixel return probability / mean / std / median maps; ``ensemble_consensus`` turns the
  maps into one scan, ``aggregate_ensemble`` sums over scans, ``member_seed`` seeds member k of scan i.
- ``ensemble_coherence``   the same K completions scored across pixels (``r2dm_ensemble_coherence``): the energy score and the variogram
  score, which tell a coherent draw from per-pixel noise with the same marginals; ``aggregate_coherence`` averages over scans.
- ``evaluate_completion``  corrupt, complete (RePaint, the data-consistent sampler ``ddpm.complete``, the same on DPM-Solver++(2M), ``ddpm.complete_dpm``, or a baseline), score; ``completion_eval.py`` is its command line.

A pixel is a *return* when its metric depth lies strictly inside ``(lo, hi)``; any other depth, NaN included, is "no return".  The errors
are taken over E: the unknown pixels (mask 0) where the real scan has a return.  A prediction without a return there counts with depth 0
(what ``LiDARUtility.postprocess`` stores for a dropped ray) in ``mae_depth`` / ``rmse_depth`` and is left out of ``*_depth_both``, which
are taken where both have a return; ``return_recall`` is the fraction of E with a predicted return and ``false_return_rate`` the fraction
of the unknown pixels without a real return where one is predicted.  Everything runs on the GPU; there is no CPU fallback."""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import torch

from . import _lib

RAW_NAMES = ("unknown", "evaluated", "both", "false_returns", "abs_depth", "sq_depth", "abs_depth_both", "sq_depth_both",
             "abs_reflectance", "sq_reflectance")
DERIVED_NAMES = ("mae_depth", "rmse_depth", "mae_depth_both", "rmse_depth_both", "mae_reflectance", "rmse_reflectance", "return_recall",
                 "false_return_rate")
ENSEMBLE_RAW_NAMES = ("unknown", "evaluated", "abs_depth_members", "pair_depth", "sq_depth_mean", "var_depth", "abs_reflectance_members",
                      "pair_reflectance", "sq_reflectance_mean", "var_reflectance", "brier", "returns_expected", "false_expected")
ENSEMBLE_DERIVED_NAMES = ("crps_depth", "crps_fair_depth", "mae_depth_members", "best_mae_depth", "rmse_depth_mean", "spread_depth",
                          "spread_skill_depth", "crps_reflectance", "crps_fair_reflectance", "mae_reflectance_members", "best_mae_reflectance",
                          "rmse_reflectance_mean", "spread_reflectance", "spread_skill_reflectance", "brier_return", "return_recall",
                          "false_return_rate")
ENSEMBLE_MAP_NAMES = ("return_probability", "depth_mean", "depth_std", "depth_median", "depth_min", "depth_max", "reflectance_mean",
                      "reflectance_std")
COHERENCE_DERIVED_NAMES = tuple(stem + "_" + name for name in ("depth", "reflectance") for stem in (
    "energy", "energy_fair", "member_rmse", "best_rmse", "diversity", "spread_skill_energy", "variogram", "variogram_total", "variogram_rel"))
DEFAULT_OFFSETS = ((0, 1), (0, 2), (0, 4), (0, 8), (1, 0), (2, 0), (1, 1), (1, -1))  # (dh, dw): along a beam, across beams, the diagonals
MAX_OFFSETS = 16
MAX_MEMBERS = 64
STOCHASTIC_METHODS = ("repaint", "ddnm", "dpmpp")
FILL_MODES = {"nearest": 0, "linear": 1}
ROW_KINDS = ("full", "beams", "random_beams")  # corruptions whose mask is whole rows: what the interpolation baselines are defined for
METHODS = ("repaint", "ddnm", "dpmpp", "nearest", "linear", "target")


# ---- corruptions -------------------------------------------------------------------------------------------------------------------------
def parse_kind(kind: str):
    """``"full"`` -> ("full", None); ``"beams:4"`` -> ("beams", 4); ``"random_beams:0.5"`` / ``"random_points:0.1"`` -> (name, 0.5 / 0.1)."""
    name, sep, arg = str(kind).partition(":")
    try:
        if name == "full" and not sep:
            return name, None
        if name == "beams" and sep:
            k = int(arg)
            if k >= 1:
                return name, k
        if name in ("random_beams", "random_points") and sep:
            p = float(arg)
            if 0.0 <= p <= 1.0:
                return name, p
    except ValueError:
        pass
    raise ValueError(f"malformed corruption {kind!r}: expected full, beams:K (K >= 1), random_beams:P or random_points:P (0 <= P <= 1)")


def corruption_mask(kind: str, H: int, W: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """The (1,H,W) float32 mask of a corruption on the CPU, 1 = known.  ``beams:K`` keeps rows 0, K, 2K, ... (``beams:4`` is
    completion_demo.py's ``[::4]``); the random kinds are Bernoulli draws from ``generator`` (a CPU generator; None: the global one) in the
    demo's shapes, (H,1) for beams and (H,W) for points."""
    name, arg = parse_kind(kind)
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"mask of {H}x{W}: sizes must be >= 1")
    mask = torch.zeros(1, H, W)
    if name == "full":
        mask[:] = 1
    elif name == "beams":
        mask[:, ::arg] = 1
    elif name == "random_beams":
        mask[0] = torch.empty(H, 1).bernoulli_(arg, generator=generator)
    else:
        mask[0] = torch.empty(H, W).bernoulli_(arg, generator=generator)
    return mask


def scan_seed(seed: int, index: int) -> int:
    """The seed of everything drawn for scan ``index`` under ``seed``: its corruption masks (a CPU generator, a fresh one per kind) and its
    RePaint noise (a device generator, ``setup_rng``).  ``seed * 2**32 + index``."""
    seed, index = int(seed), int(index)
    if not (0 <= seed < 2 ** 31 and 0 <= index < 2 ** 32):
        raise ValueError(f"seed must be in [0, 2^31) and the scan index in [0, 2^32), got {seed}, {index}")
    return seed * 2 ** 32 + index


def member_seed(seed: int, index: int, k: int) -> int:
    """The seed of member ``k`` of scan ``index``'s ensemble under ``seed``.  Member 0 is the scan's single draw: ``scan_seed(seed, index)``.
    For k > 0 the first 64-bit word of ``numpy.random.SeedSequence([seed, index, k]).generate_state(1, numpy.uint64)`` with its top bit
    cleared: a pure function of the three into [0, 2^63), what a ``torch.Generator`` takes."""
    import numpy as np

    base, k = scan_seed(seed, index), int(k)
    if not 0 <= k < 2 ** 32:
        raise ValueError(f"the member index must be in [0, 2^32), got {k}")
    if k == 0:
        return base
    return int(np.random.SeedSequence([int(seed), int(index), k]).generate_state(1, np.uint64)[0]) >> 1


# ---- errors ------------------------------------------------------------------------------------------------------------------------------
def _ratio(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
    nan = torch.full_like(num, math.nan)
    return torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), nan)


def derived_errors(raw: torch.Tensor) -> Dict[str, torch.Tensor]:
    """(...,10) float64 raw values (``RAW_NAMES``) -> the derived values (``DERIVED_NAMES``), NaN where the denominator is 0."""
    raw = raw.double()
    U, E, Bo, fr = raw[..., 0], raw[..., 1], raw[..., 2], raw[..., 3]
    return {"mae_depth": _ratio(raw[..., 4], E), "rmse_depth": _ratio(raw[..., 5], E).sqrt(),
            "mae_depth_both": _ratio(raw[..., 6], Bo), "rmse_depth_both": _ratio(raw[..., 7], Bo).sqrt(),
            "mae_reflectance": _ratio(raw[..., 8], E), "rmse_reflectance": _ratio(raw[..., 9], E).sqrt(),
            "return_recall": _ratio(Bo, E), "false_return_rate": _ratio(fr, U - E)}


def completion_error_sums(pred: torch.Tensor, target: torch.Tensor, known: torch.Tensor, lo: float, hi: float) -> torch.Tensor:
    """(B,10) float64 on the device: ``r2dm_completion_error`` (``RAW_NAMES``)."""
    _lib.require_gpu(pred, "pred")
    if pred.dim() != 4 or pred.shape[1] != 5 or target.shape != pred.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} must be one (B,5,H,W) shape [depth, x, y, z, reflectance]")
    B, _, H, W = pred.shape
    if tuple(known.shape) != (B, 1, H, W):
        raise ValueError(f"known {tuple(known.shape)} must be (B,1,H,W) = {(B, 1, H, W)}")
    dev = pred.device
    pred, target, known = _lib.f32c(pred), _lib.f32c(target.to(dev)), _lib.f32c(known.to(dev))
    out = torch.empty(B, len(RAW_NAMES), dtype=torch.float64, device=dev)
    if B == 0:
        return out
    L = _lib.lib()
    nbytes = L.r2dm_completion_error_scratch_bytes(B, H * W)
    if nbytes == 0:
        raise _lib.R2DMError(f"completion_errors: empty or oversized problem (B={B}, plane={H * W})")
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.r2dm_completion_error(_lib.ptr(pred), _lib.ptr(target), _lib.ptr(known), float(lo), float(hi), B, H * W, _lib.ptr(scratch),
                                           _lib.ptr(out), _lib.stream_ptr(dev)))
    return out


def completion_errors(pred: torch.Tensor, target: torch.Tensor, known: torch.Tensor, lo: float, hi: float) -> Dict[str, torch.Tensor]:
    """``pred``, ``target`` (B,5,H,W) in the sample layout (``LiDARUtility.postprocess``, ``project_scans(layout="sample")``), ``known``
    (B,1,H,W) zeros and ones -> (B,) float64 tensors: the ten raw values under ``RAW_NAMES`` and the derived ``DERIVED_NAMES`` (NaN where
    the denominator is 0)."""
    raw = completion_error_sums(pred, target, known, lo, hi)
    out = {name: raw[:, k] for k, name in enumerate(RAW_NAMES)}
    out.update(derived_errors(raw))
    return out


# ---- ensembles: K completions of a scan scored as a probabilistic forecast ----------------------------------------------------------------
def derived_ensemble(raw: torch.Tensor, member: torch.Tensor) -> Dict[str, torch.Tensor]:
    """(...,13) raw values (``ENSEMBLE_RAW_NAMES``) and (...,2,K) per-member sums -> the derived values (``ENSEMBLE_DERIVED_NAMES``), NaN
    where a denominator is 0.  CRPS = E|X - y| - E|X - X'| / 2 with both expectations over the K members (``crps_fair`` with the second over
    the K (K - 1) pairs of distinct members: unbiased for the underlying distribution, NaN at K = 1); ``spread_skill`` =
    sqrt((K + 1) / K * mean variance / mean squared error of the ensemble mean), 1 for a calibrated ensemble."""
    raw, member = raw.double(), member.double()
    K = member.shape[-1]
    U, E = raw[..., 0], raw[..., 1]
    nan = torch.full_like(E, math.nan)
    out = {}
    for c, name in ((2, "depth"), (6, "reflectance")):
        a, pr, sq, var = raw[..., c], raw[..., c + 1], raw[..., c + 2], raw[..., c + 3]
        best = member[..., 0 if name == "depth" else 1, :].min(dim=-1).values if K else nan
        out["crps_" + name] = _ratio(a / K - pr / K ** 2, E)
        out["crps_fair_" + name] = _ratio(a / K - pr / (K * (K - 1)), E) if K > 1 else nan
        out["mae_" + name + "_members"] = _ratio(a, K * E)
        out["best_mae_" + name] = _ratio(best, E)
        out["rmse_" + name + "_mean"] = _ratio(sq, E).sqrt()
        out["spread_" + name] = _ratio(var, E).sqrt()
        out["spread_skill_" + name] = ((K + 1) / K * _ratio(var, sq)).sqrt()
    out["brier_return"] = _ratio(raw[..., 10], U)
    out["return_recall"] = _ratio(raw[..., 11], E)
    out["false_return_rate"] = _ratio(raw[..., 12], U - E)
    return {name: out[name] for name in ENSEMBLE_DERIVED_NAMES}


def ensemble_score_sums(samples: torch.Tensor, target: torch.Tensor, known: torch.Tensor, lo: float, hi: float, maps: bool = True):
    """``r2dm_ensemble_score`` on the device: ``samples`` (B,K,5,H,W) -> ``(raw (B,13) float64, member (B,2,K) float64, rank (B,K+1) int64,
    maps (B,8,H,W) float32 or None)``."""
    _lib.require_gpu(samples, "samples")
    if samples.dim() != 5 or samples.shape[2] != 5:
        raise ValueError(f"samples {tuple(samples.shape)} must be (B,K,5,H,W): K members per scan in the layout [depth, x, y, z, reflectance]")
    B, K, _, H, W = samples.shape
    if not 1 <= K <= MAX_MEMBERS:
        raise ValueError(f"an ensemble has 1 to {MAX_MEMBERS} members, got {K}")
    if tuple(target.shape) != (B, 5, H, W) or tuple(known.shape) != (B, 1, H, W):
        raise ValueError(f"target {tuple(target.shape)} must be {(B, 5, H, W)} and known {tuple(known.shape)} {(B, 1, H, W)}")
    dev = samples.device
    samples, target, known = _lib.f32c(samples), _lib.f32c(target.to(dev)), _lib.f32c(known.to(dev))
    raw = torch.empty(B, len(ENSEMBLE_RAW_NAMES), dtype=torch.float64, device=dev)
    member = torch.empty(B, 2, K, dtype=torch.float64, device=dev)
    rank = torch.empty(B, K + 1, dtype=torch.int64, device=dev)
    out = torch.empty(B, len(ENSEMBLE_MAP_NAMES), H, W, dtype=torch.float32, device=dev) if maps else None
    if B == 0:
        return raw, member, rank, out
    L = _lib.lib()
    nbytes = L.r2dm_ensemble_score_scratch_bytes(B, K, H * W)
    if nbytes == 0:
        raise _lib.R2DMError(f"ensemble_scores: empty or oversized problem (B={B}, K={K}, plane={H * W})")
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.r2dm_ensemble_score(_lib.ptr(samples), _lib.ptr(target), _lib.ptr(known), float(lo), float(hi), B, K, H * W, _lib.ptr(scratch),
                                         _lib.ptr(raw), _lib.ptr(member), _lib.ptr(rank), _lib.ptr(out), _lib.stream_ptr(dev)))
    return raw, member, rank, out


def ensemble_scores(samples: torch.Tensor, target: torch.Tensor, known: torch.Tensor, lo: float, hi: float, maps: bool = True) -> dict:
    """K completions per scan scored as an ensemble.  ``samples`` (B,K,5,H,W) in the sample layout, the K members of a scan adjacent;
    ``target`` (B,5,H,W), ``known`` (B,1,H,W) as for ``completion_errors`` -> a dict of (B,) float64 tensors, the raw sums under
    ``ENSEMBLE_RAW_NAMES`` and the derived values under ``ENSEMBLE_DERIVED_NAMES`` (NaN where a denominator is 0), plus
    ``member_abs_depth`` / ``member_abs_reflectance`` (B,K), ``rank_histogram`` (B,K+1) int64 (over E, how many members lie below the
    measured depth: flat for a calibrated ensemble) and ``maps`` (B,8,H,W) float32 (``ENSEMBLE_MAP_NAMES``; None with ``maps=False``).
    ``crps_depth`` at K = 1 is ``completion_errors``' ``mae_depth``."""
    raw, member, rank, out = ensemble_score_sums(samples, target, known, lo, hi, maps)
    res = {name: raw[:, k] for k, name in enumerate(ENSEMBLE_RAW_NAMES)}
    res.update(derived_ensemble(raw, member))
    res.update(member_abs_depth=member[:, 0], member_abs_reflectance=member[:, 1], rank_histogram=rank, maps=out)
    return res


def ensemble_consensus(maps: torch.Tensor, lidar_utils) -> torch.Tensor:
    """The ensemble's point forecast, (B,5,H,W) in the sample layout: depth = the median of the returning members where at least half of
    the members return, else 0 (no return); xyz = ``lidar_utils.to_xyz`` of it; reflectance = the members' mean.  What
    ``completion_errors``, the Chamfer metrics and the segmentation take."""
    if maps.dim() != 4 or maps.shape[1] != len(ENSEMBLE_MAP_NAMES):
        raise ValueError(f"expected maps (B,8,H,W) ({', '.join(ENSEMBLE_MAP_NAMES)}), got {tuple(maps.shape)}")
    depth = torch.where(maps[:, [0]] >= 0.5, maps[:, [3]], torch.zeros_like(maps[:, [3]]))
    return torch.cat([depth, lidar_utils.to_xyz(depth), maps[:, [6]]], dim=1).float().contiguous()


def aggregate_ensemble(raw: torch.Tensor, member: torch.Tensor, rank: torch.Tensor) -> dict:
    """Per-scan (N,13), (N,2,K), (N,K+1) -> ``{"counts", "sums", "micro", "macro", "rank_histogram"}`` in the shape of ``aggregate_errors``:
    micro = the derived values of the sums over all scans (``best_mae`` from the summed per-member errors: the best member over the whole
    set), macro = the mean of the per-scan derived values, ignoring the NaN ones; the rank histogram is summed."""
    raw = torch.as_tensor(raw).detach().cpu().double().reshape(-1, len(ENSEMBLE_RAW_NAMES))
    member = torch.as_tensor(member).detach().cpu().double()
    K = member.shape[-1]
    member, rank = member.reshape(-1, 2, K), torch.as_tensor(rank).detach().cpu().long().reshape(-1, K + 1)
    total = raw.sum(0)
    out = {"counts": {"scans": int(raw.shape[0]), "members": int(K), **{name: int(total[k].item()) for k, name in enumerate(ENSEMBLE_RAW_NAMES[:2])}},
           "sums": {name: total[k].item() for k, name in enumerate(ENSEMBLE_RAW_NAMES) if k >= 2},
           "micro": {name: v.item() for name, v in derived_ensemble(total, member.sum(0)).items()}, "macro": {},
           "rank_histogram": rank.sum(0).tolist()}
    out["counts"]["unknown_without_return"] = out["counts"]["unknown"] - out["counts"]["evaluated"]
    for name, v in derived_ensemble(raw, member).items():
        ok = ~v.isnan()
        out["macro"][name] = v[ok].mean().item() if ok.any() else math.nan
    return out


# ---- ensemble coherence: the energy score and the variogram score, across pixels ----------------------------------------------------------
def _check_offsets(offsets, H: int, W: int):
    out = []
    for o in offsets:
        try:
            dh, dw = (int(v) for v in o)
            if (dh, dw) != tuple(o):
                raise TypeError
        except (TypeError, ValueError):
            raise ValueError(f"an offset is a pair of integers (dh, dw), got {o!r}") from None
        if (dh, dw) == (0, 0) or abs(dh) >= H or abs(dw) >= W:
            raise ValueError(f"offset {(dh, dw)} must satisfy |dh| < {H}, |dw| < {W} and not be (0, 0)")
        out.append((dh, dw))
    if len(out) > MAX_OFFSETS:
        raise ValueError(f"at most {MAX_OFFSETS} offsets, got {len(out)}")
    return tuple(out)


def ensemble_coherence_sums(samples: torch.Tensor, target: torch.Tensor, known: torch.Tensor, lo: float, hi: float, offsets=None):
    """``r2dm_ensemble_coherence`` on the device: ``samples`` (B,K,5,H,W) -> ``(counts (B,2), dist (B,2,K+1,K+1), vario (B,2,O,4), offsets)``,
    float64.  ``offsets``: pairs (dh, dw) with |dh| < H, |dw| < W, not (0, 0), at most 16 (an invalid one is a ``ValueError``); None: the
    members of ``DEFAULT_OFFSETS`` that are valid for (H, W), possibly none.  The offsets used are returned as a tuple."""
    _lib.require_gpu(samples, "samples")
    if samples.dim() != 5 or samples.shape[2] != 5:
        raise ValueError(f"samples {tuple(samples.shape)} must be (B,K,5,H,W): K members per scan in the layout [depth, x, y, z, reflectance]")
    B, K, _, H, W = samples.shape
    if not 1 <= K <= MAX_MEMBERS:
        raise ValueError(f"an ensemble has 1 to {MAX_MEMBERS} members, got {K}")
    if tuple(target.shape) != (B, 5, H, W) or tuple(known.shape) != (B, 1, H, W):
        raise ValueError(f"target {tuple(target.shape)} must be {(B, 5, H, W)} and known {tuple(known.shape)} {(B, 1, H, W)}")
    if H < 1 or W < 1:
        raise ValueError(f"scans of {H}x{W}: sizes must be >= 1")
    if offsets is None:
        offsets = tuple((dh, dw) for dh, dw in DEFAULT_OFFSETS if abs(dh) < H and abs(dw) < W)
    else:
        offsets = _check_offsets(offsets, H, W)
    n = len(offsets)
    dev = samples.device
    samples, target, known = _lib.f32c(samples), _lib.f32c(target.to(dev)), _lib.f32c(known.to(dev))
    counts = torch.empty(B, 2, dtype=torch.float64, device=dev)
    dist = torch.empty(B, 2, K + 1, K + 1, dtype=torch.float64, device=dev)
    vario = torch.empty(B, 2, n, 4, dtype=torch.float64, device=dev)
    if B == 0:
        return counts, dist, vario, offsets
    L = _lib.lib()
    nbytes = L.r2dm_ensemble_coherence_scratch_bytes(B, K, H, W, n)
    if nbytes == 0:
        raise _lib.R2DMError(f"ensemble_coherence: empty or oversized problem (B={B}, K={K}, {H}x{W}, {n} offsets)")
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    import ctypes

    host = (ctypes.c_int32 * (2 * max(n, 1)))(*[v for o in offsets for v in o])
    with torch.cuda.device(dev):
        _lib.check(L.r2dm_ensemble_coherence(_lib.ptr(samples), _lib.ptr(target), _lib.ptr(known), float(lo), float(hi), B, K, H, W,
                                             ctypes.cast(host, ctypes.c_void_p), n, _lib.ptr(scratch), _lib.ptr(counts), _lib.ptr(dist),
                                             _lib.ptr(vario) if n else None, _lib.stream_ptr(dev)))
    return counts, dist, vario, offsets


def derived_coherence(counts: torch.Tensor, dist: torch.Tensor, vario: torch.Tensor) -> Dict[str, torch.Tensor]:
    """(...,2) counts, (...,2,K+1,K+1) squared distances between the K members and, as row K, the target, (...,2,O,4) variogram sums -> the
    derived values (``COHERENCE_DERIVED_NAMES``), NaN where a denominator is 0.  With D_ij = sqrt(dist[i][j]), per channel:
    ``energy`` = [(1/K) sum_k D_kK - (1/(2 K^2)) sum_{k != l} D_kl] / sqrt|E| (``energy_fair``: 1/(2 K (K - 1)) on the second term, NaN at
    K = 1), both sums over the roots sorted ascending, so the same bits under any permutation of the members; at K = 1 it is
    ``completion_errors``' ``rmse``.  ``member_rmse`` (...,K) = D_kK / sqrt|E|, ``best_rmse`` its least; ``diversity`` = the mean over k < l of
    D_kl / sqrt|E| (NaN at K = 1); ``spread_skill_energy`` = the mean pair distance over the mean distance to the target, 1 when the truth is
    exchangeable with the members.  ``variogram`` (...,O) = sum (a - m)^2 / pairs per offset, ``variogram_total`` the same over all
    offsets, ``variogram_rel`` = sum (a - m)^2 / sum a^2 over all offsets."""
    counts, dist, vario = counts.double(), dist.double(), vario.double()
    K = dist.shape[-1] - 1
    E = counts[..., 1]
    nan = torch.full_like(E, math.nan)
    rootE = E.sqrt()
    out = {}
    for c, name in enumerate(("depth", "reflectance")):
        d = dist[..., c, :, :]
        to_target = d[..., :K, K].sqrt().sort(dim=-1).values                    # (...,K) ascending
        pairs = d[..., :K, :K].sqrt().flatten(-2).sort(dim=-1).values.sum(-1)   # both orders of every pair; the K diagonal zeros add nothing
        skill = to_target.sum(-1) / K
        out["energy_" + name] = _ratio(skill - pairs / (2 * K * K), rootE)
        out["energy_fair_" + name] = _ratio(skill - pairs / (2 * K * (K - 1)), rootE) if K > 1 else nan
        rmse = _ratio(d[..., :K, K], E[..., None].expand(d[..., :K, K].shape)).sqrt()
        out["member_rmse_" + name] = rmse
        out["best_rmse_" + name] = rmse.min(dim=-1).values
        between = _ratio(d[..., :K, :K], E[..., None, None].expand(d[..., :K, :K].shape)).sqrt().flatten(-2).sort(dim=-1).values.sum(-1)
        out["diversity_" + name] = between / (K * (K - 1)) if K > 1 else nan
        out["spread_skill_energy_" + name] = _ratio(out["diversity_" + name], rmse.sort(dim=-1).values.sum(-1) / K) if K > 1 else nan
        v = vario[..., c, :, :]
        out["variogram_" + name] = _ratio(v[..., 1], v[..., 0])
        out["variogram_total_" + name] = _ratio(v[..., 1].sum(-1), v[..., 0].sum(-1))
        out["variogram_rel_" + name] = _ratio(v[..., 1].sum(-1), v[..., 2].sum(-1))
    return {name: out[name] for name in COHERENCE_DERIVED_NAMES}


def ensemble_coherence(samples: torch.Tensor, target: torch.Tensor, known: torch.Tensor, lo: float, hi: float, offsets=None) -> dict:
    """K completions per scan scored across pixels, where ``ensemble_scores`` scores each pixel alone: shuffle the members independently
    at every pixel and every score of ``ensemble_scores`` keeps its bits, while the energy score rises and the variogram score rises by an
    order of magnitude.  Arguments as for ``ensemble_scores``; ``offsets`` as for ``ensemble_coherence_sums`` -> a dict: ``counts`` (B,2)
    [|U|, |E|], ``dist`` (B,2,K+1,K+1), ``vario`` (B,2,O,4) [pairs, sum (a - m)^2, sum a^2, sum m^2], ``offsets`` (the tuple used) and
    the values of ``derived_coherence`` under ``COHERENCE_DERIVED_NAMES``."""
    counts, dist, vario, used = ensemble_coherence_sums(samples, target, known, lo, hi, offsets)
    res = {"counts": counts, "dist": dist, "vario": vario, "offsets": used}
    res.update(derived_coherence(counts, dist, vario))
    return res


def aggregate_coherence(counts: torch.Tensor, dist: torch.Tensor, vario: torch.Tensor, offsets) -> dict:
    """Per-scan (N,2), (N,2,K+1,K+1), (N,2,O,4) -> ``{"counts", "offsets", "sums", "micro", "macro"}``.  ``macro``: the mean of the per-scan
    derived values, ignoring the NaN ones (a value with one entry per member or per offset: entry by entry).  The energy-score family --
    per-scan norms, not additive -- appears there only; ``micro`` holds the variogram values of the sums over all scans and ``sums`` those
    sums, per channel (O,3) [sum (a - m)^2, sum a^2, sum m^2]; ``counts["pairs"]`` is per offset."""
    dist = torch.as_tensor(dist).detach().cpu().double()
    K = dist.shape[-1] - 1
    dist = dist.reshape(-1, 2, K + 1, K + 1)
    vario = torch.as_tensor(vario).detach().cpu().double()
    O = vario.shape[-2]
    vario, counts = vario.reshape(-1, 2, O, 4), torch.as_tensor(counts).detach().cpu().double().reshape(-1, 2)
    total = vario.sum(0)
    out = {"counts": {"scans": int(counts.shape[0]), "members": int(K), "unknown": int(counts[:, 0].sum().item()),
                      "evaluated": int(counts[:, 1].sum().item()), "pairs": [int(v) for v in total[0, :, 0].tolist()]},
           "offsets": [[int(dh), int(dw)] for dh, dw in offsets],
           "sums": {name: total[c, :, 1:].tolist() for c, name in enumerate(("depth", "reflectance"))}, "micro": {}, "macro": {}}
    micro = derived_coherence(counts.sum(0), torch.zeros(2, K + 1, K + 1, dtype=torch.float64), total)
    for name, v in micro.items():
        if name.startswith("variogram"):
            out["micro"][name] = v.tolist() if v.dim() else v.item()
    for name, v in derived_coherence(counts, dist, vario).items():
        ok = ~v.isnan()
        mean = torch.where(ok, v, torch.zeros_like(v)).sum(0) / ok.sum(0)  # 0 / 0 = NaN where no scan has the value
        out["macro"][name] = mean.tolist() if mean.dim() else mean.item()
    return out


# ---- labels ------------------------------------------------------------------------------------------------------------------------------
def confusion_matrix(pred: torch.Tensor, target: torch.Tensor, num_classes: int, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int64 (B,C,C) counts ``[b][target][pred]`` of two int64 label tensors (B,...) over the pixels whose ``mask`` (same shape, None: all)
    is not 0.  An unmasked label outside ``[0, num_classes)`` raises ``ValueError`` (one read of a device counter per call)."""
    _lib.require_gpu(pred, "pred")
    C = int(num_classes)
    if not 1 <= C <= 64:
        raise ValueError(f"num_classes must be in [1, 64], got {num_classes}")
    if pred.dim() < 1 or target.shape != pred.shape or (mask is not None and mask.shape != pred.shape):
        raise ValueError(f"pred {tuple(pred.shape)}, target {tuple(target.shape)} and mask {None if mask is None else tuple(mask.shape)} "
                         "must have one (B,...) shape")
    if pred.dtype != torch.int64 or target.dtype != torch.int64:
        raise ValueError(f"labels must be int64, got {pred.dtype} and {target.dtype}")
    dev, B = pred.device, pred.shape[0]
    counts = torch.zeros(B, C, C, dtype=torch.int64, device=dev)
    n = pred.numel() // max(B, 1)
    if B == 0 or n == 0:
        return counts
    pred, target = pred.reshape(B, n).contiguous(), target.to(dev).reshape(B, n).contiguous()
    mask = None if mask is None else _lib.f32c(mask.to(dev).reshape(B, n))
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().r2dm_confusion_matrix(_lib.ptr(pred), _lib.ptr(target), _lib.ptr(mask), B, n, C, _lib.ptr(counts), _lib.ptr(bad),
                                                    _lib.stream_ptr(dev)))
        nbad = int(bad.item())
    if nbad:
        raise ValueError(f"confusion_matrix: {nbad} unmasked pixels carry a label outside [0, {C})")
    return counts


def iou_from_confusion(conf, ignore: Sequence[int] = (0,)):
    """``conf`` (...,C,C) counts ``[target][pred]`` (leading dimensions are summed) -> ``(iou (C,) float64, mIoU float)`` on the host.  The
    pixels whose *target* is an ignored class are dropped (SemanticKITTI's class 0 is "unlabeled"); IoU_c = tp / (tp + fp + fn); a class
    absent from both target and prediction, and an ignored class, is NaN; mIoU is the mean over the other classes (NaN if there is none)."""
    conf = torch.as_tensor(conf).detach().cpu().double()
    if conf.dim() < 2 or conf.shape[-1] != conf.shape[-2]:
        raise ValueError(f"expected (...,C,C) counts, got {tuple(conf.shape)}")
    C = conf.shape[-1]
    conf = conf.reshape(-1, C, C).sum(0)
    ignore = sorted({int(c) for c in ignore})
    if any(not 0 <= c < C for c in ignore):
        raise ValueError(f"ignored classes {ignore} outside [0, {C})")
    conf[ignore, :] = 0
    tp = conf.diagonal()
    union = conf.sum(0) + conf.sum(1) - tp  # tp + fp + fn
    iou = _ratio(tp, union)
    iou[ignore] = math.nan
    valid = ~iou.isnan()
    return iou, (iou[valid].mean().item() if valid.any() else math.nan)


# ---- baselines ---------------------------------------------------------------------------------------------------------------------------
def fill_beams(x: torch.Tensor, rows: torch.Tensor, mode: str, nodata: float = -1.0) -> torch.Tensor:
    """``x`` (B,C,H,W), ``rows`` (B,H) (non-zero / True = this beam is known) -> (B,C,H,W): known rows copied, every other row from the
    nearest known row above and below (``mode`` "nearest", the upper one on a tie, or "linear" in fp32), per column and only from endpoints
    whose channel 0 is not ``nodata``; ``nodata`` in every channel where there is none.  Rows do not wrap."""
    if mode not in FILL_MODES:
        raise ValueError(f"mode must be one of {sorted(FILL_MODES)}, got {mode!r}")
    _lib.require_gpu(x, "x")
    if x.dim() != 4:
        raise ValueError(f"expected x (B,C,H,W), got {tuple(x.shape)}")
    B, C, H, W = x.shape
    if tuple(rows.shape) != (B, H):
        raise ValueError(f"rows {tuple(rows.shape)} must be (B,H) = {(B, H)}")
    if math.isnan(float(nodata)):
        raise ValueError("nodata must be a number: NaN compares unequal to itself")
    x = _lib.f32c(x)
    rows = (rows.to(x.device) != 0).to(torch.uint8).contiguous()
    out = torch.empty_like(x)
    if x.numel() == 0:
        return out
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().r2dm_fill_beams(_lib.ptr(x), _lib.ptr(rows), _lib.ptr(out), B, C, H, W, float(nodata), FILL_MODES[mode],
                                              _lib.stream_ptr(x.device)))
    return out


# ---- aggregation (host, float64) ---------------------------------------------------------------------------------------------------------
def aggregate_errors(raw: torch.Tensor) -> dict:
    """(N,10) per-scan raw values -> ``{"counts", "sums", "micro", "macro"}``: micro = the derived values of the sums over all scans
    (summed errors over summed counts), macro = the mean of the per-scan derived values, ignoring the NaN ones.  NaN where undefined."""
    raw = torch.as_tensor(raw).detach().cpu().double().reshape(-1, len(RAW_NAMES))
    total = raw.sum(0)
    out = {"counts": {"scans": int(raw.shape[0]), **{name: int(total[k].item()) for k, name in enumerate(RAW_NAMES[:4])}},
           "sums": {name: total[k].item() for k, name in enumerate(RAW_NAMES) if k >= 4},
           "micro": {name: v.item() for name, v in derived_errors(total).items()}, "macro": {}}
    out["counts"]["unknown_without_return"] = out["counts"]["unknown"] - out["counts"]["evaluated"]
    for name, v in derived_errors(raw).items():
        ok = ~v.isnan()
        out["macro"][name] = v[ok].mean().item() if ok.any() else math.nan
    return out


def jsonable(obj):
    """The same structure with every non-finite float as None (JSON ``null``) and tensors as lists."""
    if isinstance(obj, dict):
        return {str(k): jsonable(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [jsonable(v) for v in obj]
    if isinstance(obj, torch.Tensor):
        return jsonable(obj.tolist())
    if isinstance(obj, float):
        return obj if math.isfinite(obj) else None
    return obj


# ---- the evaluation ----------------------------------------------------------------------------------------------------------------------
def rows_of_mask(mask: torch.Tensor) -> torch.Tensor:
    """(B,1,H,W) mask of whole rows -> (B,H) uint8, 1 = the row is known"""
    return (mask[:, 0] != 0).all(dim=-1).to(torch.uint8)


def target_of_planes(planes: torch.Tensor) -> torch.Tensor:
    """(N,6,H,W) [x, y, z, reflectance, depth, mask] -> the sample layout (N,5,H,W) [depth, x, y, z, reflectance]"""
    return planes[:, [4, 0, 1, 2, 3]].float().contiguous()


@torch.no_grad()
def evaluate_completion(ddpm, lidar_utils, planes: torch.Tensor, kinds: Sequence[str], methods: Sequence[str] = ("repaint",), num_steps: int = 32,
                        num_resample_steps: int = 10, jump_length: int = 1, seed: int = 0, batch_size: int = 8, semseg=None,
                        semseg_postprocess=None, lo: Optional[float] = None, hi: Optional[float] = None, keep: bool = False,
                        chamfer: bool = False, fscore_threshold: float = 0.2, ddnm_resample_steps: int = 1, ddnm_init: Optional[str] = None,
                        ddnm_t_start: float = 1.0, dpmpp_eta: float = 1.0, dpmpp_order: int = 2, dpmpp_init: Optional[str] = None,
                        dpmpp_t_start: float = 1.0, ensemble: Optional[int] = None, ensemble_coherence: bool = False,
                        coherence_offsets=None, voxel_sizes=None):
    """Corrupt, complete and score ``planes`` (N,6,H,W), the masked planes of ``project_scans(layout="xyzrdm", apply_mask=True)`` at the
    model's resolution, on the GPU.

    For every kind of ``kinds`` (``corruption_mask``) and every scan i: the mask is drawn from a CPU generator seeded ``scan_seed(seed, i)``
    and RePaint draws from ``setup_rng([scan_seed(seed, i)])``, so a scan's inputs depend neither on ``batch_size`` nor on the scans after
    it.  ``x_in = mask * known + (1 - mask) * -1`` with ``known = known_from_scan(planes)``; a method's prediction is
    ``lidar_utils.postprocess(x_out.clamp(-1, 1))``; the target is the scan's own measured planes, not a decode of ``known``.
    ``methods``: "repaint"; "ddnm" (``ddpm.complete`` on ``x_in`` under the mask, from the same generators as RePaint, ``num_steps`` and
    ``jump_length`` shared with it and ``ddnm_resample_steps`` resamplings; with ``ddnm_init`` "nearest" / "linear" it starts from
    ``fill_beams(x_in, ...)`` noised to ``ddnm_t_start`` < 1 instead of from noise at t = 1 -- defined, like the baselines, for the kinds
    whose mask is whole rows and reported as skipped for the others); "dpmpp" (``ddpm.complete_dpm``: the same projection on DPM-Solver++(2M),
    ``num_steps`` steps of order ``dpmpp_order`` with ``dpmpp_eta``, from the same generators as RePaint, no resampling; ``dpmpp_init`` /
    ``dpmpp_t_start`` as ``ddnm_init`` / ``ddnm_t_start``, with the same rules); "nearest" / "linear" (``fill_beams`` on ``x_in``; defined for the kinds whose mask is whole rows, reported as
    skipped for the others); "target" (the target's own planes as the prediction: errors 0, mIoU 1).  ``lo``, ``hi``: the depth window of
    a return (default: the model's ``min_depth``, ``max_depth``).  ``semseg``: a ``RangeNetExtractor``; the labels of prediction and target
    come from the same net and ``semseg_postprocess`` (what ``segment`` accepts), the confusion matrix is taken over the target's measured
    pixels of the whole image.  ``chamfer``: also score the completion in 3-D (``r2dm_amd.geometry``): the prediction's returns as a point
    cloud against the target's, over the whole image (``"all"``) and over the unknown pixels only (``"inpainted"``), with the F-score at
    ``fscore_threshold`` metres.

    -> ``results[kind][method]`` = ``aggregate_errors`` of the scans (counts, sums, micro and macro averages) plus, with ``semseg``,
    ``"iou": {"per_class", "miou", "pixels"}`` and, with ``chamfer``, ``"geometry": {"all", "inpainted"}``, each the
    ``geometry.aggregate_chamfer`` of the scans (micro and macro ``cd_sq``, ``cd``, ``precision``, ``recall``, ``fscore``, the number of
    scans with an empty cloud); or ``{"skipped": why}``.  ``keep=True``: ``(results, kept)`` with ``kept[kind]`` =
    ``{"mask", "x_in", "target", "x_out": {method}, "pred": {method}, "raw": {method}}`` and, with ``semseg``, ``"target_labels"``,
    ``"labels": {method}`` and ``"confusion": {method}``, with ``chamfer`` ``"geometry_raw": {method: {"all", "inpainted"}}`` ((N,8) sums,
    ``geometry.RAW_NAMES``), all on the CPU.

    ``ensemble`` = K (1 to 64): every stochastic method ("repaint", "ddnm", "dpmpp") draws K members per scan, member k of scan i from
    ``setup_rng([member_seed(seed, i, k)])``, all under the scan's one mask; members fill the batch (``batch_size`` counts members) and, the
    generators being per sample, a member does not depend on the batch it is drawn in.  Member 0 is the single draw of a run without
    ``ensemble``, and everything above is still scored on it.  A deterministic method is an ensemble of one.  Every entry gains
    ``"ensemble"``: ``{"members", **aggregate_ensemble(...), "consensus"}`` with ``consensus`` the ``aggregate_errors`` of
    ``ensemble_consensus`` (median depth where at least half of the members return, mean reflectance); ``kept[kind]["ensemble"][method]`` =
    ``{"raw" (N,13), "member" (N,2,K), "rank" (N,K+1), "consensus_raw" (N,10), "maps" (N,8,H,W), "x_out" (N,K,2,H,W) or None}``.  None
    (the default): nothing of this is computed, and keys and numbers are what they were.

    ``ensemble_coherence=True`` (with ``ensemble``; without it a ``ValueError``): the members are also scored across pixels
    (``ensemble_coherence_sums`` with ``coherence_offsets``, None: ``DEFAULT_OFFSETS``): every entry's ``"ensemble"`` gains ``"coherence"``
    = ``aggregate_coherence(...)`` (energy score, variogram score, diversity) and ``kept[kind]["ensemble"][method]`` gains ``"counts"``
    (N,2), ``"dist"`` (N,2,K+1,K+1), ``"vario"`` (N,2,O,4) and ``"offsets"``.  False (the default): none of it is computed.

    ``voxel_sizes`` = 1 to 8 voxel sizes in metres: also the voxel occupancy of the clouds ``chamfer`` scores (``geometry.voxel_iou``): every
    entry gains ``"voxel": {"sizes", "all", "inpainted"}``, each the ``geometry.aggregate_voxel`` of the scans (micro and macro ``iou``,
    ``precision``, ``recall``, ``f1``, a list over the sizes), and ``kept[kind]["voxel_raw"][method]`` = ``{"all", "inpainted"}`` holds the
    (N,S,3) counts ``[intersection, voxels of the prediction, voxels of the target]``.  With ``ensemble`` (at most 63 members then: a
    ``ValueError`` for 64) the members vote on every voxel: ``entry["ensemble"]`` gains ``"occupancy": {"sizes", "all", "inpainted"}``, each
    the ``geometry.aggregate_occupancy`` of the scans (the members' IoU, "any" and "consensus" occupancy against the target, the Brier score
    of the occupancy probability, the reliability curve), and ``kept[kind]["ensemble"][method]`` gains ``"occupancy"`` = ``{"all",
    "inpainted"}``, each ``{"member" (N,S,K,2), "hist" (N,S,2,K+1)}``.  None (the default): none of it is computed."""
    from . import geometry
    from .inference import setup_rng
    from .projection import known_from_scan

    if ddnm_init is not None and ddnm_init not in FILL_MODES:
        raise ValueError(f"ddnm_init must be None or one of {sorted(FILL_MODES)}, got {ddnm_init!r}")
    if (ddnm_init is None) != (float(ddnm_t_start) == 1.0):
        raise ValueError(f"ddnm_init and ddnm_t_start < 1 go together (a start from the interpolated scan, noised to ddnm_t_start): got {ddnm_init!r} "
                         f"and {ddnm_t_start}")
    if not 0.0 < float(ddnm_t_start) <= 1.0:
        raise ValueError(f"ddnm_t_start must be in (0, 1], got {ddnm_t_start}")
    if ddnm_resample_steps < 1:
        raise ValueError(f"ddnm_resample_steps must be >= 1, got {ddnm_resample_steps}")
    if dpmpp_init is not None and dpmpp_init not in FILL_MODES:
        raise ValueError(f"dpmpp_init must be None or one of {sorted(FILL_MODES)}, got {dpmpp_init!r}")
    if (dpmpp_init is None) != (float(dpmpp_t_start) == 1.0):
        raise ValueError(f"dpmpp_init and dpmpp_t_start < 1 go together (a start from the interpolated scan, noised to dpmpp_t_start): got {dpmpp_init!r} "
                         f"and {dpmpp_t_start}")
    if not 0.0 < float(dpmpp_t_start) <= 1.0:
        raise ValueError(f"dpmpp_t_start must be in (0, 1], got {dpmpp_t_start}")
    if dpmpp_order not in (1, 2):
        raise ValueError(f"dpmpp_order must be 1 or 2, got {dpmpp_order!r}")
    if not float(dpmpp_eta) >= 0.0 or float(dpmpp_eta) == float("inf"):
        raise ValueError(f"dpmpp_eta must be finite and >= 0, got {dpmpp_eta}")
    if ensemble is not None and not (isinstance(ensemble, int) and 1 <= ensemble <= MAX_MEMBERS):
        raise ValueError(f"ensemble must be None or a number of members in [1, {MAX_MEMBERS}], got {ensemble!r}")
    if ensemble_coherence and ensemble is None:
        raise ValueError("ensemble_coherence scores the members of an ensemble: give ensemble = K as well")
    if voxel_sizes is not None:
        voxel_sizes = [float(v) for v in geometry._voxel_sizes(voxel_sizes)]
        if ensemble is not None:
            geometry._check_members(ensemble)
    if planes.dim() != 4 or planes.shape[1] != 6:
        raise ValueError(f"expected planes (N,6,H,W) [x, y, z, reflectance, depth, mask], got {tuple(planes.shape)}")
    _lib.require_gpu(planes, "planes")
    for m in methods:
        if m not in METHODS:
            raise ValueError(f"unknown method {m!r}: expected one of {METHODS}")
    parsed = {kind: parse_kind(kind) for kind in kinds}
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    if chamfer:
        fscore_threshold = geometry._check_tau(fscore_threshold)
    N, _, H, W = planes.shape
    if ensemble_coherence:
        coherence_offsets = tuple(o for o in DEFAULT_OFFSETS if abs(o[0]) < H and abs(o[1]) < W) if coherence_offsets is None \
            else _check_offsets(coherence_offsets, H, W)
    if ("repaint" in methods or "ddnm" in methods or "dpmpp" in methods) and tuple(ddpm.sampling_shape) != (2, H, W):
        raise ValueError(f"planes of {H}x{W} for a model that samples {tuple(ddpm.sampling_shape)}: RePaint needs a depth + reflectance model "
                         "at the planes' resolution")
    dev = planes.device
    lo = float(lidar_utils.min_depth if lo is None else lo)
    hi = float(lidar_utils.max_depth if hi is None else hi)
    known = known_from_scan(planes, lidar_utils, (H, W))
    target = target_of_planes(planes)
    measured = torch.logical_and(target[:, [0]] > lo, target[:, [0]] < hi).float()

    def labels_of(img):
        m = torch.logical_and(img[:, [0]] > lo, img[:, [0]] < hi).float()
        return torch.cat([semseg.segment(img[k:k + batch_size], m[k:k + batch_size], postprocess=semseg_postprocess)
                          for k in range(0, N, batch_size)]) if N else torch.empty(0, 1, H, W, dtype=torch.int64, device=dev)

    def geometry_of(pred, region):
        raws = []
        for k in range(0, N, batch_size):
            reg = None if region is None else region[k:k + batch_size]
            raws.append(geometry.chamfer_sums(*geometry.clouds_of_samples(pred[k:k + batch_size], lo, hi, reg),
                                              *geometry.clouds_of_samples(target[k:k + batch_size], lo, hi, reg), tau=fscore_threshold).cpu())
        return torch.cat(raws) if raws else torch.empty(0, len(geometry.RAW_NAMES), dtype=torch.float64)

    def voxel_of(pred, region):
        raws = []
        for k in range(0, N, batch_size):
            reg = None if region is None else region[k:k + batch_size]
            raws.append(geometry.voxel_iou(*geometry.clouds_of_samples(pred[k:k + batch_size], lo, hi, reg),
                                           *geometry.clouds_of_samples(target[k:k + batch_size], lo, hi, reg), sizes=voxel_sizes)["counts"].cpu())
        return torch.cat(raws) if raws else torch.empty(0, len(voxel_sizes), 3, dtype=torch.int64)

    def occupancy_of(samples, tgt, region):
        """the members of every scan of a batch, (B,K,5,H,W), vote on the voxels: (member (B,S,K,2), hist (B,S,2,K+1)) on the CPU"""
        B, K = samples.shape[:2]
        reg = None if region is None else region.repeat_interleave(K, dim=0)
        res = geometry.voxel_occupancy_counts(*geometry.clouds_of_samples(samples.flatten(0, 1), lo, hi, reg),
                                              *geometry.clouds_of_samples(tgt, lo, hi, region), torch.arange(B * K).reshape(B, K), torch.arange(B),
                                              voxel_sizes)
        return res["member"].cpu(), res["hist"].cpu()

    target_labels = labels_of(target) if semseg is not None else None
    results, kept = {}, {}
    for kind, (name, _) in parsed.items():
        mask = torch.stack([corruption_mask(kind, H, W, torch.Generator().manual_seed(scan_seed(seed, i))) for i in range(N)]).to(dev) \
            if N else torch.empty(0, 1, H, W, device=dev)
        x_in = mask * known + (1 - mask) * -1
        results[kind] = {}
        if keep:
            kept[kind] = {"mask": mask.cpu(), "x_in": x_in.cpu(), "target": target.cpu(), "x_out": {}, "pred": {}, "raw": {}}
            if semseg is not None:
                kept[kind].update(target_labels=target_labels.cpu(), labels={}, confusion={})
            if chamfer:
                kept[kind]["geometry_raw"] = {}
            if voxel_sizes is not None:
                kept[kind]["voxel_raw"] = {}
        for method in methods:
            if method in FILL_MODES and name not in ROW_KINDS:
                results[kind][method] = {"skipped": f"{method} interpolation is defined for masks of whole rows ({', '.join(ROW_KINDS)})"}
                continue
            if method == "ddnm" and ddnm_init is not None and name not in ROW_KINDS:
                results[kind][method] = {"skipped": f"ddnm_init = {ddnm_init} interpolation is defined for masks of whole rows ({', '.join(ROW_KINDS)})"}
                continue
            if method == "dpmpp" and dpmpp_init is not None and name not in ROW_KINDS:
                results[kind][method] = {"skipped": f"dpmpp_init = {dpmpp_init} interpolation is defined for masks of whole rows ({', '.join(ROW_KINDS)})"}
                continue
            members = ensemble if ensemble is not None and method in STOCHASTIC_METHODS else 1
            x_members = None
            if method in STOCHASTIC_METHODS:
                how = {"dpmpp": dpmpp_init, "ddnm": ddnm_init, "repaint": None}[method]
                init = fill_beams(x_in, rows_of_mask(mask), how, nodata=-1.0) if how is not None and N else None
                jobs = [(i, k) for i in range(N) for k in range(members)]  # a scan's members adjacent; member 0 is the single draw
                parts = []
                for j in range(0, len(jobs), batch_size):
                    job = jobs[j:j + batch_size]
                    idx = torch.tensor([i for i, _ in job], device=dev)
                    rng = setup_rng([member_seed(seed, i, k) for i, k in job], dev)
                    kn, mk, it = x_in[idx], mask[idx], None if init is None else init[idx]
                    if method == "dpmpp":
                        parts.append(ddpm.complete_dpm(known=kn, mask=mk, num_steps=num_steps, order=dpmpp_order, eta=float(dpmpp_eta),
                                                       t_start=float(dpmpp_t_start), init=it, progress=False, rng=rng))
                    elif method == "ddnm":
                        parts.append(ddpm.complete(known=kn, mask=mk, num_steps=num_steps, num_resample_steps=ddnm_resample_steps,
                                                   jump_length=jump_length, t_start=float(ddnm_t_start), init=it, progress=False, rng=rng))
                    else:
                        parts.append(ddpm.repaint(known=kn, mask=mk, num_steps=num_steps, num_resample_steps=num_resample_steps,
                                                  jump_length=jump_length, progress=False, rng=rng))
                x_members = torch.cat(parts).reshape(N, members, *x_in.shape[1:]) if parts else x_in[:, None]
                x_out = x_members[:, 0].contiguous()
            elif method in FILL_MODES:
                x_out = fill_beams(x_in, rows_of_mask(mask), method, nodata=-1.0) if N else x_in
            else:
                x_out = None
            pred = target if x_out is None else lidar_utils.postprocess(x_out.clamp(-1, 1))
            raw = completion_error_sums(pred, target, mask, lo, hi).cpu()
            entry = aggregate_errors(raw)
            if semseg is not None:
                labels = target_labels if x_out is None else labels_of(pred)
                conf = confusion_matrix(labels, target_labels, semseg.num_classes, measured).cpu()
                iou, miou = iou_from_confusion(conf)
                entry["iou"] = {"per_class": iou.tolist(), "miou": miou, "pixels": int(conf.sum().item())}
            if chamfer:
                graw = {"all": geometry_of(pred, None), "inpainted": geometry_of(pred, mask == 0)}
                entry["geometry"] = {where: geometry.aggregate_chamfer(r) for where, r in graw.items()}
            if voxel_sizes is not None:
                vraw = {"all": voxel_of(pred, None), "inpainted": voxel_of(pred, mask == 0)}
                entry["voxel"] = {"sizes": voxel_sizes, **{where: geometry.aggregate_voxel(r, voxel_sizes) for where, r in vraw.items()}}
            if ensemble is not None:
                eraw, emember, erank, emaps, craw = [], [], [], [], []
                ccounts, cdist, cvario = [], [], []
                occ = {"all": ([], []), "inpainted": ([], [])}
                for k in range(0, N, batch_size):
                    if x_members is None or members == 1:
                        samples = pred[k:k + batch_size, None]
                    else:
                        xs = x_members[k:k + batch_size]
                        samples = lidar_utils.postprocess(xs.flatten(0, 1).clamp(-1, 1)).reshape(xs.shape[0], members, 5, H, W)
                    r, m, h, maps = ensemble_score_sums(samples, target[k:k + batch_size], mask[k:k + batch_size], lo, hi, maps=True)
                    craw.append(completion_error_sums(ensemble_consensus(maps, lidar_utils), target[k:k + batch_size], mask[k:k + batch_size],
                                                      lo, hi).cpu())
                    eraw.append(r.cpu()), emember.append(m.cpu()), erank.append(h.cpu())
                    if ensemble_coherence:
                        cc, cd, cv, _ = ensemble_coherence_sums(samples, target[k:k + batch_size], mask[k:k + batch_size], lo, hi, coherence_offsets)
                        ccounts.append(cc.cpu()), cdist.append(cd.cpu()), cvario.append(cv.cpu())
                    if voxel_sizes is not None:
                        for where, region in (("all", None), ("inpainted", mask[k:k + batch_size] == 0)):
                            om, oh = occupancy_of(samples, target[k:k + batch_size], region)
                            occ[where][0].append(om), occ[where][1].append(oh)
                    if keep:
                        emaps.append(maps.cpu())
                eraw = torch.cat(eraw) if eraw else torch.empty(0, len(ENSEMBLE_RAW_NAMES), dtype=torch.float64)
                emember = torch.cat(emember) if emember else torch.empty(0, 2, members, dtype=torch.float64)
                erank = torch.cat(erank) if erank else torch.empty(0, members + 1, dtype=torch.int64)
                craw = torch.cat(craw) if craw else torch.empty(0, len(RAW_NAMES), dtype=torch.float64)
                entry["ensemble"] = {"members": members, **aggregate_ensemble(eraw, emember, erank), "consensus": aggregate_errors(craw)}
                if ensemble_coherence:
                    ccounts = torch.cat(ccounts) if ccounts else torch.empty(0, 2, dtype=torch.float64)
                    cdist = torch.cat(cdist) if cdist else torch.empty(0, 2, members + 1, members + 1, dtype=torch.float64)
                    cvario = torch.cat(cvario) if cvario else torch.empty(0, 2, len(coherence_offsets), 4, dtype=torch.float64)
                    entry["ensemble"]["coherence"] = aggregate_coherence(ccounts, cdist, cvario, coherence_offsets)
                if voxel_sizes is not None:
                    S = len(voxel_sizes)
                    occ = {where: {"member": torch.cat(m) if m else torch.empty(0, S, members, 2, dtype=torch.int64),
                                   "hist": torch.cat(h) if h else torch.empty(0, S, 2, members + 1, dtype=torch.int64)} for where, (m, h) in occ.items()}
                    entry["ensemble"]["occupancy"] = {"sizes": voxel_sizes, **{where: geometry.aggregate_occupancy(o["member"], o["hist"], voxel_sizes)
                                                                              for where, o in occ.items()}}
            results[kind][method] = entry
            if keep:
                if ensemble is not None:
                    kept[kind].setdefault("ensemble", {})[method] = {
                        "raw": eraw, "member": emember, "rank": erank, "consensus_raw": craw,
                        "maps": torch.cat(emaps) if emaps else torch.empty(0, len(ENSEMBLE_MAP_NAMES), H, W),
                        "x_out": None if x_members is None else x_members.cpu()}
                    if ensemble_coherence:
                        kept[kind]["ensemble"][method].update(counts=ccounts, dist=cdist, vario=cvario, offsets=coherence_offsets)
                    if voxel_sizes is not None:
                        kept[kind]["ensemble"][method]["occupancy"] = occ
                kept[kind]["x_out"][method] = None if x_out is None else x_out.cpu()
                kept[kind]["pred"][method] = pred.cpu()
                kept[kind]["raw"][method] = raw
                if semseg is not None:
                    kept[kind]["labels"][method] = labels.cpu()
                    kept[kind]["confusion"][method] = conf
                if chamfer:
                    kept[kind]["geometry_raw"][method] = graw
                if voxel_sizes is not None:
                    kept[kind]["voxel_raw"][method] = vraw
    return (results, kept) if keep else results
