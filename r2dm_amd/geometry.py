"""Geometry metrics: how far two scans are from each other in 3-D.

Clouds are sets of 3-D points in metres; ``d(x, Y) = min_{y in Y} |x - y|``.

- nearest neighbour X -> Y: for every x, ``d^2(x, Y)`` and the index of the minimiser, the lowest one on an exact fp32 tie; against an
  empty Y ``+inf`` and ``-1``.
- Chamfer distance of a pair: ``cd_sq = mean_x d^2(x, Y) + mean_y d^2(y, X)`` and ``cd = (mean_x d(x, Y) + mean_y d(y, X)) / 2``.
- F-score at ``tau``: ``precision = |{x: d(x, Y) <= tau}| / |X|`` with X the prediction, ``recall = |{y: d(y, X) <= tau}| / |Y|``,
  ``fscore = 2 P R / (P + R)``, 0 if ``P + R = 0``.  All five are NaN if either cloud is empty.
- set metrics of generated clouds G against real clouds R under ``D = cd_sq`` (the PointFlow / LiDM definitions):
  ``COV = |{argmin_r D(g, r): g in G}| / |R|``, ``MMD = mean_r min_g D(g, r)``, ``1-NNA`` = over S = G u R the fraction of s whose nearest
  neighbour in S \\ {s} lies in the same set as s (0.5 is ideal).  Every argmin tie goes to the lowest index, G before R.
- earth mover's distance of two clouds of the same number n of points: ``EMD = (1/n) min_sigma sum_i |a_i - b_sigma(i)|`` over the
  permutations sigma (Euclidean, not squared: PointFlow's convention).  ``emd_pairs`` returns a permutation, its true cost ``emd`` and a
  certified ``lower <= EMD <= emd``; the set metrics above take its matrix (``pairwise_emd``) as they take ``cd_sq``'s.
- voxel occupancy at voxel size s: the voxel of a point is ``floor(x / s), floor(y / s), floor(z / s)`` (IEEE float32 divisions, a grid
  anchored at the origin), ``V(X)`` the set of voxels of cloud X.  ``voxel_iou``: ``|V(A) n V(B)| / |V(A) u V(B)|`` with precision, recall
  and F1 of the voxel sets.  For an ensemble of K clouds against a target, ``voxel_occupancy_counts`` gives per voxel of the union the
  number c of members that occupy it and whether the target does, as a ``2 x (K + 1)`` histogram; ``occupancy_from_counts`` derives the
  members' IoU, the "any" (c >= 1) and "consensus" (2 c >= K) occupancy against the target, the Brier score of the occupancy probability
  c / K and its reliability curve.  All of it from integer counts: exact, and the same bits in any order.

The search is one HIP kernel (``r2dm_nn_pairs``, ``r2dm_amd/csrc/geometry.hip``) over a list of cloud pairs, the assignment solver another
(``r2dm_emd_pairs``, ``r2dm_amd/csrc/emd.hip``), the voxel sets a hash set in global memory (``r2dm_voxel_occupancy``,
``r2dm_amd/csrc/voxel.hip``); none has a CPU fallback.
What is derived from its sums and from distance matrices is plain torch and works on CPU tensors too."""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib

RAW_NAMES = ("sum_sq_ab", "sum_d_ab", "within_ab", "sum_sq_ba", "sum_d_ba", "within_ba", "count_a", "count_b")
DERIVED_NAMES = ("cd_sq", "cd", "precision", "recall", "fscore")
MAX_POINTS = 1 << 21          # per cloud (r2dm_nn_pairs)
SLAB_BYTES = 64 << 20         # pairwise_chamfer: pair list + sums + scratch of one call stay below this


# ---- the search --------------------------------------------------------------------------------------------------------------------------
def _host_offsets(offsets, total: int, what: str) -> np.ndarray:
    off = offsets.detach().cpu().numpy() if isinstance(offsets, torch.Tensor) else np.asarray(offsets)
    if off.ndim != 1 or off.size < 2 or off.dtype.kind not in "iu":
        raise ValueError(f"{what}: expected (clouds + 1,) integer offsets with at least one cloud, got shape {off.shape} {off.dtype}")
    off = off.astype(np.int64)
    if off[0] < 0 or (np.diff(off) < 0).any() or off[-1] > total:
        raise ValueError(f"{what}: offsets must ascend from >= 0 to at most the {total} rows of the points")
    if np.diff(off).max() > MAX_POINTS:
        raise ValueError(f"{what}: a cloud of {int(np.diff(off).max())} points; the search takes clouds of up to 2^21 = {MAX_POINTS}")
    return off


def _points(p: torch.Tensor, what: str) -> torch.Tensor:
    if p.dim() != 2 or p.shape[1] != 4:
        raise ValueError(f"{what}: expected (total,4) rows [x, y, z, .], got {tuple(p.shape)}")
    _lib.require_gpu(p, what)
    p = _lib.f32c(p)
    return p.clone() if p.data_ptr() % 16 else p  # rows are read as quads


def _pairs(pairs, na: int, nb: int) -> np.ndarray:
    if pairs is None:
        if na != nb:
            raise ValueError(f"pairs=None pairs cloud k with cloud k: {na} clouds against {nb}")
        k = np.arange(na, dtype=np.int64)
        return np.stack([k, k], axis=1)
    pr = pairs.detach().cpu().numpy() if isinstance(pairs, torch.Tensor) else np.asarray(pairs)
    if pr.ndim != 2 or pr.shape[1] != 2 or pr.dtype.kind not in "iu":
        raise ValueError(f"pairs: expected (P,2) integers [ia, ib], got shape {pr.shape} {pr.dtype}")
    pr = pr.astype(np.int64)
    if pr.size and (pr.min() < 0 or pr[:, 0].max() >= na or pr[:, 1].max() >= nb):
        raise ValueError(f"pairs: an index outside the {na} clouds of a or the {nb} clouds of b")
    return pr


def _check_tau(tau: float) -> float:
    tau = float(tau)
    if not (math.isfinite(tau) and tau >= 0):
        raise ValueError(f"the F-score threshold must be a finite distance >= 0, got {tau}")
    return tau


def _launch(a, off_a, clouds_a, b, off_b, clouds_b, pairs_dev, max_points, tau, per_point=None):
    """One ``r2dm_nn_pairs`` call on device tensors -> ``(sums (P,8), status (2,))``, nothing read back.  ``per_point``: None or
    ``(d2_ab, idx_ab, start_ab, d2_ba, idx_ba, start_ba)``."""
    dev, P = a.device, pairs_dev.shape[0]
    L = _lib.lib()
    nbytes = L.r2dm_nn_pairs_scratch_bytes(P, max_points)
    if nbytes == 0:
        raise ValueError(f"{P} pairs of clouds of up to {max_points} points: beyond the limits of r2dm_nn_pairs (clouds of up to 2^21 points, "
                         "2 * pairs * ceil(points / 1024) at most 2^31 - 1 blocks)")
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    sums = torch.empty(P, len(RAW_NAMES), dtype=torch.float64, device=dev)
    status = torch.empty(2, dtype=torch.int64, device=dev)
    pp = [None] * 6 if per_point is None else [_lib.ptr(t) for t in per_point]
    with torch.cuda.device(dev):
        _lib.check(L.r2dm_nn_pairs(_lib.ptr(a) or None, _lib.ptr(off_a), clouds_a, a.shape[0], _lib.ptr(b) or None, _lib.ptr(off_b), clouds_b, b.shape[0],
                                   _lib.ptr(pairs_dev), P, max_points, tau, *pp, _lib.ptr(scratch), _lib.ptr(sums), _lib.ptr(status),
                                   _lib.stream_ptr(dev)))
    return sums, status


def _raise_on_status(status: torch.Tensor) -> None:
    nonfinite, bad = (int(v) for v in status.cpu().tolist())
    if bad:
        raise _lib.R2DMError(f"r2dm_nn_pairs: {bad} pairs with an index or offsets that do not check out")
    if nonfinite:
        raise ValueError(f"nearest neighbours: {nonfinite} points with a non-finite coordinate (counted once per pair they are part of)")


def _search(a, a_offsets, b, b_offsets, pairs, tau, per_point: bool, return_index: bool):
    a, b = _points(a, "a"), _points(b, "b")
    if b.device != a.device:
        raise ValueError(f"a is on {a.device}, b on {b.device}")
    off_a, off_b = _host_offsets(a_offsets, a.shape[0], "a_offsets"), _host_offsets(b_offsets, b.shape[0], "b_offsets")
    pr = _pairs(pairs, off_a.size - 1, off_b.size - 1)
    tau = _check_tau(tau)
    dev, P = a.device, pr.shape[0]
    out = {"sums": torch.empty(0, len(RAW_NAMES), dtype=torch.float64, device=dev)}
    na, nb = np.diff(off_a)[pr[:, 0]], np.diff(off_b)[pr[:, 1]]
    start_ab, start_ba = np.concatenate([[0], np.cumsum(na)]).astype(np.int64), np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
    pp = None
    if per_point:
        out.update(d2_ab=torch.empty(int(start_ab[-1]), dtype=torch.float32, device=dev), start_ab=start_ab,
                   d2_ba=torch.empty(int(start_ba[-1]), dtype=torch.float32, device=dev), start_ba=start_ba)
        if return_index:
            out.update(idx_ab=torch.empty(int(start_ab[-1]), dtype=torch.int32, device=dev),
                       idx_ba=torch.empty(int(start_ba[-1]), dtype=torch.int32, device=dev))
    if P == 0:
        return out
    if per_point:
        s_ab, s_ba = torch.from_numpy(start_ab[:-1].copy()).to(dev), torch.from_numpy(start_ba[:-1].copy()).to(dev)
        pp = (out["d2_ab"], out.get("idx_ab"), s_ab, out["d2_ba"], out.get("idx_ba"), s_ba)
    max_points = max(int(max(na.max(), nb.max())), 1)
    sums, status = _launch(a, torch.from_numpy(off_a).to(dev), off_a.size - 1, b, torch.from_numpy(off_b).to(dev), off_b.size - 1,
                           torch.from_numpy(pr).to(dev), max_points, tau, pp)
    _raise_on_status(status)
    out["sums"] = sums
    return out


def nearest_neighbors(a: torch.Tensor, a_offsets, b: torch.Tensor, b_offsets, pairs=None, return_index: bool = False, tau: float = 0.2):
    """Nearest neighbours between clouds, both ways, for a list of cloud pairs.

    ``a`` ``(totalA,4)``, ``b`` ``(totalB,4)`` float32 rows ``[x, y, z, .]`` on the GPU; cloud k of a set is the rows
    ``[offsets[k], offsets[k + 1])`` (what ``images_to_points`` returns).  ``pairs``: ``(P,2)`` integers ``[ia, ib]``; None pairs cloud k
    with cloud k.  -> a dict: ``d2_ab`` float32, for pair p the squared distance of every point of cloud ia to cloud ib at
    ``[start_ab[p], start_ab[p + 1])`` (``start_ab`` ``(P+1,)`` numpy int64); ``d2_ba``, ``start_ba`` the reverse; with ``return_index``
    ``idx_ab``, ``idx_ba`` int32, the neighbour's index inside its cloud (-1 against an empty cloud); ``sums`` as ``chamfer_sums``.
    A point with a non-finite coordinate raises ``ValueError``."""
    return _search(a, a_offsets, b, b_offsets, pairs, tau, True, return_index)


def chamfer_sums(a: torch.Tensor, a_offsets, b: torch.Tensor, b_offsets, pairs=None, tau: float = 0.2) -> torch.Tensor:
    """``(P,8)`` float64 on the device (``RAW_NAMES``): per pair the sum of ``d^2``, the sum of ``d`` and the number of points with
    ``d <= tau`` from a to b, the same from b to a, and the two counts.  Arguments as ``nearest_neighbors``."""
    return _search(a, a_offsets, b, b_offsets, pairs, tau, False, False)["sums"]


def chamfer_from_sums(raw: torch.Tensor) -> Dict[str, torch.Tensor]:
    """``(...,8)`` raw values (``RAW_NAMES``; a is the prediction) -> ``cd_sq``, ``cd``, ``precision``, ``recall``, ``fscore`` in float64,
    NaN where either cloud is empty.  Plain torch."""
    raw = torch.as_tensor(raw).double()
    if raw.dim() < 1 or raw.shape[-1] != len(RAW_NAMES):
        raise ValueError(f"expected (...,{len(RAW_NAMES)}) raw values {RAW_NAMES}, got {tuple(raw.shape)}")
    na, nb = raw[..., 6], raw[..., 7]
    ok = (na > 0) & (nb > 0)
    one, nan = torch.ones_like(na), torch.full_like(na, math.nan)
    da, db = torch.where(ok, na, one), torch.where(ok, nb, one)

    def val(x):
        return torch.where(ok, x, nan)

    # (against an empty cloud a sum is +inf: kept out of the arithmetic, not multiplied by 0)
    s = [torch.where(ok, raw[..., k], torch.zeros_like(na)) for k in range(6)]
    p, r = s[2] / da, s[5] / db
    pr = p + r
    f = torch.where(pr > 0, 2 * p * r / torch.where(pr > 0, pr, one), torch.zeros_like(pr))
    return {"cd_sq": val(s[0] / da + s[3] / db), "cd": val(0.5 * (s[1] / da + s[4] / db)), "precision": val(p), "recall": val(r), "fscore": val(f)}


def aggregate_chamfer(raw: torch.Tensor) -> dict:
    """(N,8) per-scan raw values -> ``{"scans", "empty", "micro", "macro"}`` over the scans whose two clouds both have points (``empty``
    counts the others): micro = the values of the summed sums and counts, macro = the mean of the per-scan values.  NaN if no scan is left."""
    raw = torch.as_tensor(raw).detach().cpu().double().reshape(-1, len(RAW_NAMES))
    ok = (raw[:, 6] > 0) & (raw[:, 7] > 0)
    used = raw[ok]
    per_scan = chamfer_from_sums(used)
    return {"scans": int(raw.shape[0]), "empty": int((~ok).sum().item()),
            "micro": {k: v.item() for k, v in chamfer_from_sums(used.sum(0)).items()},
            "macro": {k: (v.mean().item() if v.numel() else math.nan) for k, v in per_scan.items()}}


# ---- clouds ------------------------------------------------------------------------------------------------------------------------------
def clouds_of_samples(samples: torch.Tensor, lo: float, hi: float, region: Optional[torch.Tensor] = None):
    """``(B,5,H,W)`` planes [depth, x, y, z, reflectance] (``LiDARUtility.postprocess``) -> ``(points (total,4), offsets (B+1,))``: the
    returns (``lo < depth < hi``) of every image in image order (``images_to_points``).  ``region``: ``(B,1,H,W)``, non-zero = the pixel
    may be kept."""
    from .pointcloud import images_to_points

    if samples.dim() != 4 or samples.shape[1] != 5:
        raise ValueError(f"expected samples (B,5,H,W) [depth, x, y, z, reflectance], got {tuple(samples.shape)}")
    if region is not None:
        B, _, H, W = samples.shape
        if tuple(region.shape) != (B, 1, H, W):
            raise ValueError(f"region {tuple(region.shape)} must be (B,1,H,W) = {(B, 1, H, W)}")
        samples = samples.float().clone()
        samples[:, 0] = torch.where(region[:, 0].to(samples.device) != 0, samples[:, 0], torch.full_like(samples[:, 0], math.nan))  # NaN drops out
    return images_to_points(samples, layout="sample", order="image", keep_min=float(lo), keep_max=float(hi))


def subsample_indices(count: int, n: int, seed: int, index: int) -> torch.Tensor:
    """The rows of cloud ``index`` (``count`` points) that ``subsample`` keeps: all of them in order if ``count <= n``, else the first n of
    a permutation drawn from ``numpy.random.Generator(PCG64([seed, index]))`` (a seed sequence mixes both numbers) -- whatever else is in
    the batch."""
    count, n, seed, index = int(count), int(n), int(seed), int(index)
    if seed < 0 or index < 0:
        raise ValueError(f"seed and cloud index must be >= 0, got {seed}, {index}")
    if count <= n:
        return torch.arange(count)
    return torch.from_numpy(np.random.Generator(np.random.PCG64([seed, index])).permutation(count)[:n].astype(np.int64))


def subsample(points: torch.Tensor, offsets, n: int, seed: int, first_index: int = 0):
    """Ragged clouds -> ``(clouds (N,n,4), counts (N,) int64)`` on the points' device: per cloud n points drawn without replacement
    (``subsample_indices``; cloud k is drawn as cloud ``first_index + k``); a cloud with fewer than n points keeps all of them, zero-padded,
    and reports its count."""
    n = int(n)
    if n < 1:
        raise ValueError(f"n must be >= 1, got {n}")
    if points.dim() != 2 or points.shape[1] != 4:
        raise ValueError(f"expected points (total,4), got {tuple(points.shape)}")
    off = _host_offsets(offsets, points.shape[0], "offsets")
    N = off.size - 1
    rows = torch.zeros(N, n, dtype=torch.int64)
    counts = torch.zeros(N, dtype=torch.int64)
    for k in range(N):
        idx = subsample_indices(int(off[k + 1] - off[k]), n, seed, first_index + k)
        rows[k, :idx.numel()] = idx + int(off[k])
        counts[k] = idx.numel()
    valid = torch.arange(n)[None, :] < counts[:, None]
    out = torch.zeros(N, n, 4, dtype=torch.float32, device=points.device)
    if points.shape[0]:
        out = torch.where(valid[..., None].to(points.device), points.float()[rows.to(points.device)], out)
    return out, counts.to(points.device)


def _compact(clouds: torch.Tensor, counts: torch.Tensor, what: str):
    if clouds.dim() != 3 or clouds.shape[2] != 4:
        raise ValueError(f"{what}: expected (N,n,4) clouds, got {tuple(clouds.shape)}")
    N, n, _ = clouds.shape
    counts = torch.as_tensor(counts).to(clouds.device)
    if tuple(counts.shape) != (N,) or counts.dtype.is_floating_point:
        raise ValueError(f"{what}: counts must be ({N},) integers, got {tuple(counts.shape)} {counts.dtype}")
    host = counts.cpu().numpy().astype(np.int64)
    if N < 1 or (host < 0).any() or (host > n).any():
        raise ValueError(f"{what}: at least one cloud, and counts in [0, {n}]")
    keep = torch.arange(n, device=clouds.device)[None, :] < counts[:, None]
    return clouds.float()[keep].contiguous(), np.concatenate([[0], np.cumsum(host)]).astype(np.int64)


def pairwise_chamfer(A: torch.Tensor, countsA, B: torch.Tensor, countsB) -> torch.Tensor:
    """``(Na,Nb)`` float64 matrix of ``cd_sq`` between every cloud of ``A`` ``(Na,n,4)`` (the first ``countsA[i]`` rows of cloud i count) and
    every cloud of ``B``, on the device.  The same kernel as ``chamfer_sums``, over the pair list of all (i, j) generated in slabs, so
    that the pair list, the sums and the scratch of a call stay bounded; an entry equals the pair's own ``chamfer_sums`` bit for bit."""
    _lib.require_gpu(A, "A")
    if B.device != A.device:
        raise ValueError(f"A is on {A.device}, B on {B.device}")
    a, off_a = _compact(A, countsA, "A")
    b, off_b = _compact(B, countsB, "B")
    a, b = _points(a, "A"), _points(b, "B")
    dev, Na, Nb = A.device, off_a.size - 1, off_b.size - 1
    max_points = max(int(max(np.diff(off_a).max(), np.diff(off_b).max())), 1)
    chunks = (max_points + 1023) // 1024
    slab = max(1, min(SLAB_BYTES // (16 + 64 + 64 * chunks), ((1 << 31) - 1) // (2 * chunks)))
    oa, ob = torch.from_numpy(off_a).to(dev), torch.from_numpy(off_b).to(dev)
    out = torch.empty(Na * Nb, len(RAW_NAMES), dtype=torch.float64, device=dev)
    status = torch.zeros(2, dtype=torch.int64, device=dev)
    for s in range(0, Na * Nb, slab):
        k = torch.arange(s, min(s + slab, Na * Nb), dtype=torch.int64, device=dev)
        pairs = torch.stack([k // Nb, k % Nb], dim=1).contiguous()
        sums, st = _launch(a, oa, Na, b, ob, Nb, pairs, max_points, 0.0)
        out[s:s + slab] = sums
        status += st
    _raise_on_status(status)
    return chamfer_from_sums(out)["cd_sq"].reshape(Na, Nb)


# ---- voxel occupancy ---------------------------------------------------------------------------------------------------------------------
VOXEL_STATUS = ("nonfinite", "out_of_grid", "bad_groups", "table_full")
VOXEL_NAMES = ("iou", "precision", "recall", "f1")
VOXEL_MAX_SIZES = 8
VOXEL_MAX_MEMBERS = 63        # a voxel's membership mask has 64 bits, bit 63 is the target's
VOXEL_SLAB_BYTES = 1 << 30    # voxel_occupancy_counts: the hash tables of one call stay below this (or hold one group)


def _voxel_sizes(sizes) -> np.ndarray:
    try:
        s = np.asarray(sizes if isinstance(sizes, (list, tuple, np.ndarray)) else [sizes], dtype=np.float64).astype(np.float32)  # the size is its fp32 value
    except (TypeError, ValueError):
        raise ValueError(f"voxel sizes: expected 1 to {VOXEL_MAX_SIZES} numbers, got {sizes!r}") from None
    if s.ndim != 1 or not 1 <= s.size <= VOXEL_MAX_SIZES:
        raise ValueError(f"voxel sizes: expected 1 to {VOXEL_MAX_SIZES} numbers, got {sizes!r}")
    if not (np.isfinite(s) & (s > 0)).all():
        raise ValueError(f"voxel sizes must be finite and > 0 in float32, got {sizes!r}")
    return s


def _check_members(K: int) -> None:
    if not 1 <= K <= VOXEL_MAX_MEMBERS:
        raise ValueError(f"voxel occupancy takes 1 to {VOXEL_MAX_MEMBERS} members per group (a voxel's membership mask has 64 bits and one is the "
                         f"target's), got {K}")


def _voxel_capacity(max_group_points: int) -> int:
    cap = 2
    while cap < 2 * max_group_points:
        cap <<= 1
    return cap


def _voxel_launch(a, off_a, clouds_a, b, off_b, clouds_b, members_dev, targets_dev, sizes: np.ndarray, max_group_points: int):
    """One ``r2dm_voxel_occupancy`` call on device tensors -> ``(member (G,S,K,2), hist (G,S,2,K+1), status (4,))`` int64, nothing read back."""
    dev, (G, K), S = a.device, members_dev.shape, int(sizes.size)
    L = _lib.lib()
    nbytes = L.r2dm_voxel_occupancy_scratch_bytes(G, S, max_group_points)
    if nbytes == 0:
        raise ValueError(f"{G} groups of up to {max_group_points} points at {S} sizes: beyond the limits of r2dm_voxel_occupancy (65535 groups, "
                         "2^27 points per group, groups * sizes * capacity at most 2^36 slots)")
    scratch = torch.empty(nbytes // 16, 2, dtype=torch.int64, device=dev)
    member = torch.empty(G, S, K, 2, dtype=torch.int64, device=dev)
    hist = torch.empty(G, S, 2, K + 1, dtype=torch.int64, device=dev)
    status = torch.empty(len(VOXEL_STATUS), dtype=torch.int64, device=dev)
    host_sizes = (_lib.c_float * S)(*sizes.tolist())
    with torch.cuda.device(dev):
        _lib.check(L.r2dm_voxel_occupancy(_lib.ptr(a) or None, _lib.ptr(off_a), clouds_a, a.shape[0], _lib.ptr(b) or None, _lib.ptr(off_b), clouds_b,
                                          b.shape[0], _lib.ptr(members_dev), _lib.ptr(targets_dev), G, K, host_sizes, S, max_group_points,
                                          _lib.ptr(scratch), _lib.ptr(member), _lib.ptr(hist), _lib.ptr(status), _lib.stream_ptr(dev)))
    return member, hist, status


def _raise_on_voxel_status(status: torch.Tensor) -> None:
    counts = dict(zip(VOXEL_STATUS, (int(v) for v in status.cpu().tolist())))
    if counts["bad_groups"]:
        raise _lib.R2DMError(f"r2dm_voxel_occupancy: {counts['bad_groups']} groups with a cloud index or offsets that do not check out")
    if counts["table_full"]:
        raise _lib.R2DMError(f"r2dm_voxel_occupancy: {counts['table_full']} inserts found their hash table full (a defect: the load factor is at most 0.5)")
    if counts["nonfinite"]:
        raise ValueError(f"voxel occupancy: {counts['nonfinite']} points with a non-finite coordinate (counted once per group they are part of)")
    if counts["out_of_grid"]:
        raise ValueError(f"voxel occupancy: {counts['out_of_grid']} points outside the grid of 2^21 cells per axis, floor(x / size) in [-2^20, 2^20) "
                         "(counted once per group and size)")


def _group_indices(members, targets):
    mem = members.detach().cpu().numpy() if isinstance(members, torch.Tensor) else np.asarray(members)
    tgt = targets.detach().cpu().numpy() if isinstance(targets, torch.Tensor) else np.asarray(targets)
    if mem.ndim != 2 or mem.shape[1] < 1 or (mem.size and mem.dtype.kind not in "iu"):
        raise ValueError(f"members: expected (G,K) integers, K >= 1 cloud indices into a per group, got shape {mem.shape} {mem.dtype}")
    if tgt.ndim != 1 or tgt.shape[0] != mem.shape[0] or (tgt.size and tgt.dtype.kind not in "iu"):
        raise ValueError(f"targets: expected ({mem.shape[0]},) integers, one cloud index into b per group, got shape {tgt.shape} {tgt.dtype}")
    _check_members(mem.shape[1])
    return np.ascontiguousarray(mem.astype(np.int64)), np.ascontiguousarray(tgt.astype(np.int64))


def voxel_occupancy_counts(a: torch.Tensor, a_offsets, b: torch.Tensor, b_offsets, members, targets, sizes, _raise: bool = True) -> dict:
    """The voxels that groups of clouds occupy, counted (``r2dm_voxel_occupancy``, ``r2dm_amd/csrc/voxel.hip``).

    Clouds as for ``nearest_neighbors``.  Group g is the target cloud ``targets[g]`` of ``b`` and the K member clouds ``members[g]`` of ``a``
    (``members`` (G,K), ``targets`` (G,) integers; 1 <= K <= 63; a cloud may be part of any number of groups).  The voxel of a point at size s
    (metres, rounded to float32) is ``floor(x / s), floor(y / s), floor(z / s)`` with IEEE float32 divisions; ``sizes``: 1 to 8 of them.
    -> ``{"member": (G,S,K,2), "hist": (G,S,2,K+1)}`` int64 on the device: per group and size ``member[k] = (|V(M_k)|, |V(M_k) n V(T)|)`` and
    ``hist[o][c]`` = the number of voxels of the union that are in the target (o = 1) or not (o = 0) and in c members.  Integers summed by
    integer atomics: the same bits for any order of the points, and the member rows permute with the members.

    The groups go through the kernel in slabs, so that the hash tables of one call (16 bytes per slot, the power of two >= 2 * the points of
    the slab's largest group slots per group and size) stay below ``VOXEL_SLAB_BYTES`` or hold a single group.  A point with a non-finite
    coordinate or outside the grid (``floor(x / s)`` in [-2^20, 2^20)) raises ``ValueError``, a cloud index outside its set ``R2DMError``.
    There is no CPU fallback."""
    a, b = _points(a, "a"), _points(b, "b")
    if b.device != a.device:
        raise ValueError(f"a is on {a.device}, b on {b.device}")
    off_a, off_b = _host_offsets(a_offsets, a.shape[0], "a_offsets"), _host_offsets(b_offsets, b.shape[0], "b_offsets")
    mem, tgt = _group_indices(members, targets)
    sizes = _voxel_sizes(sizes)
    dev, (G, K), S = a.device, mem.shape, int(sizes.size)
    out = {"member": torch.zeros(G, S, K, 2, dtype=torch.int64, device=dev), "hist": torch.zeros(G, S, 2, K + 1, dtype=torch.int64, device=dev)}
    status = torch.zeros(len(VOXEL_STATUS), dtype=torch.int64, device=dev)
    if G:
        # points per group, to size the tables (an index out of range counts nothing here: the device refuses the group)
        na, nb = np.diff(off_a), np.diff(off_b)
        count = lambda n, idx: np.where((idx >= 0) & (idx < n.size), n[np.clip(idx, 0, n.size - 1)], 0)
        points = count(na, mem).sum(axis=1) + count(nb, tgt)
        oa, ob = torch.from_numpy(off_a).to(dev), torch.from_numpy(off_b).to(dev)
        mem_dev, tgt_dev = torch.from_numpy(mem).to(dev), torch.from_numpy(tgt).to(dev)
        g0 = 0
        while g0 < G:
            g1, most = g0 + 1, max(int(points[g0]), 1)
            while g1 < G and g1 - g0 < 65535:  # grow the slab while its tables fit
                grown = max(most, int(points[g1]))
                if (g1 + 1 - g0) * S * _voxel_capacity(grown) * 16 > VOXEL_SLAB_BYTES:
                    break
                g1, most = g1 + 1, grown
            m, h, st = _voxel_launch(a, oa, off_a.size - 1, b, ob, off_b.size - 1, mem_dev[g0:g1].contiguous(), tgt_dev[g0:g1].contiguous(), sizes, most)
            out["member"][g0:g1], out["hist"][g0:g1] = m, h
            status += st
            g0 = g1
    if _raise:
        _raise_on_voxel_status(status)
        return out
    return {**out, "status": status}


def _ratio64(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
    """num / den in float64, NaN where den == 0"""
    num, den = num.double(), den.double()
    return torch.where(den != 0, num / torch.where(den != 0, den, torch.ones_like(den)), torch.full_like(den, math.nan))


def _set_scores(inter: torch.Tensor, pred: torch.Tensor, target: torch.Tensor) -> Dict[str, torch.Tensor]:
    """``VOXEL_NAMES`` of a predicted set against a target set from |P n T|, |P|, |T|: IoU = |P n T| / |P u T|, precision = |P n T| / |P|,
    recall = |P n T| / |T|, F1 = 2 |P n T| / (|P| + |T|) (the harmonic mean of the two wherever both are defined); NaN for a denominator of 0."""
    return {"iou": _ratio64(inter, pred + target - inter), "precision": _ratio64(inter, pred), "recall": _ratio64(inter, target),
            "f1": _ratio64(2 * inter, pred + target)}


def _integers(t, what: str) -> torch.Tensor:
    t = torch.as_tensor(t)
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"{what}: expected integer counts, got {t.dtype}")
    return t.long()


def voxel_from_counts(counts) -> Dict[str, torch.Tensor]:
    """``(...,3)`` integers ``[intersection, voxels_a, voxels_b]`` (a is the prediction) -> ``iou``, ``precision``, ``recall``, ``f1`` in float64,
    NaN where the denominator is 0 (an empty cloud).  Plain torch."""
    counts = _integers(counts, "counts")
    if counts.dim() < 1 or counts.shape[-1] != 3:
        raise ValueError(f"expected (...,3) counts [intersection, voxels_a, voxels_b], got {tuple(counts.shape)}")
    return _set_scores(counts[..., 0], counts[..., 1], counts[..., 2])


def voxel_iou(a: torch.Tensor, a_offsets, b: torch.Tensor, b_offsets, pairs=None, sizes=(0.1,)) -> dict:
    """Voxel occupancy IoU of cloud pairs: the K = 1 case of ``voxel_occupancy_counts``.  Clouds and ``pairs`` as for ``nearest_neighbors`` (a is
    the prediction, b the target), ``sizes`` the voxel sizes in metres.  -> a dict of device tensors: ``counts`` (P,S,3) int64
    ``[intersection, voxels_a, voxels_b]`` and ``iou``, ``precision``, ``recall``, ``f1`` (P,S) float64 (``voxel_from_counts``).  An empty cloud
    has no voxels: its counts are 0 and the values whose denominator is 0 are NaN."""
    off_a, off_b = _host_offsets(a_offsets, a.shape[0], "a_offsets"), _host_offsets(b_offsets, b.shape[0], "b_offsets")
    pr = _pairs(pairs, off_a.size - 1, off_b.size - 1)
    res = voxel_occupancy_counts(a, off_a, b, off_b, pr[:, :1], pr[:, 1], sizes)
    hist = res["hist"]                                            # (P,S,2,2)
    inter = hist[..., 1, 1]
    counts = torch.stack([inter, inter + hist[..., 0, 1], inter + hist[..., 1, 0]], dim=-1)
    return {"counts": counts, **voxel_from_counts(counts)}


def occupancy_from_counts(member, hist) -> Dict[str, torch.Tensor]:
    """The occupancy scores of an ensemble from the integers of ``voxel_occupancy_counts``: ``member`` (...,K,2), ``hist`` (...,2,K+1).  In
    float64, NaN for a denominator of 0, plain torch:

    - ``union`` = |U|, ``voxels_target`` = |V(T)| (int64);
    - ``member_iou`` / ``member_precision`` / ``member_recall`` / ``member_f1`` (...,K): every member's own voxel set against the target's;
    - ``any_*``: the voxels at least one member occupies (c >= 1) against the target's;
    - ``consensus_*``: the voxels at least half of the members occupy (2 c >= K);
    - ``brier`` = the mean over U of (c / K - o)^2 = sum_c (hist[0][c] c^2 + hist[1][c] (K - c)^2) / (K^2 |U|);
    - ``reliability`` (...,K+1) = hist[1][c] / (hist[0][c] + hist[1][c]): of the voxels c members occupy, the fraction the target occupies
      (c / K for a calibrated ensemble)."""
    member, hist = _integers(member, "member"), _integers(hist, "hist")
    if hist.dim() < 2 or hist.shape[-2] != 2 or hist.shape[-1] < 2:
        raise ValueError(f"expected hist (...,2,K+1), got {tuple(hist.shape)}")
    K = hist.shape[-1] - 1
    if member.dim() < 2 or tuple(member.shape[-2:]) != (K, 2) or member.shape[:-2] != hist.shape[:-2]:
        raise ValueError(f"expected member (...,{K},2) next to hist {tuple(hist.shape)}, got {tuple(member.shape)}")
    c = torch.arange(K + 1, device=hist.device)
    target = hist[..., 1, :].sum(-1)
    out = {"union": hist.sum((-2, -1)), "voxels_target": target}
    for name, v in _set_scores(member[..., 1], member[..., 0], target[..., None]).items():
        out[f"member_{name}"] = v
    for head, keep in (("any", c >= 1), ("consensus", 2 * c >= K)):
        sel = hist * keep.long()
        for name, v in _set_scores(sel[..., 1, :].sum(-1), sel.sum((-2, -1)), target).items():
            out[f"{head}_{name}"] = v
    out["brier"] = _ratio64((hist[..., 0, :] * c * c + hist[..., 1, :] * (K - c) * (K - c)).sum(-1), K * K * out["union"])
    out["reliability"] = _ratio64(hist[..., 1, :], hist[..., 0, :] + hist[..., 1, :])
    return out


def _mean_defined(v: torch.Tensor) -> torch.Tensor:
    """the mean over dim 0 of the values that are not NaN; NaN where there is none"""
    ok = ~v.isnan()
    return _ratio64(torch.where(ok, v, torch.zeros_like(v)).sum(0), ok.sum(0))


def aggregate_voxel(counts, sizes) -> dict:
    """(N,S,3) per-scan counts -> ``{"scans", "empty", "sizes", "micro", "macro"}`` over the scans whose two clouds both have points (``empty``
    counts the others): micro = the values of the summed counts, macro = the mean of the per-scan values; each a list over the sizes, NaN if
    no scan is left."""
    counts = _integers(counts, "counts").detach().cpu()
    sizes = [float(s) for s in _voxel_sizes(sizes)]
    counts = counts.reshape(-1, len(sizes), 3)
    ok = ((counts[..., 1] > 0) & (counts[..., 2] > 0)).all(dim=1) if counts.shape[0] else torch.zeros(0, dtype=torch.bool)
    used = counts[ok]
    return {"scans": int(counts.shape[0]), "empty": int((~ok).sum().item()), "sizes": sizes,
            "micro": {k: v.tolist() for k, v in voxel_from_counts(used.sum(0)).items()},
            "macro": {k: _mean_defined(v).tolist() for k, v in voxel_from_counts(used).items()}}


def aggregate_occupancy(member, hist, sizes) -> dict:
    """(N,S,K,2), (N,S,2,K+1) per-scan integers -> ``{"scans", "empty", "members", "sizes", "hist", "micro", "macro"}`` over the scans whose
    target has voxels (``empty`` counts the others): ``hist`` (S,2,K+1) the summed histogram, micro = ``occupancy_from_counts`` of the summed
    integers, macro = the mean of the per-scan values that are defined; lists over the sizes (and the members, and c)."""
    member, hist = _integers(member, "member").detach().cpu(), _integers(hist, "hist").detach().cpu()
    sizes = [float(s) for s in _voxel_sizes(sizes)]
    K = hist.shape[-1] - 1
    member, hist = member.reshape(-1, len(sizes), K, 2), hist.reshape(-1, len(sizes), 2, K + 1)
    ok = (hist[:, :, 1].sum(-1) > 0).all(dim=1) if hist.shape[0] else torch.zeros(0, dtype=torch.bool)
    um, uh = member[ok], hist[ok]
    skip = ("union", "voxels_target")
    return {"scans": int(hist.shape[0]), "empty": int((~ok).sum().item()), "members": K, "sizes": sizes, "hist": uh.sum(0).tolist(),
            "micro": {k: v.tolist() for k, v in occupancy_from_counts(um.sum(0), uh.sum(0)).items() if k not in skip},
            "macro": {k: _mean_defined(v).tolist() for k, v in occupancy_from_counts(um, uh).items() if k not in skip}}


# ---- earth mover's distance --------------------------------------------------------------------------------------------------------------
def _emd_knobs(eps, max_rounds):
    eps, max_rounds = float(eps), int(max_rounds)
    if not (math.isfinite(eps) and eps > 0):
        raise ValueError(f"eps must be a finite distance > 0 (metres per point), got {eps}")
    if max_rounds < 1:
        raise ValueError(f"max_rounds must be >= 1, got {max_rounds}")
    return eps, max_rounds


def _emd_launch(a, off_a, clouds_a, b, off_b, clouds_b, pairs_dev, max_points, eps, max_rounds, assignment=False, prices=False):
    """One ``r2dm_emd_pairs`` call on device tensors -> dict of ``out`` (P,4), ``status`` (5,), ``code`` (P,) and the optional
    ``assignment`` / ``prices`` (P, max_points); nothing read back, nothing raised for what the device refuses."""
    dev, P = a.device, pairs_dev.shape[0]
    L = _lib.lib()
    nbytes = L.r2dm_emd_pairs_scratch_bytes(P, max_points)
    if nbytes == 0:
        raise ValueError(f"{P} pairs of clouds of up to {max_points} points: beyond the limits of r2dm_emd_pairs (at least one pair, clouds of 1 to "
                         f"{emd_max_points()} points)")
    res = {"out": torch.empty(P, 4, dtype=torch.float64, device=dev), "status": torch.empty(len(EMD_STATUS), dtype=torch.int64, device=dev),
           "code": torch.empty(nbytes // 8, dtype=torch.int64, device=dev)}
    if assignment:
        res["assignment"] = torch.empty(P, max_points, dtype=torch.int32, device=dev)
    if prices:
        res["prices"] = torch.empty(P, max_points, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.r2dm_emd_pairs(_lib.ptr(a) or None, _lib.ptr(off_a), clouds_a, a.shape[0], _lib.ptr(b) or None, _lib.ptr(off_b), clouds_b, b.shape[0],
                                    _lib.ptr(pairs_dev), P, max_points, eps, max_rounds, _lib.ptr(res.get("assignment")), _lib.ptr(res.get("prices")),
                                    _lib.ptr(res["out"]), _lib.ptr(res["code"]), _lib.ptr(res["status"]), _lib.stream_ptr(dev)))
    return res


EMD_STATUS = ("bad_pair", "unequal_counts", "non_finite", "eps_floor", "round_cap")  # status[k] counts the pairs that ended with code k + 1


def emd_max_points() -> int:
    """The largest cloud ``r2dm_emd_pairs`` takes (the auction of a pair lives in one workgroup's LDS)."""
    return int(_lib.lib().r2dm_emd_max_points())


def _raise_on_emd_status(status: torch.Tensor, code: torch.Tensor, eps: float, first: int, allow_unconverged: bool) -> None:
    """One read of the counters; the per-pair codes are read only to name the pairs of an error."""
    counts = dict(zip(EMD_STATUS, (int(v) for v in status.cpu().tolist())))
    if not any(counts.values()):
        return

    def which(k):
        at = (torch.nonzero(code == k + 1).flatten() + first).cpu().tolist()
        return f"{at[:8]}{' ...' if len(at) > 8 else ''}"

    if counts["bad_pair"]:
        raise ValueError(f"earth mover's distance: {counts['bad_pair']} pairs {which(0)} with an index or offsets that do not check out, no points, "
                         f"or more than {emd_max_points()} points")
    if counts["unequal_counts"]:
        raise ValueError(f"earth mover's distance: {counts['unequal_counts']} pairs {which(1)} whose two clouds differ in size (the distance is "
                         "defined for equal counts)")
    if counts["non_finite"]:
        raise ValueError(f"earth mover's distance: {counts['non_finite']} pairs {which(2)} with a non-finite coordinate")
    if counts["eps_floor"]:
        raise ValueError(f"earth mover's distance: eps = {eps} is below 2^-18 of the bounding-box diagonal of {counts['eps_floor']} pairs {which(3)}: "
                         "a bid increment could vanish in fp32")
    if counts["round_cap"] and not allow_unconverged:
        raise _lib.R2DMError(f"earth mover's distance: {counts['round_cap']} pairs {which(4)} did not converge within max_rounds "
                             "(allow_unconverged=True returns NaN for them)")


def emd_pairs(a: torch.Tensor, a_offsets, b: torch.Tensor, b_offsets, pairs=None, eps: float = 0.01, max_rounds: int = 1 << 20,
              return_assignment: bool = False, return_prices: bool = False, allow_unconverged: bool = False) -> dict:
    """Earth mover's distance of a list of cloud pairs: ``EMD(A, B) = (1/n) min_sigma sum_i |a_i - b_sigma(i)|`` in metres, for two clouds of
    the same number n >= 1 of points (at most ``emd_max_points()``).  Clouds and ``pairs`` as ``nearest_neighbors``.

    One HIP kernel (``r2dm_emd_pairs``, ``r2dm_amd/csrc/emd.hip``): a forward auction with epsilon-scaling, which does not promise the
    minimum.  -> a dict of device tensors, ``(P,)`` each: ``emd`` float64, the true cost of the permutation found; ``lower`` float64, a
    lower bound of the minimum certified by weak duality from the final prices (``lower <= EMD <= emd``; in exact arithmetic
    ``emd - lower <= eps``); ``rounds`` int64; ``converged`` bool; with ``return_assignment`` ``assignment`` ``(P, max n)`` int32
    (``sigma(i)``, -1 beyond a pair's n), with ``return_prices`` ``prices`` ``(P, max n)`` float32 (NaN beyond n).

    ``eps`` is the accuracy knob, metres per point; below ``2^-18`` of a pair's bounding-box diagonal it is refused.  Raises ``ValueError``
    for bad pairs, unequal counts, non-finite points and such an eps, and ``R2DMError`` naming the pairs that did not converge within
    ``max_rounds`` bidding rounds unless ``allow_unconverged`` (their values are NaN)."""
    a, b = _points(a, "a"), _points(b, "b")
    if b.device != a.device:
        raise ValueError(f"a is on {a.device}, b on {b.device}")
    off_a, off_b = _host_offsets(a_offsets, a.shape[0], "a_offsets"), _host_offsets(b_offsets, b.shape[0], "b_offsets")
    pr = _pairs(pairs, off_a.size - 1, off_b.size - 1)
    eps, max_rounds = _emd_knobs(eps, max_rounds)
    dev, P = a.device, pr.shape[0]
    na, nb = np.diff(off_a)[pr[:, 0]], np.diff(off_b)[pr[:, 1]]
    if (na != nb).any():
        at = np.flatnonzero(na != nb)
        raise ValueError(f"earth mover's distance: {at.size} pairs {at[:8].tolist()} whose two clouds differ in size ({int(na[at[0]])} and "
                         f"{int(nb[at[0]])} points): the distance is defined for equal counts")
    if P and (na.min() < 1 or na.max() > emd_max_points()):
        raise ValueError(f"earth mover's distance: clouds of 1 to {emd_max_points()} points, got {int(na.min())} to {int(na.max())}")
    width = int(na.max()) if P else 0
    out = {"emd": torch.empty(P, dtype=torch.float64, device=dev), "lower": torch.empty(P, dtype=torch.float64, device=dev),
           "rounds": torch.empty(P, dtype=torch.int64, device=dev), "converged": torch.empty(P, dtype=torch.bool, device=dev)}
    if return_assignment:
        out["assignment"] = torch.empty(P, width, dtype=torch.int32, device=dev)
    if return_prices:
        out["prices"] = torch.empty(P, width, dtype=torch.float32, device=dev)
    if P == 0:
        return out
    res = _emd_launch(a, torch.from_numpy(off_a).to(dev), off_a.size - 1, b, torch.from_numpy(off_b).to(dev), off_b.size - 1,
                      torch.from_numpy(pr).to(dev), width, eps, max_rounds, return_assignment, return_prices)
    _raise_on_emd_status(res["status"], res["code"], eps, 0, allow_unconverged)
    out.update(emd=res["out"][:, 0].contiguous(), lower=res["out"][:, 1].contiguous(), rounds=res["out"][:, 2].long(), converged=res["out"][:, 3] != 0)
    for k in ("assignment", "prices"):
        if k in res:
            out[k] = res[k]
    return out


EMD_SLAB_PAIRS = 1 << 16      # pairwise_emd: pairs per call (32 bytes of results, 16 of pair list and 8 of codes each)


def pairwise_emd(A: torch.Tensor, countsA, B: Optional[torch.Tensor] = None, countsB=None, eps: float = 0.01, max_rounds: int = 1 << 20):
    """``(D, gap)``: ``(Na,Nb)`` float64 matrices on the device of ``emd`` and of the certified ``emd - lower`` between every cloud of ``A``
    ``(Na,n,4)`` and every cloud of ``B``; the kernel of ``emd_pairs`` over the pair list of all (i, j) in slabs, an entry equal to the
    pair's own ``emd_pairs`` bit for bit.  With ``B=None`` the matrix of ``A`` against itself: only ``i < j`` is solved and mirrored, the
    diagonal is 0 (the auction's answers for (A, B) and (B, A) may differ inside the gap; this matrix is symmetric by construction).
    Every cloud must hold the same number of points (``ValueError``)."""
    _lib.require_gpu(A, "A")
    same = B is None
    if same:
        if countsB is not None:
            raise ValueError("countsB without B")
        B, countsB = A, countsA
    elif countsB is None:
        raise ValueError("B needs countsB")
    if B.device != A.device:
        raise ValueError(f"A is on {A.device}, B on {B.device}")
    eps, max_rounds = _emd_knobs(eps, max_rounds)
    a, off_a = _compact(A, countsA, "A")
    b, off_b = (a, off_a) if same else _compact(B, countsB, "B")
    na = np.concatenate([np.diff(off_a), np.diff(off_b)])
    if (na != na[0]).any() or na[0] < 1:
        raise ValueError(f"earth mover's distance: every cloud must hold the same number (>= 1) of points, got counts from {int(na.min())} to "
                         f"{int(na.max())}")
    n = int(na[0])
    if n > emd_max_points():
        raise ValueError(f"earth mover's distance: clouds of up to {emd_max_points()} points, got {n}")
    a = _points(a, "A")
    b = a if same else _points(b, "B")
    dev, Na, Nb = A.device, off_a.size - 1, off_b.size - 1
    oa = torch.from_numpy(off_a).to(dev)
    ob = oa if same else torch.from_numpy(off_b).to(dev)
    if same:
        iu = torch.triu_indices(Na, Na, offset=1, device=dev)
        every = torch.stack([iu[0], iu[1]], dim=1).contiguous()
    else:
        k = torch.arange(Na * Nb, dtype=torch.int64, device=dev)
        every = torch.stack([k // Nb, k % Nb], dim=1).contiguous()
    total = every.shape[0]
    out = torch.empty(total, 4, dtype=torch.float64, device=dev)
    for s in range(0, total, EMD_SLAB_PAIRS):
        res = _emd_launch(a, oa, Na, b, ob, Nb, every[s:s + EMD_SLAB_PAIRS].contiguous(), n, eps, max_rounds)
        _raise_on_emd_status(res["status"], res["code"], eps, s, False)  # (a slab may run for minutes: an error ends the matrix here)
        out[s:s + EMD_SLAB_PAIRS] = res["out"]
    D, gap = torch.zeros(Na, Nb, dtype=torch.float64, device=dev), torch.zeros(Na, Nb, dtype=torch.float64, device=dev)
    D[every[:, 0], every[:, 1]] = out[:, 0]
    gap[every[:, 0], every[:, 1]] = out[:, 0] - out[:, 1]
    if same:
        D, gap = D + D.t(), gap + gap.t()  # (x + 0: exact)
    return D, gap


# ---- set metrics (plain torch) -----------------------------------------------------------------------------------------------------------
def _matrix(D, what: str) -> torch.Tensor:
    D = torch.as_tensor(D).double()
    if D.dim() != 2 or D.shape[0] < 1 or D.shape[1] < 1:
        raise ValueError(f"{what}: expected a non-empty distance matrix, got {tuple(D.shape)}")
    if D.isnan().any():
        raise ValueError(f"{what}: a NaN distance (an empty cloud): the set metrics are defined for clouds with points")
    return D


def _argmin_lowest(D: torch.Tensor) -> torch.Tensor:
    """per row the LOWEST column index that attains the row's minimum"""
    cols = torch.arange(D.shape[1], device=D.device).expand_as(D)
    return torch.where(D == D.min(dim=1, keepdim=True).values, cols, torch.full_like(cols, D.shape[1])).min(dim=1).values


def coverage(D) -> float:
    """``D`` (generated, real) -> the fraction of real clouds that are the nearest real cloud of some generated one."""
    D = _matrix(D, "coverage")
    return _argmin_lowest(D).unique().numel() / D.shape[1]


def minimum_matching_distance(D) -> float:
    """``D`` (generated, real) -> the mean over the real clouds of the distance to their nearest generated cloud."""
    nearest = _matrix(D, "minimum_matching_distance").min(dim=0).values
    return math.fsum(nearest.tolist()) / nearest.numel()  # (a correctly rounded sum: the value does not depend on an order of summation)


def one_nn_accuracy(D_gg, D_gr, D_rr) -> float:
    """Leave-one-out 1-nearest-neighbour accuracy over S = G u R from the three blocks of its distance matrix."""
    D_gg, D_gr, D_rr = _matrix(D_gg, "D_gg"), _matrix(D_gr, "D_gr"), _matrix(D_rr, "D_rr")
    G, R = D_gr.shape
    if tuple(D_gg.shape) != (G, G) or tuple(D_rr.shape) != (R, R):
        raise ValueError(f"D_gg {tuple(D_gg.shape)}, D_gr {tuple(D_gr.shape)}, D_rr {tuple(D_rr.shape)} must be (G,G), (G,R), (R,R)")
    D_gg, D_rr = D_gg.to(D_gr.device), D_rr.to(D_gr.device)
    M = torch.cat([torch.cat([D_gg, D_gr], dim=1), torch.cat([D_gr.t(), D_rr], dim=1)], dim=0).clone()
    if G + R < 2:
        raise ValueError("1-NNA needs at least two clouds")
    M.fill_diagonal_(math.inf)
    nearest = _argmin_lowest(M)
    is_g = torch.arange(G + R, device=M.device) < G
    return ((nearest < G) == is_g).double().mean().item()


def set_metrics(D_gg, D_gr, D_rr) -> Dict[str, float]:
    """``{"cov", "mmd", "1-nna"}`` from the distance matrices generated x generated, generated x real, real x real -- of any distance between
    clouds: ``cd_sq`` (``pairwise_chamfer``) or the earth mover's distance (``pairwise_emd``)."""
    return {"cov": coverage(D_gr), "mmd": minimum_matching_distance(D_gr), "1-nna": one_nn_accuracy(D_gg, D_gr, D_rr)}
