"""Plain numpy specification of the ensemble coherence sums (``coherence_dist_kernel`` / ``coherence_vario_kernel`` in
r2dm_amd/csrc/completion.hip) and of the scores derived from them, written from the definitions and sharing no code with the library.
Everything is float64 on widened float32 values.  ``dist`` is the double loop over the K + 1 rows (the K members, then the target) of the
squared differences summed over E; ``vario`` the loops over the offsets and, inside, over the members in member order; the derived scores
are the double loops over members and over offsets of the definitions, nothing sorted."""
import numpy as np

CHANNELS = ("depth", "reflectance")


def values(samples, target, lo, hi):
    """samples (B,K,5,H,W), target (B,5,H,W) float32 -> v (B,2,K+1,H,W) float64: per channel the K members and, as row K, the target.  A
    member's depth is d if lo < d < hi, else 0; a member's reflectance as stored with NaN read as 0; the target's values as stored."""
    samples, target = np.asarray(samples, np.float32), np.asarray(target, np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    B, K = samples.shape[:2]
    v = np.zeros((B, 2, K + 1) + samples.shape[3:], np.float64)
    with np.errstate(invalid="ignore"):
        d, rho = samples[:, :, 0], samples[:, :, 4]
        v[:, 0, :K] = np.where((lo < d) & (d < hi), d, np.float32(0))
        v[:, 1, :K] = np.where(np.isnan(rho), np.float32(0), rho)
    v[:, 0, K], v[:, 1, K] = target[:, 0], target[:, 4]
    return v


def evaluated(target, known, lo, hi):
    """-> U, E (B,H,W) bool: the unknown pixels, and those of them where the target returns"""
    target, known = np.asarray(target, np.float32), np.asarray(known, np.float32)
    with np.errstate(invalid="ignore"):
        U = known[:, 0] == 0
        G = (np.float32(lo) < target[:, 0]) & (target[:, 0] < np.float32(hi))
    return U, U & G


def scores(samples, target, known, lo, hi, offsets):
    """-> counts (B,2), dist (B,2,K+1,K+1), vario (B,2,O,4) float64"""
    v = values(samples, target, lo, hi)
    U, E = evaluated(target, known, lo, hi)
    B, _, R, H, W = v.shape
    K = R - 1
    offsets = [(int(dh), int(dw)) for dh, dw in offsets]
    counts = np.stack([U.reshape(B, -1).sum(1), E.reshape(B, -1).sum(1)], 1).astype(np.float64)
    dist = np.zeros((B, 2, R, R), np.float64)
    vario = np.zeros((B, 2, len(offsets), 4), np.float64)
    with np.errstate(invalid="ignore"):
        for b in range(B):
            for c in range(2):
                x = v[b, c][:, E[b]]  # (K+1, |E|)
                for i in range(R):
                    for j in range(R):
                        d = x[i] - x[j]
                        dist[b, c, i, j] = (d * d).sum()
                for o, (dh, dw) in enumerate(offsets):
                    assert (dh, dw) != (0, 0) and abs(dh) < H and abs(dw) < W
                    hs = np.arange(H)[(np.arange(H) + dh >= 0) & (np.arange(H) + dh < H)]  # azimuth wraps, elevation does not
                    p = (hs[:, None], np.arange(W)[None, :])
                    q = (hs[:, None] + dh, (np.arange(W)[None, :] + dw) % W)
                    pair = E[b][p] & E[b][q]
                    a = np.sqrt(np.abs(v[b, c, K][p] - v[b, c, K][q]))[pair]
                    s = np.zeros(a.shape, np.float64)
                    for k in range(K):
                        s = s + np.sqrt(np.abs(v[b, c, k][p] - v[b, c, k][q]))[pair]
                    m = s / float(K)
                    vario[b, c, o] = [pair.sum(), ((a - m) * (a - m)).sum(), (a * a).sum(), (m * m).sum()]
    return counts, dist, vario


def derived(counts, dist, vario):
    """(...,2), (...,2,K+1,K+1), (...,2,O,4) -> dict of the derived values, NaN where a denominator is 0; the sums as the double loops"""
    counts, dist, vario = (np.asarray(a, np.float64) for a in (counts, dist, vario))
    K = dist.shape[-1] - 1
    lead = counts.shape[:-1]
    E = counts[..., 1]

    def ratio(num, den):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.nan)

    out = {}
    for c, name in enumerate(CHANNELS):
        D = np.sqrt(dist[..., c, :, :])
        skill, pairs, between, to_target = np.zeros(lead), np.zeros(lead), np.zeros(lead), np.zeros(lead)
        member = np.zeros(lead + (K,))
        for k in range(K):
            skill = skill + D[..., k, K]
            member[..., k] = np.sqrt(ratio(dist[..., c, k, K], E))
            to_target = to_target + member[..., k]
            for l in range(K):
                if l != k:
                    pairs = pairs + D[..., k, l]
                if l > k:
                    between = between + np.sqrt(ratio(dist[..., c, k, l], E))
        nan = np.full(lead, np.nan)
        out["energy_" + name] = ratio(skill / K - pairs / (2 * K * K), np.sqrt(E))
        out["energy_fair_" + name] = ratio(skill / K - pairs / (2 * K * (K - 1)), np.sqrt(E)) if K > 1 else nan
        out["member_rmse_" + name] = member
        out["best_rmse_" + name] = member.min(-1)
        out["diversity_" + name] = between / (K * (K - 1) / 2) if K > 1 else nan
        out["spread_skill_energy_" + name] = ratio(out["diversity_" + name], to_target / K) if K > 1 else nan
        v = vario[..., c, :, :]
        out["variogram_" + name] = ratio(v[..., 1], v[..., 0])
        out["variogram_total_" + name] = ratio(v[..., 1].sum(-1), v[..., 0].sum(-1))
        out["variogram_rel_" + name] = ratio(v[..., 1].sum(-1), v[..., 2].sum(-1))
    return out


def shuffle_inputs(seed, scans=8, H=8, W=32, K=16):
    """The input that shows what the per-pixel scores cannot see.  Per scan a smooth field; the target and each of the K members are the
    field plus one N(0, 1) offset of their own plus N(0, 0.05^2) noise per pixel (the truth is exchangeable with the members); rows 0 and 4
    are known.  -> (coherent, shuffled, target, known): ``shuffled`` holds at every pixel the same K values (both channels together) as
    ``coherent``, permuted independently per pixel -- every per-pixel score keeps its value, every draw turns into salt and pepper."""
    g = np.random.Generator(np.random.PCG64(seed))
    h, w = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    coherent = np.zeros((scans, K, 5, H, W), np.float32)
    target = np.zeros((scans, 5, H, W), np.float32)
    for b in range(scans):
        phase = g.uniform(0, 2 * np.pi, 2)
        field = 20.0 + 6.0 * np.sin(2 * np.pi * w / W + phase[0]) + 3.0 * np.cos(np.pi * h / H + phase[1])
        refl = 0.5 + 0.2 * np.cos(2 * np.pi * w / W + phase[1]) * np.sin(np.pi * (h + 0.5) / H)
        draw = lambda: (field + g.normal() + g.normal(0, 0.05, (H, W)), refl + 0.1 * g.normal() + g.normal(0, 0.005, (H, W)))
        target[b, 0], target[b, 4] = draw()
        for k in range(K):
            coherent[b, k, 0], coherent[b, k, 4] = draw()
    order = np.argsort(g.uniform(size=(scans, K, 1, H, W)), axis=1)  # an independent permutation of the members at every pixel
    shuffled = np.take_along_axis(coherent, np.broadcast_to(order, coherent.shape), axis=1)
    known = np.zeros((scans, 1, H, W), np.float32)
    known[:, :, ::4] = 1
    return coherent, shuffled, target, known
