"""Plain numpy specification of the ensemble scores (``ensemble_score_kernel`` in r2dm_amd/csrc/completion.hip), written from the
definitions and sharing no code with the library.  Everything is float64 on widened float32 values.  The pair terms are the brute-force
double loop over members (``pair_gaps`` is the sorted-gap form the kernel uses, kept here to compare the two); the sums over members run
over ``np.sort``-ed values one member at a time, in the kernel's order; the maps use ``np.sort`` / ``np.median`` on the returning members
of each pixel; the counts and the rank histogram are integers."""
import numpy as np

RAW = ("unknown", "evaluated", "abs_depth_members", "pair_depth", "sq_depth_mean", "var_depth", "abs_reflectance_members", "pair_reflectance",
       "sq_reflectance_mean", "var_reflectance", "brier", "returns_expected", "false_expected")
MAPS = ("return_probability", "depth_mean", "depth_std", "depth_median", "depth_min", "depth_max", "reflectance_mean", "reflectance_std")


def pair_brute(x):
    """x (K,P) float64 -> (P,) sum over k < l of |x_k - x_l|, the double loop"""
    out = np.zeros(x.shape[1], np.float64)
    for k in range(x.shape[0]):
        for l in range(k + 1, x.shape[0]):
            out += np.abs(x[k] - x[l])
    return out


def pair_gaps(x):
    """the same from the sorted gaps: sum over i = 1 .. K-1 of i (K - i) (x_(i+1) - x_(i)), every term non-negative"""
    K = x.shape[0]
    s = np.sort(x, axis=0)
    out = np.zeros(x.shape[1], np.float64)
    for i in range(1, K):
        out += float(i * (K - i)) * (s[i] - s[i - 1])
    return out


def _channel(x, t):
    """x (K,P) member values, t (P,) target, float64 -> per pixel sum_k |x_k - t|, the pair term, the mean, sum_k (x_k - mean)^2; sums
    over the sorted members, one at a time"""
    K = x.shape[0]
    s = np.sort(x, axis=0)
    tot, sabs = np.zeros_like(t), np.zeros_like(t)
    for i in range(K):
        tot = tot + s[i]
        sabs = sabs + np.abs(s[i] - t)
    mean = tot / float(K)
    ss = np.zeros_like(t)
    for i in range(K):
        ss = ss + (s[i] - mean) * (s[i] - mean)
    return sabs, pair_brute(x), mean, ss


def scores(samples, target, known, lo, hi):
    """samples (B,K,5,H,W), target (B,5,H,W), known (B,1,H,W) float32 -> raw (B,13) float64, member (B,2,K) float64, rank (B,K+1) int64,
    maps (B,8,H,W) float32"""
    samples, target, known = (np.asarray(a, dtype=np.float32) for a in (samples, target, known))
    lo, hi = np.float32(lo), np.float32(hi)
    B, K = samples.shape[:2]
    shape = samples.shape[3:]
    raw = np.zeros((B, 13), np.float64)
    member = np.zeros((B, 2, K), np.float64)
    rank = np.zeros((B, K + 1), np.int64)
    maps = np.zeros((B, 8) + tuple(shape), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            d = samples[b, :, 0].reshape(K, -1)
            rho = samples[b, :, 4].reshape(K, -1)
            r, rt = target[b, 0].ravel(), target[b, 4].ravel().astype(np.float64)
            U = known[b, 0].ravel() == 0
            G = (lo < r) & (r < hi)
            E = U & G
            ret = (lo < d) & (d < hi)
            n = ret.sum(0)
            rhat = np.where(ret, d, np.float32(0)).astype(np.float64)
            rho = np.where(np.isnan(rho), np.float32(0), rho).astype(np.float64)
            r64 = r.astype(np.float64)
            p = n.astype(np.float64) / float(K)
            raw[b, 0], raw[b, 1] = U.sum(), E.sum()
            for c, (x, t) in enumerate(((rhat, r64), (rho, rt))):
                sabs, pair, mean, ss = _channel(x[:, E], t[E])
                raw[b, 2 + 4 * c] = sabs.sum()
                raw[b, 3 + 4 * c] = pair.sum()
                raw[b, 4 + 4 * c] = ((mean - t[E]) * (mean - t[E])).sum()
                raw[b, 5 + 4 * c] = (ss / float(K - 1)).sum() if K > 1 else 0.0
                member[b, c] = np.abs(x[:, E] - t[E]).sum(1)
            q = p - G.astype(np.float64)
            raw[b, 10] = (q[U] * q[U]).sum()
            raw[b, 11] = p[E].sum()
            raw[b, 12] = p[U & ~G].sum()
            below = (rhat[:, E] < r64[E]).sum(0)
            rank[b] = np.bincount(below, minlength=K + 1)
            m = np.zeros((8, d.shape[1]), np.float64)
            m[0] = p
            for i in range(d.shape[1]):
                v = np.sort(d[ret[:, i], i].astype(np.float64))
                if v.size:
                    tot = 0.0
                    for a in v:
                        tot += a
                    mu = tot / v.size
                    dev = 0.0
                    for a in v:
                        dev += (a - mu) * (a - mu)
                    m[1:6, i] = [mu, np.sqrt(dev / v.size) if v.size > 1 else 0.0, np.median(v), v[0], v[-1]]
            _, _, mean, ss = _channel(rho, rt)
            m[6], m[7] = mean, np.sqrt(ss / float(K))
            maps[b] = m.astype(np.float32).reshape((8,) + tuple(shape))
    return raw, member, rank, maps


def derived(raw, member):
    """(...,13), (...,2,K) -> dict of the derived values, NaN where a denominator is 0"""
    raw, member = np.asarray(raw, np.float64), np.asarray(member, np.float64)
    K = member.shape[-1]

    def ratio(num, den):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(den > 0, num / den, np.nan)

    U, E = raw[..., 0], raw[..., 1]
    out = {}
    for c, name in ((0, "depth"), (1, "reflectance")):
        a, pr, sq, var = (raw[..., 2 + 4 * c + j] for j in range(4))
        out["crps_" + name] = ratio(a / K - pr / K ** 2, E)
        out["crps_fair_" + name] = ratio(a / K - pr / (K * (K - 1)), E) if K > 1 else np.full(E.shape, np.nan)
        out["mae_" + name + "_members"] = ratio(a, K * E)
        out["best_mae_" + name] = ratio(member[..., c, :].min(-1), E)
        out["rmse_" + name + "_mean"] = np.sqrt(ratio(sq, E))
        out["spread_" + name] = np.sqrt(ratio(var, E))
        out["spread_skill_" + name] = np.sqrt((K + 1) / K * ratio(var, sq))
    out["brier_return"] = ratio(raw[..., 10], U)
    out["return_recall"] = ratio(raw[..., 11], E)
    out["false_return_rate"] = ratio(raw[..., 12], U - E)
    return out
