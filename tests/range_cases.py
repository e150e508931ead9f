"""What the CPU table (test_range_bound_cpu.py) and the GPU tests (test_hip_range_producers.py) of the fp16 range guard's GroupNorm bound
share: a Python mirror of gn_moments / gn_affine / gn_bound (gn_math.h) and of the two ways gn_finalize_kernel (norm.hip) gets its M, one
numpy float32 operation per fp32 operation of the kernels, and the table of data cases.

The mirror states the contract: the recorded bound is what `bound` returns for the statistics the producer left, and it is SOUND --
bound >= max|a x + d| over the group's data for the (a, d) that the consumers apply -- for statistics of every summation class the
producers have:

  fp64  every addition in fp64 (conv_epilogue, the FIR and down-GEMM statistics, the streaming kernel);
  four  (v0 + v1) + (v2 + v3) and fma(v3, v3, fma(v2, v2, fma(v1, v1, v0 v0))) in fp32, fp64 beyond (conv_epilogue_wide, conv_f16x2.hip's
        two-plane instances: the parity modes) -- gn_dc_cases.py's class of the same name;
  f32   a slot's values pairwise in fp32, fp64 from the slot on (conv_f16x2.hip's one-plane instance, the fp16 bulk mode: conv_epilogue.h).  A
        wave's share of a slot is 512 values (2 + 1 + 6 levels); groups of 16 and of 32 or 64 channels merge two and four 8-channel blocks
        in fp32 behind that: F32_SLOT = 2048 values, 11 levels, is the longest chain and the one the tables use.

SUMS_EPS: what gn_bound assumes of them.  With u = 2^-24: a value goes through at most 11 fp32 additions on its way into a slot sum, its
square through one rounding more, so |sum_c - sum| <= 11 u sum|x| and |sq_c - sq| <= 12 u sq, and

  var_c - var = (sq_c - sq) / n - (mean_c^2 - mean^2),   |var_c - var| <= (12 u + 2 * 11 u)(mean^2 + var) = 34 u (mean^2 + var) < 2^-18 (mean^2 + var)

so that (var + eps) / (var_c + eps) <= 1 + 2^-18 (1 + mean_c^2 rstd_c^2) to first order: the factor by which the computed rstd may exceed
the exact one, and with it the computed |x_hat| Samuelson's sqrt(n - 1).  gn_bound widens the worst-case bound by its square root."""
import numpy as np

EPS = 1e-6
FP16_MAX = 65504.0
SUMS_EPS = 2.0 ** -18
F32_SLOT = 2048
CLASSES = ("fp64", "four", "f32")
f32 = np.float32


# ---- the sums a producer leaves ------------------------------------------------------------------------------------------------------------
def _pairwise_f32(a):
    a = a.astype(np.float32)
    while a.shape[-1] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


def slot_sums(x, cls, slot_len):
    """x (..., n) float32 -> (..., n / slot_len, 2) float64 [sum, sum of squares] per slot of slot_len consecutive values (a multiple of 4; a
    power of two for the f32 class), in the arithmetic of the class."""
    assert x.dtype == np.float32 and x.shape[-1] % slot_len == 0 and slot_len % 4 == 0
    t = x.reshape(*x.shape[:-1], -1, slot_len)
    with np.errstate(all="ignore"):
        if cls == "fp64":
            d = t.astype(np.float64)
            s, q = d.sum(-1), (d * d).sum(-1)
        elif cls == "four":
            v = t.reshape(*t.shape[:-1], -1, 4)
            v0, v1, v2, v3 = (v[..., i] for i in range(4))
            fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)  # (a b is exact in fp64)
            s4, q4 = (v0 + v1) + (v2 + v3), fma(v3, v3, fma(v2, v2, fma(v1, v1, v0 * v0)))
            s, q = s4.astype(np.float64).sum(-1), q4.astype(np.float64).sum(-1)
        else:
            assert cls == "f32" and slot_len & (slot_len - 1) == 0
            s, q = _pairwise_f32(t).astype(np.float64), _pairwise_f32(t * t).astype(np.float64)
    return np.stack([s, q], -1)


# ---- gn_math.h, norm.hip ---------------------------------------------------------------------------------------------------------------------
def moments(s, q, n, eps=EPS):
    """gn_moments: fp64 [sum, sum of squares] of a group of n values (arrays of one shape) -> (mean, rstd) float32, well_conditioned."""
    with np.errstate(all="ignore"):
        mean_d = s / np.float64(n)
        var_d = q / np.float64(n) - mean_d * mean_d
        var_d = np.where(var_d > 0.0, var_d, 0.0)  # (a NaN variance clamps too: the comparison is false)
        rstd = (1.0 / np.sqrt(var_d + np.float64(np.float32(eps)))).astype(np.float32)
        return mean_d.astype(np.float32), rstd, var_d > 1e-6 * mean_d * mean_d


def affine(mean, rstd, w, sh):
    """gn_affine: a = rstd w, d = fmaf(-mean, a, sh); mean, rstd (...,) and w, sh (..., cpg) float32 -> a, d (..., cpg)."""
    with np.errstate(all="ignore"):
        a = rstd[..., None] * w
        d = (-mean[..., None].astype(np.float64) * a.astype(np.float64) + sh.astype(np.float64)).astype(np.float32)  # (the product is exact in fp64)
    return a, d


def sink_gmax(slots):
    """gn_finalize_kernel without a recorded maximum: M = sqrt(largest slot energy) * 1.000001 (a NaN slot never wins the comparison)."""
    with np.errstate(all="ignore"):
        emax = np.fmax.reduce(slots[..., 1], axis=-1, initial=0.0)
        return np.sqrt(emax).astype(np.float32) * f32(1.000001)


def data_gmax(x):
    """gn_partial_kernel: the exact max|x| of the group (fmaxf: a NaN element never wins)."""
    with np.errstate(all="ignore"):
        return np.fmax.reduce(np.abs(x), axis=-1, initial=f32(0))


def _data_and_safe(mean, rstd, a, d, w, sh, gmax):
    data = np.abs(a) * gmax[..., None] + np.abs(d)
    safe = np.abs(w) * rstd[..., None] * (gmax + np.abs(mean))[..., None] + np.abs(sh)
    return data, np.where(data > safe, data, safe)


def bound(mean, rstd, wc, a, d, w, sh, gmax, n):
    """gn_bound -> (bound (..., cpg) float32, branch (..., cpg) of 'data' | 'worst' | 'safe')."""
    with np.errstate(all="ignore"):
        data, safe = _data_and_safe(mean, rstd, a, d, w, sh, gmax)
        r = mean * rstd  # |mean| / sigma, as computed
        widened = np.sqrt(np.float64(n) * (1.0 + SUMS_EPS * (1.0 + r.astype(np.float64) * r.astype(np.float64)))).astype(np.float32)
        worst = (np.abs(w) * widened[..., None] + np.abs(sh)) * f32(1.000001)
        lo = np.where(wc[..., None], data, safe)
        take_worst = lo > worst
        out = np.where(take_worst, worst, lo)
        branch = np.where(take_worst, "worst", np.where(wc[..., None], "data", "safe"))
    assert out.dtype == np.float32
    return out, branch, worst


def bound_before(mean, rstd, wc, a, d, w, sh, gmax, n):
    """gn_bound as it was: Samuelson's bound with a margin of 1e-6 wherever var > 1e-6 mean^2 -- it holds for the exact variance only.  Kept so
    that the CPU table shows what it missed (test_range_bound_cpu.py)."""
    with np.errstate(all="ignore"):
        data, safe = _data_and_safe(mean, rstd, a, d, w, sh, gmax)
        worst = (np.abs(w) * f32(np.sqrt(np.float64(n))) + np.abs(sh)) * f32(1.000001)
        return np.where(wc[..., None], np.where(data > worst, worst, data), safe)


def applied_max(x, a, d):
    """float32(max|a x + d|) over the group's data, the product in fp64: x (..., n), a and d (..., cpg), channel c owns n / cpg consecutive values.
    A NaN anywhere gives NaN."""
    cpg = a.shape[-1]
    t = x.astype(np.float64).reshape(*x.shape[:-1], cpg, -1)
    with np.errstate(all="ignore"):
        y = np.abs(t * a.astype(np.float64)[..., None] + d.astype(np.float64)[..., None])
        return y.max(axis=(-1, -2)).astype(np.float32)  # (np.max propagates a NaN)


class Result:
    """One group set through the mirror: everything the tests print and compare."""

    def __init__(self, x, w, sh, slots=None, bound_fn=bound, gmax=None):
        """gmax: M in place of the one the statistics give (what a producer that missed an element would have recorded)."""
        n = x.shape[-1]
        self.n = n
        if slots is None:  # the streaming pass: fp64 sums of the data, M = max|x|
            d = x.astype(np.float64)
            with np.errstate(all="ignore"):
                s, q = d.sum(-1), (d * d).sum(-1)
            self.gmax = data_gmax(x)
        else:
            with np.errstate(all="ignore"):
                s, q = slots[..., 0].sum(-1), slots[..., 1].sum(-1)
            self.gmax = sink_gmax(slots)
        if gmax is not None:
            self.gmax = gmax
        self.mean, self.rstd, self.wc = moments(s, q, n)
        self.a, self.d = affine(self.mean, self.rstd, w, sh)
        got = bound_fn(self.mean, self.rstd, self.wc, self.a, self.d, w, sh, self.gmax, n)
        self.bound, self.branch, self.worst = got if isinstance(got, tuple) else (got, None, None)
        self.applied = applied_max(x, self.a, self.d)  # per group
        with np.errstate(all="ignore"):
            self.record = np.fmax.reduce(self.bound.reshape(-1)) if not np.isnan(self.bound).any() else f32(np.nan)
            self.data_bound = np.abs(self.a) * self.gmax[..., None] + np.abs(self.d)

    def sound(self):
        """bound (1 + 2^-20) >= float32(max|a x + d|) for every group (its loosest channel bounds the group no less than the tightest one:
        the guard records the maximum).  Derived: the bound carries two or three fp32 roundings, 2^-24 each."""
        per_group = self.bound.max(-1).astype(np.float64) * (1.0 + 2.0 ** -20)
        return bool((per_group >= self.applied.astype(np.float64)).all())


def ulps(a, b):
    """Distance of two positive finite float32 in units of the last place."""
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


# ---- the data cases ----------------------------------------------------------------------------------------------------------------------------
N, CPG = 32768, 64  # one group of the table: 64 channels of 512 values, 64 slots of 512


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _plain(cpg):
    return np.ones(cpg, np.float32), np.zeros(cpg, np.float32)


def case_noise(seed, n=N, cpg=CPG):
    """(a) zero-mean unit noise; w = 1, sh = 0."""
    return _rng(1, seed).standard_normal(n).astype(np.float32), *_plain(cpg)


def case_dc(R, seed, n=N, cpg=CPG):
    """(b) |mean| / sigma = R."""  # (R = 4 and 64: the data bound is the smaller one with the exact M; R = 300: the widened worst case)
    return (_rng(2, seed, R).standard_normal(n) + R).astype(np.float32), *_plain(cpg)


def case_constant(value, n=N, cpg=CPG, sh=0.0):
    """(c) a constant group: the variance clamps to 0.  With value = 1e-3 and sh = 1 the shift cancels mean * a in d and |mean| rstd = 1: the one
    corner where gn_moments' well_conditioned alone decides the form of the data bound (|a| M + |d| = 1 against |w| rstd (M + |mean|) + |sh| = 3)."""
    return np.full(n, value, np.float32), np.ones(cpg, np.float32), np.full(cpg, sh, np.float32)


def case_pedestal_spike(seed, n=N, cpg=CPG):
    """(d) unit noise on a pedestal R in [6e4, 9e4] and one element at R + 100 sqrt(n): var / mean^2 in [1.2e-6, 3e-6] -- 'well conditioned' by
    gn_moments' rule, |mean| / sigma of 580 ... 910 -- and the spike's normalised value is all but Samuelson's sqrt(n - 1)."""
    g = _rng(4, seed)
    R = g.uniform(6e4, 9e4)
    x = g.standard_normal(n) + R
    x[g.integers(n)] = R + 100.0 * np.sqrt(n)
    return x.astype(np.float32), *_plain(cpg)


def case_spike(seed, n=N, cpg=CPG):
    """(e) one spike of 1e6 on zero-mean unit noise: |a| M + |d| = sqrt(n) (1 + 1.5 / n) -- the worst-case bound is the smaller one."""
    g = _rng(5, seed)
    x = g.standard_normal(n)
    x[g.integers(n)] = 1e6
    return x.astype(np.float32), *_plain(cpg)


def case_adagn(seed, n=N, cpg=CPG):
    """(f) AdaGN: w = 1 + scale with |w| log-uniform over [1, 6000] and either sign, shifts N(0, 1) (test_hip_range.py's preflight)."""
    g = _rng(6, seed)
    w = (10.0 ** g.uniform(0.0, np.log10(6000.0), cpg) * np.where(g.random(cpg) < 0.5, -1.0, 1.0)).astype(np.float32)
    w[0] = 6000.0
    scale = w - f32(1)
    return g.standard_normal(n).astype(np.float32), f32(1) + scale, g.standard_normal(cpg).astype(np.float32)  # (w as the kernel forms it)


def case_gain(seed, n=N, cpg=CPG):
    """(f) a GroupNorm gain of 3e4 on every channel (test_gains_that_really_leave_the_fp16_range_fail_loudly)."""
    return _rng(7, seed).standard_normal(n).astype(np.float32), np.full(cpg, 3.0e4, np.float32), np.zeros(cpg, np.float32)


def case_nonfinite(value, seed, n=N, cpg=CPG):
    """(g), (h) one +inf / one NaN element in unit noise."""
    g = _rng(8, seed)
    x = g.standard_normal(n).astype(np.float32)
    x[g.integers(n)] = value
    return x, *_plain(cpg)


D_DRAWS = 8
TABLE = {
    "a-noise": lambda n=N, cpg=CPG: case_noise(0, n, cpg),
    "b-dc4": lambda n=N, cpg=CPG: case_dc(4, 0, n, cpg),
    "b-dc64": lambda n=N, cpg=CPG: case_dc(64, 0, n, cpg),
    "b-dc300": lambda n=N, cpg=CPG: case_dc(300, 0, n, cpg),
    "c-const3.25": lambda n=N, cpg=CPG: case_constant(3.25, n, cpg),
    "c-const0.1": lambda n=N, cpg=CPG: case_constant(0.1, n, cpg),
    "c-const1e-3-shift1": lambda n=N, cpg=CPG: case_constant(1e-3, n, cpg, sh=1.0),
    **{f"d-pedestal-spike{i}": (lambda i: lambda n=N, cpg=CPG: case_pedestal_spike(i, n, cpg))(i) for i in range(D_DRAWS)},
    "e-spike": lambda n=N, cpg=CPG: case_spike(0, n, cpg),
    "f-adagn6000": lambda n=N, cpg=CPG: case_adagn(0, n, cpg),
    "f-gain3e4": lambda n=N, cpg=CPG: case_gain(0, n, cpg),
    "g-inf": lambda n=N, cpg=CPG: case_nonfinite(np.inf, 0, n, cpg),
    "h-nan": lambda n=N, cpg=CPG: case_nonfinite(np.nan, 0, n, cpg),
}
FINITE = [k for k in TABLE if k[0] not in "gh"]


def line(label, res, record=None):
    """One printed line per case: record (GPU) | mirror bound | max|a x + d| | branches taken."""
    br = "" if res.branch is None else ",".join(sorted(set(res.branch.reshape(-1).tolist())))
    rec = "" if record is None else f"record {record:.9g}  "
    return f"{label}: {rec}mirror bound {float(res.record):.9g}  max|a x + d| {float(np.max(res.applied)):.9g}  M {float(np.max(res.gmax)):.6g}  branch {br}"
