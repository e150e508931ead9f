"""The conditioning chain of embed.hip restated stage by stage in numpy, the bound each stage is held to, the input sets of
test_hip_embed.py, and deliberately wrong restatements (the mutants) that test_embed_cpu.py uses to show those inputs and that bound
would catch a subtly wrong kernel.  No GPU, no torch in the arithmetic (torch only forms the frequency table, an INPUT of the kernels,
with the reference's own expression).

The stages, with exactly the kernels' rounding points (f32 = round to float32, everything else float64 or wider):

    emb[b]  = f32([sin64(a), cos64(a)]),  a = f32(f32(t_b) * f32(f_k))          time_hidden_kernel, the LDS fill
    hid     = f32(silu64(f32(dot(w1, emb) + b1)))                               time_hidden_kernel
    act     = f32(silu64(f32(dot(w2, hid) + b2)))                               time_out_kernel
    proj    = f32(dot(w, act) + bias)                                           ada_proj_kernel

Each stage is evaluated on the PREVIOUS stage's values as the GPU stored them (the tests pass the GPU's own hidden / act in), so one
stage's rounding is never charged to the next.

The reference dot product.  Products of two float32 are exact in float64 (48 bits).  They are summed in np.longdouble where that has a
64-bit significand (x86: pairwise, error <= log2(K) 2^-64 sum|terms|), else with math.fsum (exact): in both cases far below float64's
2^-53, i.e. the reference is more accurate than the kernel, not a different order of the same arithmetic.  `wide` below is that sum plus
the bias, rounded once to float64 (2^-53 |wide|, inside the second term of the bound).

The bound of a dot-product stage of K terms (derived, not measured).  The kernels add K exact products in float64: each lane
ceil(K / 64) of them in sequence, then six exchange steps, then the bias.  A term passes through at most n = ceil(K / 64) + 6 roundings
(additions whose other operand is zero are exact, so n <= K for small K as well), each of relative size 2^-53, hence

    |s - wide| <= ((1 + 2^-53)^n - 1) (sum_k |w_k a_k| + |bias|) <= K 2^-52 (sum_k |w_k a_k| + |bias|)  =: delta

for the kernel's float64 total s.  The stored value is got = f32(s), and |f32(s) - s| <= 1/2 spacing32(s), so

    |got - wide| <= 1/2 spacing32(wide) + delta                                                              (dot stage)

-- the error is measured against the UNROUNDED wide value: where wide lies within delta of a float32 tie the kernel may legitimately
store the other neighbour, and f32(wide) itself is only reported (`flips` counts such elements).  Since delta is some 2^-20 of a
float32 spacing, the bound says: got is one of the two float32 neighbours of wide, and the nearer one unless wide is a near-tie.

A SiLU stage stores f32(silu64(p)) of the float32 pre-activation p, |p - wide| <= beta = 1/2 spacing32(wide) + delta.  |silu'| <= 1.0999
< 1.1 on the whole line, silu64 itself (d / (1 + exp(-d)): exp within a float64 ulp, an addition, a division) is worth 2^-50 |silu|, and
the store rounds once:

    |got - silu64(wide)| <= 1.1 beta + 1/2 spacing32(silu64(wide)) + 2^-50 |silu64(wide)|                    (SiLU stage)

That bound is about one float32 spacing wide, because it is stated against silu64 of the UNROUNDED pre-activation while the kernel (and
the restated expression) rounds p first.  So a SiLU stage is held to more: p is f32(wide), or its neighbour where wide is within delta
of their midpoint; the stored value is f32(silu64(p)), or the neighbour where silu64(p) is within 2^-50 of a tie -- `admissible`, at most
six float32 values per element and almost always one.  within_bound asks for both.

The sinusoid: sin and cos of the float64 library are within one float64 ulp, so the stored float32 is the correctly rounded value or,
at a near-tie, its neighbour: `ulps(got, f32(sin64(a))) <= 1`.
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
WIDE = np.longdouble if np.finfo(np.longdouble).nmant > 52 else None  # the accumulator of dot_wide (None: math.fsum)
SILU_SLOPE = 1.1  # max |silu'| = 1.0998...
SILU_EVAL = 2.0 ** -50  # relative error of silu64 as a kernel evaluates it: exp within an ulp, one addition, one division


def f32(x):
    return np.asarray(x, dtype=F64).astype(F32)


def spacing32(x):
    """The float32 spacing at |x| (x float64 or float32), as float64."""
    with np.errstate(over="ignore"):
        return np.spacing(np.abs(np.asarray(x, dtype=F64).astype(F32))).astype(F64)


def ulps(got, ref):
    """Largest |got - ref| in float32 spacings of ref; inf where exactly one of the two is NaN or they are different infinities."""
    got, ref = np.asarray(got, dtype=F64), np.asarray(ref, dtype=F64)
    bad = (np.isnan(got) != np.isnan(ref)) | ((np.isinf(got) | np.isinf(ref)) & (got != ref) & ~np.isnan(got) & ~np.isnan(ref))
    if bad.any():
        return math.inf
    ok = np.isfinite(got) & np.isfinite(ref)
    if not ok.any():
        return 0.0
    return float((np.abs(got[ok] - ref[ok]) / spacing32(ref[ok])).max())


def silu64(x):
    x = np.asarray(x, dtype=F64)
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-x))


def freqs(base):
    """The frequency table f_k the kernels are handed: the reference's own float32 expression (SinusoidalPositionalEmbedding), as
    oracle.r2dm_oracle.sinusoidal_embedding spells it."""
    import torch

    half = base // 2
    return torch.exp(-math.log(10_000.0) / (half - 1) * torch.arange(half)).numpy().astype(F32)


def sin_args(t, fr):
    """a = f32(f32(t_b) * f32(f_k)), (B, base / 2) float32."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(t, dtype=F32)[:, None] * np.asarray(fr, dtype=F32)[None, :]


def sinusoid(t, fr):
    """emb (B, base) float32 = f32([sin64(a) | cos64(a)])."""
    a = sin_args(t, fr).astype(F64)
    with np.errstate(invalid="ignore"):
        return np.concatenate([np.sin(a), np.cos(a)], axis=1).astype(F32)


def dot_wide(w, a, bias):
    """(wide, mass): wide (B, R) float64 = sum_k w[r, k] a[b, k] + bias[r] accumulated in WIDE; mass = sum_k |w a| + |bias| (float64)."""
    w, a, bias = np.asarray(w, dtype=F64), np.asarray(a, dtype=F64), np.asarray(bias, dtype=F64)
    B, R = a.shape[0], w.shape[0]
    wide, mass = np.empty((B, R), F64), np.empty((B, R), F64)
    for b in range(B):
        with np.errstate(invalid="ignore", over="ignore"):
            prod = w * a[b][None, :]  # exact: two float32 factors
        if WIDE is not None:
            wide[b] = (prod.astype(WIDE).sum(axis=1) + bias.astype(WIDE)).astype(F64)
        else:
            wide[b] = [math.fsum(list(prod[r]) + [bias[r]]) if np.isfinite(prod[r]).all() else np.nan for r in range(R)]
        mass[b] = np.abs(prod).sum(axis=1) + np.abs(bias)
    return wide, mass


class Stage:
    """One stage's reference: `value` float64 (unrounded: wide, or silu64(wide)), `ref` = f32(value), `bound` float64 per element."""

    def __init__(self, value, bound):
        self.value, self.bound, self.ref = value, bound, f32(value)


def dot_stage(w, a, bias):
    """proj = f32(dot(w, a) + bias)."""
    K = np.asarray(w).shape[1]
    wide, mass = dot_wide(w, a, bias)
    st = Stage(wide, 0.5 * spacing32(wide) + K * 2.0 ** -52 * mass)
    st.delta = K * 2.0 ** -52 * mass  # (the float64 accumulation's share of the bound)
    return st


def silu_stage(w, a, bias):
    """f32(silu64(f32(dot(w, a) + bias))): the bound, and the few float32 values a correctly rounding kernel can store (`admissible`)."""
    pre = dot_stage(w, a, bias)
    v = silu64(pre.value)
    st = Stage(v, SILU_SLOPE * pre.bound + 0.5 * spacing32(v) + SILU_EVAL * np.abs(v))
    st.pre = pre  # (the pre-activation's own stage: what the reference calls the time embedding is act's)
    with np.errstate(invalid="ignore", over="ignore"):
        p0 = f32(pre.value)
        other = np.nextafter(p0, np.where(pre.value > p0, np.inf, -np.inf).astype(F32))  # the float32 neighbour on wide's side
        tie = 0.5 * (p0.astype(F64) + other.astype(F64))
        ps = [p0, np.where(np.abs(pre.value - tie) <= pre.delta, other, p0)]
        st.ref = f32(silu64(p0))
        st.admissible = []
        for p in ps:
            vp = silu64(p)
            st.admissible += [f32(vp), f32(vp - SILU_EVAL * np.abs(vp)), f32(vp + SILU_EVAL * np.abs(vp))]
    return st


def within_bound(got, stage):
    """(verdict, the largest error in units of the bound, flips).  The verdict: every element inside the stage's bound and, for a SiLU stage,
    one of its admissible values.  flips = elements that differ from stage.ref, the restated expression evaluated with round-to-nearest
    throughout -- inside the bound these are near-ties.  A NaN on one side where the other has none fails."""
    got = np.asarray(got, dtype=F64)
    assert got.shape == stage.value.shape, (got.shape, stage.value.shape)
    nan_g, nan_r = np.isnan(got), np.isnan(stage.value)
    if (nan_g != nan_r).any():
        return False, math.inf, int((nan_g != nan_r).sum())
    ok = ~nan_r
    if not ok.any():
        return True, 0.0, 0
    worst = float((np.abs(got[ok] - stage.value[ok]) / stage.bound[ok]).max())
    g32 = got.astype(F32)
    admitted = np.ones(got.shape, bool)
    if hasattr(stage, "admissible"):
        admitted = np.zeros(got.shape, bool)
        for c in stage.admissible:
            admitted |= g32 == c
    return worst <= 1.0 and bool(admitted[ok].all()), worst, int((g32[ok] != stage.ref[ok]).sum())


def time_embedding(t, fr, w1, b1, w2, b2, hidden=None):
    """(emb, Stage of hidden, Stage of act): the act stage on `hidden` (the GPU's own) where given, else on the reference's."""
    emb = sinusoid(t, fr)
    h = silu_stage(w1, emb, b1)
    return emb, h, silu_stage(w2, h.ref if hidden is None else hidden, b2)


# ---- the input sets of test_hip_embed.py -----------------------------------------------------------------------------------------------------
def rng(*key):
    return np.random.Generator(np.random.PCG64(list(key)))


TIME_SHAPES = [(64, 256), (128, 512), (32, 128), (8, 10), (6, 7), (520, 260)]  # (base, T)
TIME_BATCHES = [1, 5, 9, 33]
_CONDS = [0.5, -3.2, 999.0, 0.0, 1.0, 500.0, 1e-8, 1e4, -15.0, 15.0, 0.25]  # continuous log-SNR, [0, 1] times, discrete steps, the extremes


def conds(B):
    """B distinct conditions: the named ones first, then log-SNR values between -12 and 12."""
    rest = np.linspace(-12.0, 12.0, 33 - len(_CONDS)) + 0.0625
    return np.concatenate([np.asarray(_CONDS), rest])[:B].astype(F32)


SIN_CONDS = {"unit": np.linspace(0.0, 1.0, 33).astype(F32), "discrete": np.asarray([0.0, 1.0, 500.0, 999.0], F32),
             "extreme": np.asarray([1e-8, -3.2, 1e4], F32)}  # (plus the golden file's sin_t)


def one_hot_weights(base):
    """(w1, b1, w2, b2) with T = base: w1 the identity and b1 = 0, so hidden[b][r] = silu(emb[b][r]); w2, b2 anything finite."""
    g = rng(7, base)
    return (np.eye(base, dtype=F32), np.zeros(base, F32), (g.standard_normal((base, base)) / math.sqrt(base)).astype(F32),
            g.standard_normal(base).astype(F32))


def time_weights(base, T):
    """Random weights at the scale of a trained network's (Linear's 1 / sqrt(fan-in))."""
    g = rng(11, base, T)
    return ((g.standard_normal((T, base)) / math.sqrt(base)).astype(F32), (0.5 * g.standard_normal(T)).astype(F32),
            (g.standard_normal((T, T)) / math.sqrt(T)).astype(F32), (0.5 * g.standard_normal(T)).astype(F32))


def time_exact(base, T):
    """t = 0: emb = [0 .. 0, 1 .. 1] exactly; integer w1, b1 -> (w1, b1, n) with n (T,) the exact integer pre-activation."""
    r, k = np.arange(T)[:, None], np.arange(base)[None, :]
    w1 = ((5 * r + k) % 13 - 6).astype(F32)
    b1 = ((3 * np.arange(T)) % 7 - 3).astype(F32)
    n = w1[:, base // 2:].astype(np.int64).sum(axis=1) + b1.astype(np.int64)
    return w1, b1, n


ADA_VECTOR_T, ADA_SCALAR_T = [256, 512, 768], [64, 100, 257, 320]
ADA_ROWS, ADA_BATCHES = [1, 3, 4, 5, 130], [1, 7, 8, 9, 15, 16, 17, 32, 33]


def ada_cases():
    """(T, B, rows): every T at B in {9, 33} and rows in {5, 130}; every B and rows at T in {256, 100}."""
    cases = [(T, B, R) for T in ADA_VECTOR_T + ADA_SCALAR_T for B in (9, 33) for R in (5, 130)]
    cases += [(T, B, R) for T in (256, 100) for B in ADA_BATCHES for R in ADA_ROWS]
    return sorted(set(cases))


ADA_BIAS_STEP, ADA_SAMPLE_STEP = 1 << 17, 1 << 13  # the exact case's tags: see ada_exact


def ada_exact(T, B, rows):
    """(act, w, bias, out): integer activations that differ per sample, integer weights that differ per row, an integer bias; out (B, rows)
    int64, the exact result.  The patterns in k leave |dot| of a few thousand; on top of them term 0 tags the sample (act[b][0] = b - 16 times
    w[r][0] = ADA_SAMPLE_STEP) and the bias tags the row (a multiple of ADA_BIAS_STEP), each step more than twice what lies below it -- so
    out is pairwise distinct within a row and within a sample (test_embed_cpu.py checks that, and that sum |terms| stays below 2^24)."""
    b, r, k = np.arange(B)[:, None], np.arange(rows)[:, None], np.arange(T)[None, :]
    act = (7 * b + 3 * k + (b * k) % 5) % 37 - 18
    w = (5 * r + k + (r * k) % 3) % 13 - 6
    act[:, 0], w[:, 0] = np.arange(B) - 16, ADA_SAMPLE_STEP
    bias = (np.arange(rows) - rows // 2) * ADA_BIAS_STEP + (3 * np.arange(rows)) % 17 - 8
    out = act.astype(np.int64) @ w.astype(np.int64).T + bias[None, :]
    return act.astype(F32), w.astype(F32), bias.astype(F32), out


def ada_random(T, B, rows):
    """(act, w, bias): SiLU of N(0, 1) activations, as the network's are; weights N(0, 1) / sqrt(T); bias N(0, 1) (distinct per row)."""
    g = rng(13, T, B, rows)
    act = silu64(g.standard_normal((B, T))).astype(F32)
    return act, (g.standard_normal((rows, T)) / math.sqrt(T)).astype(F32), g.standard_normal(rows).astype(F32)


# ---- the mutants: each a wrong kernel, restated ------------------------------------------------------------------------------------------------
def dot_kernel_order(w, a, bias, dtype):
    """A kernel of embed.hip's shape with every product and sum in `dtype`: lane-strided partials (lane = k % 64), a six-step tree, the bias.
    float64: a model of the kernels as they are (unrounded); float32: the fp32-accumulation mutant."""
    w, a = np.asarray(w, dtype=dtype), np.asarray(a, dtype=dtype)
    K = w.shape[1]
    pad = (-K) % 64
    prod = w[None, :, :] * a[:, None, :]  # (B, R, K)
    prod = np.concatenate([prod, np.zeros(prod.shape[:2] + (pad,), dtype)], axis=2).reshape(prod.shape[0], prod.shape[1], -1, 64)
    lanes = np.zeros(prod.shape[:2] + (64,), dtype)
    for i in range(prod.shape[2]):
        lanes = lanes + prod[:, :, i, :]
    n = 64
    while n > 1:
        n //= 2
        lanes = lanes[..., :n] + lanes[..., n:2 * n]
    return lanes[..., 0] + np.asarray(bias, dtype=dtype)[None, :]


def _dot(w, a, bias):
    """The right kernel's float32 result."""
    return f32(dot_wide(w, a, bias)[0])


def mut_fp32_accumulate(w, a, bias):
    return dot_kernel_order(w, a, bias, F32)


def mut_drop_last(w, a, bias):
    return _dot(np.asarray(w)[:, :-1], np.asarray(a)[:, :-1], bias)


def mut_double_last(w, a, bias):
    w, a = np.asarray(w), np.asarray(a)
    return _dot(np.concatenate([w, w[:, -1:]], 1), np.concatenate([a, a[:, -1:]], 1), bias)


def mut_next_bias(w, a, bias):
    """(None: a single row has no neighbour)"""
    return _dot(w, a, np.roll(np.asarray(bias), -1)) if len(bias) > 1 else None


def mut_swap_pair(w, a, bias):
    """Samples b and b ^ 1 swapped in the last group of eight that holds at least two samples (None: B = 1)."""
    out = _dot(w, a, bias)
    B = out.shape[0]
    if B < 2:
        return None
    b0 = (B - 1) // 8 * 8
    if B - b0 < 2:
        b0 -= 8
    idx = np.arange(B)
    for b in range(b0, min(b0 + 8, B) - 1, 2):
        idx[b], idx[b + 1] = b + 1, b
    return out[idx]


def mut_tail_clamp(w, a, bias):
    """The clamped lanes of the last, partial group of eight (j >= B - b0: they READ sample b0 instead of one past the batch, and add
    nothing) also WRITE: row b0 ends as what the last of them holds, the bias alone (None: B % 8 == 0, no such lane)."""
    out = _dot(w, a, bias).copy()
    B = out.shape[0]
    if B % 8 == 0:
        return None
    out[B // 8 * 8] = np.asarray(bias, dtype=F32)
    return out


def mut_swap_halves(t, fr):
    emb = sinusoid(t, fr)
    h = emb.shape[1] // 2
    return np.concatenate([emb[:, h:], emb[:, :h]], axis=1)


def mut_fp32_sincos(t, fr):
    """sin / cos evaluated in float32: np.sin on float32 behind the float32 range reduction a - round(a / 2 pi) f32(2 pi) of a fast sinf
    (np.sin on the float32 argument alone is correctly rounded on some hosts, i.e. no mutant there)."""
    a = sin_args(t, fr)
    two_pi = F32(2.0 * math.pi)
    with np.errstate(invalid="ignore"):
        red = (a - np.round(a / two_pi).astype(F32) * two_pi).astype(F32)
        return np.concatenate([np.sin(red), np.cos(red)], axis=1).astype(F32)


DOT_MUTANTS = {"fp32 accumulation": mut_fp32_accumulate, "last term dropped": mut_drop_last, "term T-1 twice": mut_double_last,
               "bias of row r+1": mut_next_bias}
SAMPLE_MUTANTS = {"b <-> b^1 in a group": mut_swap_pair, "tail clamp writes row b0": mut_tail_clamp}
SINUSOID_MUTANTS = {"sin / cos halves swapped": mut_swap_halves, "fp32 sin / cos": mut_fp32_sincos}


# ---- a checkpoint's own projections, packed as the engine packs them ---------------------------------------------------------------------------
STAGES = ("d_block1", "d_block2", "d_block3", "d_block4", "u_block4", "u_block3", "u_block2", "u_block1")  # plan.hip: the order of the rows


def packed_ada(sd):
    """(w (ada_rows, T), bias (ada_rows,)) float32 of a U-Net state dict (tensors or arrays): every residual block's norm2.proj.1 in the
    order of the forward walk."""
    ws, bs = [], []
    for s in STAGES:
        i = 0
        while f"{s}.residual_blocks.{i}.norm2.proj.1.weight" in sd:
            ws.append(np.asarray(sd[f"{s}.residual_blocks.{i}.norm2.proj.1.weight"], dtype=F32))
            bs.append(np.asarray(sd[f"{s}.residual_blocks.{i}.norm2.proj.1.bias"], dtype=F32))
            i += 1
    return np.concatenate(ws, 0), np.concatenate(bs, 0)
