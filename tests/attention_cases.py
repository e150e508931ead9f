"""What the CPU preconditions (test_attention_cases_cpu.py) and the GPU tests (test_hip_attention.py) of the attention kernels share: the shape
table with the kernel every row reaches, the structured inputs, the fp64 / fp32 reference expressions and the bars.  Numpy / torch on the CPU,
integer seeds, no GPU.

Layout (attention.hip): qkv (B, 3C, N), rows [0, C) = Q, [C, 2C) = K, [2C, 3C) = V, head h owns rows h d .. h d + d - 1; out (B, C, N).

The bars, none of them tuned on a kernel:
  fp32 class   max|out - fp64| <= max(3 err32, 3e-6 max|v|), err32 = max error of the same expression in fp32 torch on the CPU: test_attention's ratio.
  one product  (pieces 1 on a matrix-pipe row) relative rms in (1e-5, 3e-3): test_attention_one_product's bounds, in (a), (c) and (d).  The lower one says
               that the reduced mode really ran; the generic kernel is fp32 whatever the mode and takes the fp32-class bar in every mode.  One deviation:
               under the span shift of (d) the upper bound cannot hold for ANY kernel of this mode -- fp16 rounding of k + c alone costs 6e-3 (a constant of
               ~27 per component takes four bits from k's own part: half an ulp of 2^-6 per component is a logit error of ~4e-3 rms per key;
               test_attention_cases_cpu.py asserts it on the emulation).  There, and in the all-negative case besides the 3e-3, the kernel is pinned to the
               emulation itself (one_product_operands): per element |out - emul| <= the rigorous bound of p's fp16 rounding + the fp32-class allowance
               max(3 err32, 3e-6 max|v|) for the fp32 accumulation.
  one-hot      |out - v[:, pi(n)]| <= 4 2^-24 |v[:, pi(n)]| per element for the fp32 kernels, 2^-21 |v[:, pi(n)]| for the split fp16 pipe.  Derivation: with a
               one-hot softmax the winning P is exp(0) = 1 exactly, every alpha that matters is exactly 1 or underflows, and l = 1 + (off mass) rounds
               to 1, so an fp32 kernel returns v (1 - eps) + eps v_other with eps < 2^-30 and one rounding of the final product: 2^-24 + 2 (max|v| / min|v|)
               2^-30 = 1.25 2^-24 with |v| in [0.5, 4).  The split pipe (f16x2.h) carries an operand as h + 2^-11 l, h and l fp16 with 11 significant bits
               each: 22 bits, representation error <= 2^-22 |v| while l stays normal (|v| > ~1e-4; v here is >= 0.5 in magnitude so that the split's absolute
               floor below that does not enter).  P = 1 splits exactly; V's split 2^-22, the plane-combining fmaf and the final product 2^-24 each and the off
               mass 2^-26 are 1.6 2^-22 -- inside 2^-21, the sum of two 22-bit operand splits (P and V).
  DC on V      pieces 2: max(3 err32, 2^-21 max|v'|) -- the same two 22-bit splits, relative to the largest operand of the convex combination."""
import math
from collections import namedtuple

import numpy as np
import torch

MODES = (1, 2, 3)  # r2dm_set_conv_pieces: 2 = split fp16 pipe (default), 1 = one fp16 product, 3 = fp32 MFMA
Row = namedtuple("Row", "what heads d N B modes kernel")  # kernel: "matrix" (the mode picks the instantiation) or the generic instantiation's DMAX

F16 = "fp16-pipe kernel"
SHAPES = [
    Row(F16 + ", one wave", 8, 64, 32, 2, MODES, "matrix"),
    Row(F16 + ", two waves", 8, 32, 64, 2, MODES, "matrix"),
    Row(F16 + ", one full block", 8, 64, 256, 2, MODES, "matrix"),
    Row(F16 + ", a block plus one wave", 8, 32, 288, 2, MODES, "matrix"),
    Row(F16 + ", a block plus one wave", 4, 64, 288, 2, MODES, "matrix"),
    Row(F16 + ", two blocks plus one wave", 2, 32, 544, 2, MODES, "matrix"),
    Row("fp32-MFMA kernel, one block plus one wave", 8, 64, 160, 2, (3,), "matrix"),
    Row("fp32-MFMA kernel, one block plus one wave", 8, 32, 160, 2, (3,), "matrix"),
    Row("generic <32>, D = DMAX", 8, 32, 50, 2, MODES, 32),
    Row("generic <32>, tiny D, one token", 4, 8, 1, 2, MODES, 32),
    Row("generic <32>, D = 1", 3, 1, 64, 2, MODES, 32),
    Row("generic <64>, head size 64 off the fast path", 8, 64, 33, 2, MODES, 64),
    Row("generic <64>", 4, 48, 64, 2, MODES, 64),
    Row("generic <64>, D = 33", 12, 33, 96, 1, MODES, 64),
    Row("generic <128>, D = 65", 2, 65, 32, 2, MODES, 128),
    Row("generic <128>, D = DMAX", 1, 128, 65, 2, MODES, 128),
    Row("one head on the fast path", 1, 64, 64, 2, MODES, "matrix"),
    Row("twelve heads on the fast path", 12, 32, 96, 2, MODES, "matrix"),
]
BY_SHAPE = {(r.heads, r.d, r.N): r for r in SHAPES}


def row_id(r):
    return f"h{r.heads}-d{r.d}-N{r.N}"


def supported(C, heads, N):
    """attention_supported (attention.hip)."""
    return heads > 0 and C % heads == 0 and N > 0 and C // heads <= 128


def kernel_for(heads, d, N, pieces):
    """The documented dispatch rule (attention.hip, launch_attention): head size 32 or 64 and N % 32 == 0 -> a matrix-pipe kernel, picked by the mode;
    otherwise the generic kernel, <32> for d <= 32, <64> for d <= 64, <128> beyond, whatever the mode."""
    assert supported(heads * d, heads, N)
    if d in (32, 64) and N % 32 == 0:
        return {1: f"attention_f16x2_kernel<{d}, 1>", 2: f"attention_f16x2_kernel<{d}, 2>", 3: f"attention_kernel<{d}>"}[pieces]
    return f"attention_generic_kernel<{32 if d <= 32 else 64 if d <= 64 else 128}>"


def is_generic(r):
    return r.kernel != "matrix"


def block_fill(N, pieces):
    """(blocks, active waves of the last block, waves per block) of a matrix-pipe launch: one wave per 32 queries, 8 waves per block in the fp16-pipe
    kernel and 4 in the fp32-MFMA kernel."""
    per = 4 if pieces == 3 else 8
    waves = N // 32
    return (waves + per - 1) // per, (waves - 1) % per + 1, per


def rnd(seed, *shape):
    return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal(shape).astype(np.float32))


def heads_view(qkv, heads):
    """(q, k, v), each a (B, heads, d, N) view of qkv's own storage."""
    B, C3, N = qkv.shape
    C = C3 // 3
    return tuple(qkv[:, i * C:(i + 1) * C].view(B, heads, C // heads, N) for i in range(3))


def assemble(q, k, v):
    B, heads, d, N = q.shape
    return torch.cat([t.reshape(B, heads * d, N) for t in (q, k, v)], 1).float().contiguous()


def logits(qkv, heads, dtype=torch.float64):
    """(B, heads, N queries, N keys)"""
    q, k, _ = heads_view(qkv.to(dtype), heads)
    return torch.einsum("bhdn,bhdm->bhnm", q, k) / math.sqrt(q.shape[2])


def attention(qkv, heads, dtype):
    """softmax(Q^T K / sqrt(d)) V per head on the fp32 inputs, evaluated in `dtype`: (B, C, N) -- test_attention's expression."""
    B, C3, N = qkv.shape
    v = heads_view(qkv.to(dtype), heads)[2]
    p = torch.softmax(logits(qkv, heads, dtype), -1)
    return torch.einsum("bhnm,bhdm->bhdn", p, v).reshape(B, C3 // 3, N)


def references(qkv, heads):
    """(fp64 truth, the fp32 expression's error against it)"""
    ref = attention(qkv, heads, torch.float64)
    return ref, attention(qkv, heads, torch.float32).double() - ref


def vmax(qkv):
    return qkv[:, 2 * (qkv.shape[1] // 3):].abs().max().item()


def fp32_class_bar(err32, v_max):
    return max(3 * err32, 3e-6 * v_max)


ONE_PRODUCT = (1e-5, 3e-3)  # test_attention_one_product's bounds on the relative rms error


def rel_rms(a, ref):
    return ((a.double() - ref.double()).pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt()).item()


def one_product_operands(qkv, heads):
    """(emul, bound), both (B, C, N) float64.  emul: the expression in fp64 on the operands as the one-product mode rounds them (attention.hip, NPLK = 1):
    q / sqrt(d) formed in fp32 and rounded to fp16, k and v rounded to fp16 -- exact products of exactly those numbers, exact softmax.  bound: what the
    mode's one further rounding can add, per output element, rigorously: the kernel rounds p = exp(s - running max) <= 1 to fp16 before the second product,
    an error of at most 2^-11 p (round to nearest, 11 significant bits) or 2^-25 (below fp16's normal range), which later rescaling by alpha <= 1 only
    shrinks; the row sum uses the unrounded p.  So |out - emul| <= sum_j (2^-11 p_nj + 2^-25) |v_j - emul_n| / l_n, p relative to the row's final maximum."""
    B, C3, N = qkv.shape
    q, k, v = heads_view(qkv, heads)
    d = q.shape[2]
    scale = np.float32(1.0) / np.sqrt(np.float32(d))  # launch_attention: 1.0f / sqrtf((float)d)
    qs, kh, vh = (q * float(scale)).half().double(), k.half().double(), v.half().double()
    s = torch.einsum("bhdn,bhdm->bhnm", qs, kh)
    p = torch.exp(s - s.amax(-1, keepdim=True))
    l = p.sum(-1)
    emul = torch.einsum("bhnm,bhdm->bhdn", p, vh) / l[:, :, None, :]
    bound = torch.empty_like(emul)
    w = (2.0 ** -11 * p + 2.0 ** -25) / l[..., None]
    for b in range(B):
        for h in range(heads):  # (d, N queries, N keys) at a time
            dev = (vh[b, h][:, None, :] - emul[b, h][:, :, None]).abs()
            bound[b, h] = (dev * w[b, h][None]).sum(-1)
    return emul.reshape(B, C3 // 3, N), bound.reshape(B, C3 // 3, N)


# ---- (a) benign ------------------------------------------------------------------------------------------------------------------------
def benign(r, seed=50):
    return rnd(seed + r.heads + r.d + r.N, r.B, 3 * r.heads * r.d, r.N)


# ---- (b) one-hot softmax by construction -----------------------------------------------------------------------------------------------
ONE_HOT_GENERIC = [(8, 32, 50), (4, 48, 64), (2, 65, 32)]  # one row per generic instantiation
ONE_HOT_SHAPES = [r for r in SHAPES if (not is_generic(r) and r.N >= 64) or (r.heads, r.d, r.N) in ONE_HOT_GENERIC]
PERMS = ("identity", "reversal", "random")
OFF_MASS = 2.0 ** -30
Q_MAX = 1e3
ONE_HOT_FP32 = 4 * 2.0 ** -24
ONE_HOT_SPLIT = 2.0 ** -21
V_LO, V_HI = 0.5, 4.0


def permutation(kind, N, seed=7):
    if kind == "identity":
        return torch.arange(N)
    if kind == "reversal":  # the low queries take keys of the last tile, query n's key sits in the other half-wave's registers
        return torch.arange(N - 1, -1, -1)
    return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).permutation(N))


def one_hot(r, kind, seed=100):
    """(qkv, pi, expected (B, C, N), gamma, seed used): keys are random unit vectors, q_n = gamma k_pi(n), |v| uniform in [0.5, 4) with a random sign.
    gamma is the smallest integer that puts every query's gap to its runner-up, gamma (1 - cos) / sqrt(d), at ln N + 30 ln 2 + 2 for the most
    correlated pair of keys: the off mass is then below N exp(-gap) = 2^-30 / e^2.  If that needs gamma >= 1000 the keys are drawn again with the
    next seed; no query is ever dropped."""
    B, heads, d, N = r.B, r.heads, r.d, r.N
    for s in range(seed, seed + 16):
        k = rnd(s, B, heads, d, N).double()
        k = (k / k.norm(dim=2, keepdim=True)).float()
        cos = torch.einsum("bhdn,bhdm->bhnm", k.double(), k.double())
        cos.diagonal(dim1=-2, dim2=-1).fill_(-1.0)
        gamma = math.ceil(math.sqrt(d) * (math.log(N) + 30 * math.log(2) + 2) / (1 - cos.max().item()))
        if gamma < Q_MAX:
            break
    else:
        raise AssertionError(f"{row_id(r)}: no key set among 16 seeds is uncorrelated enough for |q| < {Q_MAX}")
    pi = permutation(kind, N)
    g = np.random.Generator(np.random.PCG64(s + 1000))
    mag = torch.from_numpy(g.uniform(V_LO, V_HI, (B, heads, d, N)).astype(np.float32))
    v = mag * torch.from_numpy(g.choice([-1.0, 1.0], (B, heads, d, N)).astype(np.float32))
    q = (gamma * k)[..., pi]
    return assemble(q, k, v), pi, v[..., pi].reshape(B, heads * d, N), gamma, s


# ---- (c) a late maximum ----------------------------------------------------------------------------------------------------------------
LATE_SHAPES = [BY_SHAPE[s] for s in ((8, 64, 256), (8, 32, 288), (4, 64, 288), (2, 32, 544), (8, 64, 160), (8, 32, 160))]
LATE_HALVES = {"low": 2, "high": 5}  # key's place in the last tile: (pos % 32) < 4 -- the low half-wave's registers --, in [4, 8) -- the high half-wave's
LATE_QUERIES = ("wave0", "last_wave", "all")
LATE_LOGIT = 64.0


def late_queries(which, N):
    if which == "wave0":
        return [7]  # exactly one query of wave 0 of block 0
    if which == "last_wave":
        return [N - 13]  # one query of the last active wave of the last block
    return list(range(N))


def late_maximum(r, half, which, seed=200):
    """(base, mod, pos, queries).  base: benign data with head coordinate d - 1 of every query and key zeroed.  mod: the same with that coordinate of key
    `pos` (in the last 32-key tile) and of the chosen queries set to a, a^2 / sqrt(d) = 64: the key's logit is its benign one + 64 for the chosen
    queries -- about 60 above every earlier key's, below 100 -- and unchanged, to the bit, for all others (0 a = 0), whose rows must therefore
    come out as in base."""
    B, heads, d, N = r.B, r.heads, r.d, r.N
    base = rnd(seed + r.heads + r.d + r.N, B, 3 * heads * d, N)
    q, k, _ = heads_view(base, heads)
    q[:, :, d - 1] = 0
    k[:, :, d - 1] = 0
    mod = base.clone()
    q, k, _ = heads_view(mod, heads)
    pos, queries = N - 32 + LATE_HALVES[half], late_queries(which, N)
    a = math.sqrt(LATE_LOGIT * math.sqrt(d))
    q[:, :, d - 1, queries] = a
    k[:, :, d - 1, pos] = a
    return base, mod, pos, queries


# ---- (d) shift invariance --------------------------------------------------------------------------------------------------------------
SHIFT_SHAPES = [BY_SHAPE[s] for s in ((8, 64, 256), (8, 32, 288), (4, 64, 288), (8, 64, 160), (8, 32, 160), (8, 32, 50), (8, 64, 33), (4, 48, 64), (1, 128, 65))]
SHIFT_KINDS = ("span", "negative")
SHIFT_SPAN = 80.0
NEGATIVE_CENTRE = 160.0


def shifted(r, kind, seed=300):
    """qkv with k' = k + c, c one constant vector per (sample, head).
    span:     c = a Gaussian direction scaled so that the per-query logit offsets q_n . c / sqrt(d) span 160 from the lowest to the highest in every head.
    negative: q' = q + a u, k' = k - a u, u = ones / sqrt(d), a^2 / sqrt(d) = 160 (a trained in_proj has biases in both): every logit is
              -160 +- cross terms, <= -100."""
    B, heads, d, N = r.B, r.heads, r.d, r.N
    qkv = rnd(seed + r.heads + r.d + r.N, B, 3 * heads * d, N)
    q, k, _ = heads_view(qkv, heads)
    if kind == "span":
        g = rnd(seed + 1, B, heads, d, 1).double()
        off = (q.double() * g).sum(2) / math.sqrt(d)
        k += (g * 2 * SHIFT_SPAN / (off.amax(-1) - off.amin(-1))[..., None, None]).float()
    else:
        a = math.sqrt(NEGATIVE_CENTRE * math.sqrt(d)) / math.sqrt(d)
        q += a
        k -= a
    return qkv


# ---- (e) DC on V -----------------------------------------------------------------------------------------------------------------------
DC_SHAPES = [BY_SHAPE[s] for s in ((8, 64, 256), (8, 32, 288), (4, 64, 288), (8, 64, 160), (8, 32, 160), (8, 32, 50), (8, 64, 33), (1, 128, 65))]
DC_LADDER = (16, 256)
DC_SPLIT = 2.0 ** -21


def dc_on_v(r, R, seed=400):
    """(qkv, sigma): benign data with v' = v + R sigma, sigma the fp64 standard deviation of v."""
    qkv = rnd(seed + r.heads + r.d + r.N, r.B, 3 * r.heads * r.d, r.N)
    v = heads_view(qkv, r.heads)[2]
    sigma = v.double().std(unbiased=False).item()
    v += R * sigma
    return qkv, sigma


# ---- (f) containment and independence, (g) refusals ------------------------------------------------------------------------------------
INDEPENDENCE = [(BY_SHAPE[4, 64, 288], MODES), (BY_SHAPE[8, 32, 288], MODES), (BY_SHAPE[8, 32, 50], (2,)), (BY_SHAPE[8, 64, 33], (2,)), (BY_SHAPE[2, 65, 32], (2,))]
REFUSALS = {"heads = 0": (64, 0, 32), "C % heads != 0": (100, 8, 32), "N = 0": (64, 8, 0), "head size 129": (258, 2, 32)}  # (C, heads, N)
