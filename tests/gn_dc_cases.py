"""What the CPU model (test_gn_statistics_cpu.py) and the GPU ladder (test_hip_gn_dc_offset.py) of "GroupNorm from fused statistics under a
DC offset" share: the case table, the ladder of |mean| / sigma, the DC recipe and the bar.

The fused statistics are [sum, sum of squares]; gn_moments (gn_math.h) forms var = E[x^2] - mean^2, which multiplies the relative error of
the two sums by about R^2 for a group with |mean| / sigma = R.  A residual stream with a DC component has such groups; zero-mean test data
has none."""
import numpy as np
import torch
import torch.nn.functional as F

GROUPS = 8
EPS = 1e-6
# (Cin, Cout, H, W, B, groups, channels per group): the smallest fused geometries of test_hip_conv_engine_paths.SHAPES, and the network's own
# level-4 group -- 64 channels x 8 x 128 = 65 536 values, 128 slots per group
CASES = [
    (64, 64, 4, 64, 2, 8, 8),
    (64, 128, 8, 128, 2, 8, 16),
    (64, 256, 8, 64, 3, 8, 32),
    (64, 512, 4, 64, 3, 8, 64),
    (256, 512, 4, 64, 2, 8, 64),
    (64, 512, 8, 128, 1, 8, 64),
]
LADDER = (0, 4, 16, 64)  # R = |mean| / sigma of every group

# (case, R) pairs that are measured and printed but not asserted, each with its reason.  The CPU model asserts that the "four" and "fp64"
# classes meet the bar on every draw at every pair that is NOT listed here, and that "four" misses it on some draw at every pair that is.
# Expected from a single draw: R = 64 at the 2048-element group alone.  Over 32 draws the model says more: the error that is left is one
# rounding pattern per (sample, group) -- of the four-pixel sums, times R^2 = 4096 in the variance -- so max error / reference max error is the
# ratio of two maxima over 8 ... 24 groups, and at R = 64 its median is 2.4 ... 3.6 against the bar of 4 at EVERY geometry of the table: the
# "four" class misses in 5 ... 9 of the model's 32 draws where a group has 16 384 values, in 1 (of another 32: in 4) where it has 65 536 and in 30
# where it has 2048.  A GPU assertion there would pass or fail with the draw, whatever the kernel does.  R = 16 is asserted everywhere
# (median 0.9 ... 2.2).
_R64 = ("R = 64: the 'four' class itself misses the x4 max bar in {} of 32 draws of the CPU model (test_gn_statistics_cpu.py) -- fp32 roundoff of the "
        "four-pixel sums times R^2 = 4096, one pattern per group")
RECORDED = {
    ((64, 64, 4, 64, 2, 8, 8), 64): _R64.format(30) + "; 2048 values per group: 512 four-pixel sums and no further slots to average them down",
    ((64, 128, 8, 128, 2, 8, 16), 64): _R64.format(9),
    ((64, 256, 8, 64, 3, 8, 32), 64): _R64.format(5),
    ((64, 512, 4, 64, 3, 8, 64), 64): _R64.format(7),
    ((256, 512, 4, 64, 2, 8, 64), 64): _R64.format(9),
    ((64, 512, 8, 128, 1, 8, 64), 64): _R64.format(1) + " (4 of another 32); 8 groups in all: the reference's own maximum varies by x2 from draw to draw, the bar with it",
}


def case_id(case):
    cin, cout, h, w, b, g, cpg = case
    return f"{cin}-{cout}-{h}x{w}-B{b}-G{g}x{cpg}"


def asserted(case, R):
    return (tuple(case), R) not in RECORDED


def signs(groups=GROUPS):
    """+1, -1, +1, ... per group."""
    return torch.tensor([1.0 if g % 2 == 0 else -1.0 for g in range(groups)], dtype=torch.float64)


def per_channel(per_group, cpg):
    """(..., groups) -> (..., groups * cpg)"""
    return per_group.repeat_interleave(cpg, dim=-1)


def group_std(y, groups=GROUPS):
    """Per-group fp64 standard deviation over the batch, the group's channels and the pixels: (groups,)."""
    B, C = y.shape[:2]
    return y.double().reshape(B, groups, -1).transpose(0, 1).reshape(groups, -1).std(-1, unbiased=False)


def dc_per_channel(y0, R, cpg, groups=GROUPS):
    """The DC recipe: +-R sigma per group with alternating sign, sigma the per-group fp64 std of the zero-DC output y0; (C,) float64.  A
    producer whose output is (conv + bias + residual) / sqrt(2) gives bias and residual this much / sqrt(2) EACH, so that the output carries
    +-R sigma and the ladder's R is the |mean| / sigma the CPU model was run at (the GPU test checks: >= 0.9 R)."""
    return per_channel(signs(groups) * R * group_std(y0, groups), cpg)


def dc_ratio(y, groups=GROUPS):
    """|mean| / sigma of every (sample, group) of y, in fp64: (B, groups)."""
    t = y.double().reshape(y.shape[0], groups, -1)
    return t.mean(-1).abs() / t.std(-1, unbiased=False)


def fir_row_profile(h_in):
    """u (h_in,) float64 with FIR_rows(u) = 1 on every output row, the least-norm one: the [1, 3, 3, 1] / 8 window of the stride-2 resampler is
    zero-padded in the rows, so a CONSTANT input comes out 7/8 as large on the first and last output row -- at R = 64 that step alone would be
    a standard deviation of several sigma.  (The columns are circular: a constant stays one.)"""
    f = [0.125, 0.375, 0.375, 0.125]
    A = np.zeros((h_in // 2, h_in))
    for i in range(h_in // 2):
        for t in range(4):
            if 0 <= 2 * i - 1 + t < h_in:
                A[i, 2 * i - 1 + t] = f[t]
    u = np.linalg.pinv(A) @ np.ones(h_in // 2)
    assert np.abs(A @ u - 1).max() < 1e-12
    return torch.from_numpy(u)


def references(y, groups=GROUPS):
    """(fp64 GroupNorm of y, error of torch's fp32 GroupNorm of the same y against it) on the CPU; y is fp32 as the kernel stored it."""
    y = y.detach().float().cpu()
    ref64 = F.group_norm(y.double(), groups, eps=EPS)
    return ref64, F.group_norm(y, groups, eps=EPS).double() - ref64


MAX_FACTOR, RMS_FACTOR, MAX_FLOOR = 4.0, 2.0, 1e-6


def bar(x_hat, ref64, ref_err):
    """The rule of test_hip_configs.py for an error relative to the reference's own: max error <= 4 x the fp32 reference's max error (with a
    floor of 1e-6 absolute, test_group_norm_stats' bar), rms error <= 2 x its rms error.  Returns (ok, max ratio, rms ratio, max error, rms error)."""
    e = x_hat.detach().double().cpu() - ref64
    emax, erms = e.abs().max().item(), e.pow(2).mean().sqrt().item()
    rmax, rrms = ref_err.abs().max().item(), ref_err.pow(2).mean().sqrt().item()
    ok = emax <= max(MAX_FACTOR * rmax, MAX_FLOOR) and erms <= RMS_FACTOR * rrms
    return ok, emax / rmax, erms / rrms, emax, erms
