"""-m gpu: GroupNorm from the FUSED statistics under a DC offset, producer by producer.

Every other test of these statistics draws zero-mean data, and holds the sums against sum|y| and sum y^2 -- bars that do not see what
gn_moments (gn_math.h) does with them: var = E[y^2] - mean^2 multiplies the sums' relative error by (mean / sigma)^2.  Here every group of
the output carries +-R sigma, R in {0, 4, 16, 64} (gn_dc_cases.py: the case table, the DC recipe, the bar), and what is checked is the
NORMALISED tensor: sink -> gn_finalize_kernel (r2dm_group_norm_from_stats; the consumer-side fold of conv_f16x2.hip repeats its arithmetic
bit for bit) -> x a + d (r2dm_affine_act), against fp64 GroupNorm of the stored output, relative to the error of torch's fp32 GroupNorm
of the same tensor: max error <= 4 x, rms error <= 2 x (floor 1e-6 on the max).  The streaming statistics (r2dm_group_norm_affine: fp64
from the first addition) are measured on the same tensor and must meet the bar at every R.

Producers: the convolution kernels of test_hip_conv_engine_paths.VARIANTS (prologue 2 -- 1 for proj_f16x2.hip --, residual, 1 / sqrt(2)),
fir_down2_stats_kernel and the down-sampling GEMM.  Which (case, R) pairs are asserted is gn_dc_cases.RECORDED's business (the CPU model
of test_gn_statistics_cpu.py: the 'four' class itself misses the bar at R = 64); producers whose every addition is fp64 are asserted at
every R; the fp16 bulk mode's producer ("f16x2/64 one plane": fp32 sums to the slot) is recorded, never asserted -- its class is the
reference's autocast (test_hip_fp16_mode.py)."""
import math
import os

import pytest
import torch

import gn_dc_cases as D
import test_hip_conv_engine_paths as E
from conftest import rnd

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(os.environ.get("R2DM_CONV_ALGO", "").startswith("f"), reason="fp32-MFMA algorithm forced")]
DEV = "cuda"
FP64_PRODUCERS = ("f32 mfma 3x3", "f32 mfma 1x1", "fir_down2_stats", "down_gemm")  # every addition of the statistics is fp64
BULK = "f16x2/64 one plane"


@pytest.fixture(scope="module")
def H():
    import hipops

    return hipops


def check_normalised(H, label, producer, case, R, y, stat):
    """The ladder's assertions on one stored output y (fp32, on the device) and the sink its producer filled."""
    cin, cout, h, w, B, G, cpg = case
    assert y.shape == (B, cout, h, w) and torch.isfinite(stat).all()
    ratio = D.dc_ratio(y.cpu(), G)
    assert ratio.min().item() >= 0.9 * R, f"{label}: |mean| / sigma = {ratio.min().item():.2f} in some group: the case does not carry the DC it claims"
    ref64, ref_err = D.references(y, G)
    aff, st = H.group_norm_from_stats(stat.contiguous(), cout, h, w, D.EPS)
    fused = D.bar(H.affine_act(y, aff, silu=False), ref64, ref_err)
    aff_s, st_s = H.group_norm_affine(y, G, D.EPS)
    stream = D.bar(H.affine_act(y, aff_s, silu=False), ref64, ref_err)
    yd = y.double().cpu().reshape(B, G, -1)
    mean, rstd = yd.mean(-1), 1.0 / (yd.var(-1, unbiased=False) + D.EPS).sqrt()
    e_mean = lambda s: ((s[..., 0].double().cpu() - mean).abs() / yd.std(-1, unbiased=False)).max().item()
    e_rstd = lambda s: (s[..., 1].double().cpu() / rstd - 1).abs().max().item()
    asserted = producer != BULK and (producer in FP64_PRODUCERS or D.asserted(case, R))
    print(f"{label} |mean|/sigma {ratio.min().item():.1f}..{ratio.max().item():.1f}: fused rstd rel {e_rstd(st):.2e} mean/sigma {e_mean(st):.2e} "
          f"max x{fused[1]:.2f} ({fused[3]:.2e}) rms x{fused[2]:.2f} | streaming rstd rel {e_rstd(st_s):.2e} mean/sigma {e_mean(st_s):.2e} "
          f"max x{stream[1]:.2f} ({stream[3]:.2e}) rms x{stream[2]:.2f}" + ("" if asserted else "  [recorded, not asserted]"))
    assert stream[0], f"{label}: streaming statistics miss the bar: max x{stream[1]:.2f}, rms x{stream[2]:.2f}"
    if asserted:
        assert fused[0], f"{label}: fused statistics miss the bar: max x{fused[1]:.2f} ({fused[3]:.2e}), rms x{fused[2]:.2f} ({fused[4]:.2e})"


# ---- the convolution kernels ---------------------------------------------------------------------------------------------------------------
CONV = [pytest.param(v, c, R, id=f"{v.replace(' ', '_')}-{D.case_id(c)}-R{R}") for c in D.CASES for v in E.VARIANTS if E.supports(v, *c[:4]) for R in D.LADDER]
_sigma = {}


@pytest.mark.parametrize("variant,case,R", CONV)
def test_conv_statistics_normalise_under_a_dc_offset(H, variant, case, R):
    """One launch through r2dm_conv2d_ring_ex with a sink: bias and residual carry +-R sigma / sqrt(2) each per group (alternating sign), so
    that (conv + bias + residual) / sqrt(2) carries +-R sigma; sigma from the zero-DC launch of the same kernel size and prologue (once per case)."""
    cin, cout, h, w, B, G, cpg = case
    k = E.VARIANTS[variant][2]
    x, wt, b, res, aff = E.inputs(cin, cout, h, w, B, k)
    pro = E.prologues(variant)[-1]
    kw = dict(aff=aff, prologue=pro, scale=E.INV_SQRT2)
    with E.selected(H, variant):
        if (case, k, pro) not in _sigma:
            _sigma[case, k, pro] = D.dc_per_channel(H.conv2d_ring(x, wt, b, residual=res, **kw).cpu(), 1.0, cpg, G)
        dc = (_sigma[case, k, pro] * (R / math.sqrt(2.0))).float().to(DEV)
        got = H.conv2d_ring_ex(x, wt, b + dc, residual=res + dc[None, :, None, None], stat_groups=G, stat_cpg=cpg, **kw)
    assert E.ran(variant, got.chosen), (variant, got.chosen)
    check_normalised(H, f"{variant} {D.case_id(case)} R={R}", variant, case, R, got.y, got.stat)


# ---- the FIR down-sampler and the down-sampling GEMM ----------------------------------------------------------------------------------------
def fir_supported(C, G, hin, win):
    """fir_down2_stat_slots (resample.hip) != 0."""
    cpg = C // G
    slots = ((hin // 2 + 3) // 4) * ((win // 2 + 63) // 64) * 8
    used = slots // 2 if cpg < 64 else slots
    items = cpg * (hin // 4) * (win // 8)
    return C % G == 0 and win % 8 == 0 and hin % 4 == 0 and cpg in (8, 16, 32, 64) and used >= 4 and used % 4 == 0 and items % used == 0 \
        and (items // used) % 64 == 0 and items // used <= 1024


def gemm_supported(cin, cout, G, hin, win):
    """r2dm_down_gemm_stat_slots (kernel_abi.hip) != 0."""
    return cin % 32 == 0 and cout % 64 == 0 and hin % 8 == 0 and win % 128 == 0 and cout % G == 0 and cout // G in (8, 16, 32, 64)


def test_support_rules_match_the_library():
    """The two rules above pick the parametrisation without a GPU: they must be the library's (and every case must have both producers)."""
    from r2dm_amd import _lib

    L = _lib.lib()
    for cin, cout, h, w, B, G, cpg in D.CASES:
        assert fir_supported(cout, G, 2 * h, 2 * w) and L.r2dm_fir_down2_stat_slots(cout, G, 2 * h, 2 * w) != 0
        assert gemm_supported(cin, cout, G, 2 * h, 2 * w) and L.r2dm_down_gemm_stat_slots(cin, cout, G, 2 * h, 2 * w) != 0
    assert not fir_supported(64, 8, 8, 64) and L.r2dm_fir_down2_stat_slots(64, 8, 8, 64) == 0


FIR = [pytest.param(c, R, id=f"{D.case_id(c)}-R{R}") for c in D.CASES if fir_supported(c[1], c[5], 2 * c[2], 2 * c[3]) for R in D.LADDER]
GEMM = [pytest.param(c, R, id=f"{D.case_id(c)}-R{R}") for c in D.CASES if gemm_supported(c[0], c[1], c[5], 2 * c[2], 2 * c[3]) for R in D.LADDER]


@pytest.mark.parametrize("case,R", FIR)
def test_fir_down_statistics_normalise_under_a_dc_offset(H, case, R):
    """fir_down2_stats_kernel on a (B, Cout, 2 H, 2 W) input whose groups carry +-R sigma u[row]: u undoes the 7/8 the zero-padded window
    leaves of a constant on the first and last output row (gn_dc_cases.fir_row_profile), so the OUTPUT carries +-R sigma; sigma from the
    zero-DC launch."""
    cin, cout, h, w, B, G, cpg = case
    x0 = rnd(40 + D.CASES.index(case), B, cout, 2 * h, 2 * w).to(DEV)
    if ("fir", case) not in _sigma:
        _sigma["fir", case] = D.dc_per_channel(H.fir_down2_stats(x0, G)[0].cpu(), 1.0, cpg, G)
    field = (_sigma["fir", case] * R)[:, None] * D.fir_row_profile(2 * h)[None, :]  # (Cout, 2 H)
    y, stat = H.fir_down2_stats(x0 + field.float().to(DEV)[None, :, :, None], G)
    check_normalised(H, f"fir_down2_stats {D.case_id(case)} R={R}", "fir_down2_stats", case, R, y, stat)


@pytest.mark.parametrize("case,R", GEMM)
def test_down_gemm_statistics_normalise_under_a_dc_offset(H, case, R):
    """r2dm_down_gemm = Resample(down=2)(Conv3x3(x) + bias): the bias goes through the zero-padded window (7/8 on the border rows), so the DC
    rides on an input channel instead -- channel 0 holds u[row] (constant along the circular columns) and reaches output channel o through
    its centre tap alone, w[o, 0, 1, 1] = +-R sigma: FIR(w u) = w on every output row."""
    from test_hip_down_gemm import down_gemm

    cin, cout, h, w, B, G, cpg = case
    i = D.CASES.index(case)
    x = rnd(50 + i, B, cin, 2 * h, 2 * w)
    x[:, 0] = D.fir_row_profile(2 * h).float()[None, :, None]
    wt, b = rnd(60 + i, cout, cin, 3, 3) / math.sqrt(9 * cin), rnd(70 + i, cout)
    wt[:, 0] = 0
    x, wt, b = x.to(DEV), wt.to(DEV), b.to(DEV)
    if ("gemm", case) not in _sigma:
        _sigma["gemm", case] = D.dc_per_channel(down_gemm(x, wt, b, groups=G)[0].cpu(), 1.0, cpg, G)
    wt[:, 0, 1, 1] = (_sigma["gemm", case] * R).float().to(DEV)
    y, stat = down_gemm(x, wt, b, groups=G)
    check_normalised(H, f"down_gemm {D.case_id(case)} R={R}", "down_gemm", case, R, y, stat)


# ---- end to end: a checkpoint whose residual stream carries a DC component -----------------------------------------------------------------
RES = (32, 256)  # three levels run conv_f16x2.hip with fused statistics at this size (test_hip_unet.py: test_second_golden_resolution_32x256)
CONDS = (-15.0, 0.0, 6.0)
_dc = {}


def group_norm_ratios(O, sd, cfg, x, cond):
    """Largest per-group |mean| / sigma of the input of every GroupNorm of one oracle forward, in call order (the oracle's blocks call
    group_norm through the module global)."""
    seen, inner = [], O.group_norm

    def recording(t, groups, eps, w, b):
        seen.append(D.dc_ratio(t, groups).max().item())
        return inner(t, groups, eps, w, b)

    O.group_norm = recording
    try:
        O.unet_forward(sd, cfg, x, cond)
    finally:
        O.group_norm = inner
    return seen


def dc_checkpoint(R):
    """(checkpoint, c, median over the GroupNorm calls of the largest group ratio): synthetic_ckpt(32 x 256) with +-c per group (alternating
    sign) added to conv1.bias and conv2.bias of every residual block; c = 0 for R = 0, else the first of 1/4, 1/2, 1, 2, ... at which the
    median is >= R / 2 on the test's own input at log-SNR 0."""
    from oracle import r2dm_oracle as O
    from conftest import synthetic_ckpt

    if R in _dc:
        return _dc[R]
    base = synthetic_ckpt(resolution=RES)
    cfg = O.UNetConfig(resolution=RES)
    x, cond = rnd(81, 2, 2, *RES).double().to(DEV), torch.zeros(2, dtype=torch.float64, device=DEV)

    def edited(c):
        ck = dict(base)
        w = ck["ema_weights"] = dict(base["ema_weights"])
        for k in [k for k in w if k.endswith(("conv1.bias", "conv2.bias")) and "residual_blocks" in k]:
            w[k] = w[k] + (D.per_channel(D.signs(D.GROUPS), w[k].numel() // D.GROUPS) * c).to(w[k])
        return ck

    def median(ck):
        sd = {k: v.double().to(DEV) for k, v in O.strip_prefix(ck["ema_weights"]).items()}
        return torch.tensor(group_norm_ratios(O, sd, cfg, x, cond)).median().item()

    c = 0.0 if R == 0 else 0.25
    ck = edited(c)
    m = median(ck)
    while m < R / 2:
        assert c < 1e4, f"no bias offset reaches a median group ratio of {R / 2}: {m:.2f} at c = {c}"
        c *= 2
        ck = edited(c)
        m = median(ck)
    _dc[R] = (ck, c, m)
    return _dc[R]


@pytest.mark.parametrize("R", [0, 16])
def test_unet_forward_parity_on_a_checkpoint_with_a_dc_component(R):
    """The whole denoiser at 32 x 256, batch 2, log-SNR -15, 0 and 6, both parity modes, against the oracle in fp64 on this GPU: max error <=
    4 x and rms error <= 2 x the error of the oracle in fp32 on the same device (whose GroupNorm subtracts the mean before it squares).  The
    checkpoint carries the DC it claims: the median over the GroupNorm inputs of the largest group ratio is >= R / 2."""
    import r2dm_amd
    from oracle import r2dm_oracle as O

    ck, c, med = dc_checkpoint(R)
    assert med >= R / 2
    cfg = O.UNetConfig(resolution=RES)
    sd = O.strip_prefix(ck["ema_weights"])
    sd64, sd32 = {k: v.double().to(DEV) for k, v in sd.items()}, {k: v.float().to(DEV) for k, v in sd.items()}
    x = rnd(81, 2, 2, *RES)
    ddpm, _, _ = r2dm_amd.setup_model(ck, device=DEV, show_info=False)
    print(f"R={R}: bias offset c = {c}, median over the GroupNorm inputs of the largest |mean|/sigma = {med:.1f}")
    failures = []
    for cv in CONDS:
        cond = torch.full((2,), cv)
        ref64 = O.unet_forward(sd64, cfg, x.double().to(DEV), cond.double().to(DEV))
        e32 = O.unet_forward(sd32, cfg, x.to(DEV), cond.to(DEV)).double() - ref64
        rmax, rrms = e32.abs().max().item(), e32.pow(2).mean().sqrt().item()
        for mode in ("fp32", "fp32-bf16x3"):
            ddpm.model.set_precision(mode)
            e = ddpm.model(x.to(DEV), cond.to(DEV)).double() - ref64
            emax, erms = e.abs().max().item(), e.pow(2).mean().sqrt().item()
            print(f"  R={R} log-SNR {cv:5.1f} {mode:11s}: max {emax:.2e} (x{emax / rmax:.2f}) rms {erms:.2e} (x{erms / rrms:.2f}) | fp32 oracle max {rmax:.2e} rms {rrms:.2e}")
            if not (emax <= D.MAX_FACTOR * rmax and erms <= D.RMS_FACTOR * rrms):
                failures.append((cv, mode, emax / rmax, erms / rrms))
        ddpm.model.set_precision("fp32")
    assert not failures, failures


def test_group_norm_fold_is_bit_identical_on_a_dc_checkpoint():
    """test_group_norm_folded_into_its_consumer_is_bit_identical on data whose group means are 8 sigma and more: the consumer-side fold and
    the separate finalize launch still agree bit for bit."""
    import r2dm_amd
    from hipops import env

    ck, _, _ = dc_checkpoint(16)
    x, cond = rnd(82, 2, 2, *RES).to(DEV), torch.tensor([-3.0, 4.0], device=DEV)
    outs = {}
    for mode in ("1", "0"):
        with env(R2DM_GN_FOLD=mode):
            m, _, _ = r2dm_amd.setup_model(ck, device=DEV, show_info=False)
            outs[mode] = (m.model(x, cond).clone(), m.model(x, cond).clone())
            del m
    assert torch.equal(outs["1"][0], outs["1"][1]) and torch.equal(outs["0"][0], outs["0"][1])
    assert torch.equal(outs["1"][0], outs["0"][0])

