"""-m gpu: the down path with the FIR in front of the convolution (resample.hip down_planes_kernel + the down-sampling GEMM of
proj_f16x2.hip) -- kernel by kernel against fp64, and through the engine with the switch R2DM_DOWN_GEMM on and off.

    V[ky][i][c]     = sum_t f[t] [0 <= 2i-1+t < H] x[2i-1+t + ky-1][c]         f = [1,3,3,1]/8, x zero outside rows [0, H)
    A[ky][kx][i][j] = sum_t f[t] V[ky][i][(2j + t + kx - 2) mod W]
    FIR(conv(x) + b)[co][i][j] = sum_{ky,kx,ci} w[co][ci][ky][kx] A[ky][kx][ci][i][j] + b[co] rowfac[i]
"""
import math

import pytest
import torch

from conftest import GOLDEN_RES, max_abs, rnd, synthetic_ckpt
from hipops import down_gemm, down_planes  # the ctypes wrappers of the two standalone entry points

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def O():
    from oracle import r2dm_oracle

    return r2dm_oracle


def planes_fp64(x):
    """The formula of the module docstring, term by term, in float64 on the CPU."""
    x = x.double()
    B, C, H, W = x.shape
    f = [0.125, 0.375, 0.375, 0.125]
    xz = torch.zeros(B, C, H + 6, W, dtype=torch.float64)  # row r of x at xz[r + 3]
    xz[:, :, 3:H + 3] = x
    A = torch.zeros(B, 3, 3, C, H // 2, W // 2, dtype=torch.float64)
    cols = torch.arange(W // 2) * 2
    for ky in range(3):
        V = torch.zeros(B, C, H // 2, W, dtype=torch.float64)
        for i in range(H // 2):
            for t in range(4):
                if 0 <= 2 * i - 1 + t < H:
                    V[:, :, i] += f[t] * xz[:, :, 2 * i - 1 + t + ky - 1 + 3]
        for kx in range(3):
            for t in range(4):
                A[:, ky, kx] += f[t] * V[..., (cols + t + kx - 2) % W]
    return A.reshape(B, 9 * C, H // 2, W // 2)


def test_down_planes_match_the_formula_in_fp64(O):
    """B = 2, 32 channels, 8 x 128: four output rows -- both border rows and two interior ones.  The bar of the FIR kernels (1e-6 on O(1) data), the border
    rows on their own; and the planes ARE the operand of the composition: contracted with the weights in fp64 they give Resample(down=2)(Conv3x3(x))."""
    x = rnd(70, 2, 32, 8, 128)
    want = planes_fp64(x)
    a = down_planes(x.to(DEV))
    assert torch.equal(a, down_planes(x.to(DEV)))
    got = a.cpu()
    Ho = want.shape[2]
    for name, rows in (("row 0", slice(0, 1)), ("last row", slice(Ho - 1, Ho)), ("interior", slice(1, Ho - 1))):
        e = max_abs(got[:, :, rows], want[:, :, rows])
        print(f"down_planes {name}: max|err| {e:.2e}")
        assert e < 1e-6, name
    w, b = rnd(71, 7, 32, 3, 3).double(), rnd(72, 7).double()
    wk = w.permute(0, 2, 3, 1).reshape(7, 9 * 32)  # [co][(ky, kx, ci)]
    rowfac = torch.ones(Ho, dtype=torch.float64)
    rowfac[0] = rowfac[-1] = 7.0 / 8.0
    z = torch.einsum("ok,bkij->boij", wk, want) + b[None, :, None, None] * rowfac[None, None, :, None]
    assert max_abs(z, O.fir_down2(O.conv_ring(x.double(), w, b))) < 1e-12


@pytest.mark.parametrize("B,cin,cout,h,w", [(2, 32, 64, 8, 128),      # one tile row, the 64-channel tiles
                                            (1, 64, 256, 16, 128)])  # two tile rows, the 256-channel blocks
def test_down_gemm_against_fp64(O, B, cin, cout, h, w):
    """The rule of test_conv3x3_both_operand_splits: the rms error against fp64 is no larger than that of the same composition evaluated by the oracle in fp32
    on the CPU -- over the whole output, and over the two border rows on their own (where the bias takes the factor 7/8)."""
    import hipops

    x, wt, b = rnd(73, B, cin, h, w), rnd(74, cout, cin, 3, 3) / math.sqrt(9 * cin), rnd(75, cout)
    ref = O.fir_down2(O.conv_ring(x.double(), wt.double(), b.double()))
    f32 = O.fir_down2(O.conv_ring(x, wt, b))
    y, _ = down_gemm(x.to(DEV), wt.to(DEV), b.to(DEV))
    assert torch.equal(y, down_gemm(x.to(DEV), wt.to(DEV), b.to(DEV))[0])
    old = hipops.fir_down2(hipops.conv2d_ring(x.to(DEV), wt.to(DEV), b.to(DEV)))  # conv + FIR through the existing entry points: for the record
    rms = lambda a, rows: (a.double().cpu()[:, :, rows] - ref[:, :, rows]).pow(2).mean().sqrt().item()
    border = [0, h // 2 - 1]
    whole = slice(None)
    print(f"down_gemm {cin}->{cout} {h}x{w}: rms vs fp64 -- new {rms(y, whole):.3e} (border rows {rms(y, border):.3e}) | fp32 oracle {rms(f32, whole):.3e} "
          f"(border {rms(f32, border):.3e}) | conv + FIR kernels {rms(old, whole):.3e} (border {rms(old, border):.3e}); "
          f"ratio new / fp32 oracle {rms(y, whole) / rms(f32, whole):.2f} (border {rms(y, border) / rms(f32, border):.2f}); max|err| {max_abs(y.cpu(), ref):.2e}")
    assert rms(y, whole) <= rms(f32, whole)
    assert rms(y, border) <= rms(f32, border)


@pytest.mark.parametrize("B,cin,cout,h,w", [(2, 32, 64, 8, 128), (1, 64, 256, 16, 128), (1, 64, 512, 8, 128)])
def test_down_gemm_statistics_slots(B, cin, cout, h, w):
    """The slots, reduced in fp64, are the moments of the STORED output of every (sample, group): the bar of test_fir_down_with_fused_group_norm_statistics
    (rel. 1e-12), every slot written, the second half of the grid zero for groups of fewer than 64 channels, a slot's energy a bound on its elements."""
    x, wt, b = rnd(76, B, cin, h, w) * 1.7 + 0.3, rnd(77, cout, cin, 3, 3) / math.sqrt(9 * cin), rnd(78, cout)
    y, stat = down_gemm(x.to(DEV), wt.to(DEV), b.to(DEV), groups=8)
    assert torch.equal(y, down_gemm(x.to(DEV), wt.to(DEV), b.to(DEV))[0])  # the same output with and without the statistics
    assert torch.isfinite(stat).all()
    yd = y.double().reshape(B, 8, -1)
    want_s, want_q = yd.sum(-1), (yd * yd).sum(-1)
    got = stat.sum(2)
    assert ((got[..., 0] - want_s).abs() <= 1e-12 * yd.abs().sum(-1)).all()
    assert ((got[..., 1] - want_q).abs() <= 1e-12 * want_q).all()
    n = yd.shape[-1]
    mean, var = got[..., 0] / n, got[..., 1] / n - (got[..., 0] / n) ** 2
    # (what the two bars above leave of the mean and of E[y^2] - mean^2)
    assert ((mean - yd.mean(-1)).abs() <= 1e-12 * yd.abs().mean(-1)).all()
    assert ((var - yd.var(-1, unbiased=False)).abs() <= 4e-12 * got[..., 1] / n).all()
    if cout // 8 < 64:
        assert (stat[:, :, stat.shape[2] // 2:] == 0).all()
    assert (stat[..., 1].amax(2).sqrt() >= yd.abs().amax(-1)).all()


# ---- engine --------------------------------------------------------------------------------------------------------------------
def _model(switch, resolution):
    """A model whose engine was created with R2DM_DOWN_GEMM = switch (the library reads it once, at r2dm_create)."""
    import hipops
    import r2dm_amd

    with hipops.env(R2DM_DOWN_GEMM=switch):
        ddpm, _, _ = r2dm_amd.setup_model(synthetic_ckpt(resolution=resolution), device=DEV, show_info=False)
        ddpm.model(torch.zeros(1, 2, *resolution, device=DEV), torch.zeros(1, device=DEV))  # (the engine exists now)
    return ddpm.model


@pytest.fixture(scope="module")
def engines():
    return {s: _model(s, (32, 512)) for s in ("1", "0")}


@pytest.fixture(scope="module")
def truth(O):
    """fp64 oracle outputs at 32 x 512 for the three samples the engine tests use (computed once)."""
    sd = {k: v.double().to(DEV) for k, v in O.strip_prefix(synthetic_ckpt(resolution=(32, 512))["ema_weights"]).items()}
    x, c = rnd(79, 3, 2, 32, 512), torch.tensor([-9.0, 0.5, 6.0])
    return x, c, O.unet_forward(sd, O.UNetConfig(resolution=(32, 512)), x.double().to(DEV), c.double().to(DEV)).cpu()


@pytest.mark.parametrize("B", [1, 3])
def test_engine_down_gemm_on_and_off_vs_oracle(engines, truth, B):
    """32 x 512: the smallest resolution at which all three down stages fit the GEMM's tiles.  Both settings stay under the bar test_unet_full_size_vs_oracle
    asserts against the fp64 oracle, each repeats bit for bit, and a sample's bits do not depend on the batch it is part of."""
    x, c, ref = truth
    out = {}
    for s, net in engines.items():
        y = net(x[:B].to(DEV), c[:B].to(DEV))
        assert torch.equal(y, net(x[:B].to(DEV), c[:B].to(DEV))), s
        assert torch.equal(y[:1], net(x[:1].to(DEV), c[:1].to(DEV))), s
        out[s] = y.cpu()
    e = {s: max_abs(y, ref[:B]) for s, y in out.items()}
    print(f"unet 32x512 B={B}: max|hip - fp64 oracle| on {e['1']:.2e} off {e['0']:.2e}; max|on - off| {max_abs(out['1'], out['0']):.2e}")
    assert not torch.equal(out["1"], out["0"])  # the switch took effect
    assert e["1"] < 8e-6 and e["0"] < 8e-6, e


def test_engine_precision_switch_both_directions(engines, truth):
    """set_precision at run time: the exact three-piece split keeps conv + FIR (the same bits whatever the switch was at creation), and the default
    precision comes back to the bits it gave before."""
    from r2dm_amd import _lib

    x, c, _ = truth
    xd, cd = x[:1].to(DEV), c[:1].to(DEV)
    y2 = {s: net(xd, cd) for s, net in engines.items()}
    y3 = {}
    for s, net in engines.items():
        h = net._engine.h
        _lib.check(_lib.lib().r2dm_set_conv_pieces(h, 3))
        try:
            y3[s] = net(xd, cd)
        finally:
            _lib.check(_lib.lib().r2dm_set_conv_pieces(h, 2))
        assert torch.equal(net(xd, cd), y2[s]), s
    assert torch.equal(y3["1"], y3["0"])


def _down_stages_on_the_gemm(net, B):
    """How many down stages of a forward at batch B run the FIR pre-pass + GEMM pair (the engine's listing of its launches)."""
    launches = [ln.split(" | ")[1] for ln in net._engine.listing(B).splitlines()]
    assert launches.count("down_phase_planes") == launches.count("down_gemm") and "down_planes" not in launches
    assert launches.count("down_gemm") + launches.count("fir_down2") == 3
    return launches.count("down_gemm")


def test_all_three_down_stages_take_the_gemm_at_32x512(engines, truth):
    x, c, _ = truth
    for s, want in (("1", 3), ("0", 0)):
        engines[s](x[:1].to(DEV), c[:1].to(DEV))
        assert _down_stages_on_the_gemm(engines[s], 1) == want, s


def test_golden_resolution_keeps_conv_and_fir(golden):
    """At the golden resolution (16 x 128) only d_block2's output (8 x 64) fits the GEMM's tiles, so the plan packs its matrix; what keeps conv + FIR there is the
    range tracking: d_block1's last convolution has too few tiles at this size for the fp16-operand kernel and records no max|output|, so the stage's input is
    not tracked.  Asserted on the range sites (no pre-pass ran), on the bits (those of the switch off) and on the golden vectors of test_unet_golden."""
    g = golden("unet")
    on, off = _model("1", GOLDEN_RES), _model("0", GOLDEN_RES)
    x = g["x"].to(DEV)
    for i, c in enumerate(g["conds"].tolist()):
        cond = torch.full((2,), c, device=DEV)
        y = on(x, cond)
        assert _down_stages_on_the_gemm(on, 2) == 0
        assert torch.equal(y, off(x, cond))
        assert max_abs(y.cpu(), g["y"][i]) < 2e-5, c
