"""-m gpu: the down path's operand with every distinct plane stored once (resample.hip down_planes_phase_kernel) and the loader mode of the down-sampling GEMM
that maps the nine taps onto it (proj_f16x2.hip, PHP) -- bit for bit against the nine-plane pair they replace.

    kx = 0 reads the kx = 2 plane one column to the left (circular); kx = 1 is the second column phase
    V[2][i] = V[0][i + 1] for 1 <= i <= Ho - 3; V[2][0], V[2][Ho - 2], V[2][Ho - 1] are stored on their own
    layout per sample: [phase (kx = 2 | kx = 1)][C][Ho rows V[0] | Ho rows V[1] | 3 rows][Wo + 4]; column j at float 4 + j, float 3 of phase 0 = column Wo - 1
"""
import math

import pytest
import torch

from conftest import rnd, synthetic_ckpt

pytestmark = pytest.mark.gpu
DEV = "cuda"


def nine_planes(x):
    from r2dm_amd import _lib

    B, C, H, W = x.shape
    a = torch.full((B, 9 * C, H // 2, W // 2), float("nan"), device=x.device)
    _lib.check(_lib.lib().r2dm_down_planes(x.data_ptr(), a.data_ptr(), B, C, H, W, _lib.stream_ptr(x.device)))
    torch.cuda.synchronize()
    return a


def phase_planes(x):
    """(B, 2, C, H + 3, W / 2 + 4), written into a NaN-filled destination of exactly the size the query reports."""
    from r2dm_amd import _lib

    L = _lib.lib()
    B, C, H, W = x.shape
    n = L.r2dm_down_phase_planes_floats(C, H, W)
    assert n == 2 * C * (H + 3) * (W // 2 + 4)
    a = torch.full((B, n), float("nan"), device=x.device)
    _lib.check(L.r2dm_down_phase_planes(x.data_ptr(), a.data_ptr(), B, C, H, W, _lib.stream_ptr(x.device)))
    torch.cuda.synchronize()
    return a.view(B, 2, C, H + 3, W // 2 + 4)


def phase_row(ky, i, Ho):
    if ky == 0:
        return i
    if ky == 1:
        return Ho + i
    if i == 0:
        return 2 * Ho
    if i == Ho - 1:
        return 2 * Ho + 2
    if i == Ho - 2:
        return 2 * Ho + 1
    return i + 1


def expand(pp):
    """The nine planes (B, 9 C, Ho, Wo) read out of the phase layout the way the GEMM's loader reads them."""
    B, _, C, R, P = pp.shape
    Ho, Wo = (R - 3) // 2, P - 4
    out = []
    for ky in range(3):
        rows = torch.tensor([phase_row(ky, i, Ho) for i in range(Ho)], device=pp.device)
        for kx in range(3):
            c0 = 4 - (1 if kx == 0 else 0)
            out.append(pp[:, 1 if kx == 1 else 0].index_select(2, rows)[..., c0:c0 + Wo])
    return torch.cat(out, 1)


@pytest.mark.parametrize("B,C,h,w", [(2, 32, 8, 128),    # Ho = 4: one shared row (V[2][1] = V[0][2]) and all three special rows
                                     (1, 32, 16, 128),   # shared rows 2 .. 6
                                     (1, 32, 8, 256)])   # two tile columns of the GEMM
def test_phase_planes_expand_to_the_nine_planes(B, C, h, w):
    x = (rnd(90, B, C, h, w) * 1.3 + 0.2).to(DEV)
    pp = phase_planes(x)
    got = expand(pp)
    assert torch.isfinite(got).all()  # everything the GEMM reads was written
    assert torch.equal(got, nine_planes(x))
    assert torch.equal(pp.view(torch.int32), phase_planes(x).view(torch.int32))  # (as bits: the unwritten floats are NaN)
    # nothing else is written: floats 0 .. 2 of every row and float 3 of the second phase keep the fill
    assert torch.isnan(pp[..., :3]).all() and torch.isnan(pp[:, 1, :, :, 3]).all()
    assert torch.isfinite(pp[..., 4:]).all() and torch.isfinite(pp[:, 0, :, :, 3]).all()


def down_gemm(entry, x, w, b, groups=0):
    from r2dm_amd import _lib

    L = _lib.lib()
    B, cin, H, W = x.shape
    cout = w.shape[0]
    packed = torch.empty(9 * cin * cout + 64, device=x.device)
    planes = torch.full((B * 9 * cin * (H // 2) * (W // 2),), float("nan"), device=x.device)
    y = torch.full((B, cout, H // 2, W // 2), float("nan"), device=x.device)
    stat = None
    if groups:
        slots = L.r2dm_down_gemm_stat_slots(cin, cout, groups, H, W)
        assert slots > 0
        stat = torch.full((B, groups, slots, 2), float("nan"), device=x.device, dtype=torch.float64)
    _lib.check(getattr(L, entry)(x.data_ptr(), w.data_ptr(), b.data_ptr(), packed.data_ptr(), planes.data_ptr(), y.data_ptr(), _lib.ptr(stat),
                                 B, cin, cout, groups, H, W, _lib.stream_ptr(x.device)))
    torch.cuda.synchronize()
    return y, stat


@pytest.mark.parametrize("B,cin,cout,h,w", [(2, 32, 64, 8, 128),     # 64-channel tiles, the azimuth seam in every tile
                                            (1, 32, 64, 8, 256),     # an interior tile boundary
                                            (1, 64, 256, 16, 128),   # 256-channel blocks, shared rows 2 .. 6
                                            (1, 64, 512, 8, 128)])
def test_down_gemm_over_phase_planes_is_the_nine_plane_product(B, cin, cout, h, w):
    x, wt, b = (rnd(91, B, cin, h, w) * 1.7 + 0.3).to(DEV), (rnd(92, cout, cin, 3, 3) / math.sqrt(9 * cin)).to(DEV), rnd(93, cout).to(DEV)
    for groups in (0, 8):
        y1, s1 = down_gemm("r2dm_down_gemm", x, wt, b, groups)
        y9, s9 = down_gemm("r2dm_down_gemm_nine", x, wt, b, groups)
        assert torch.isfinite(y9).all()
        assert torch.equal(y1, y9), groups
        if groups:
            assert torch.isfinite(s9).all()
            assert torch.equal(s1, s9)


def _model(switch, resolution):
    import hipops
    import r2dm_amd

    with hipops.env(R2DM_DOWN_GEMM=switch):
        ddpm, _, _ = r2dm_amd.setup_model(synthetic_ckpt(resolution=resolution), device=DEV, show_info=False)
        ddpm.model(torch.zeros(1, 2, *resolution, device=DEV), torch.zeros(1, device=DEV))  # (the engine exists now)
    return ddpm.model


@pytest.fixture(scope="module")
def engines():
    return {s: _model(s, (32, 512)) for s in ("1", "9")}


@pytest.mark.parametrize("B", [1, 3])
def test_engine_phase_planes_and_nine_planes_agree(engines, B):
    """32 x 512: all three down stages take the GEMM.  The two settings give the same bits, each repeats bit for bit, and both run the pre-pass three times."""
    x, c = rnd(94, 3, 2, 32, 512)[:B].to(DEV), torch.tensor([-9.0, 0.5, 6.0])[:B].to(DEV)
    out = {}
    for s, net in engines.items():
        out[s] = net(x, c)
        assert torch.equal(out[s], net(x, c)), s
        launches = [ln.split(" | ")[1] for ln in net._engine.listing(B).splitlines()]
        assert launches.count("down_gemm") == 3, s
        # ... and each its own: the forward's listing says which layout the engine writes, so a switch that was ignored cannot pass as agreement
        assert launches.count("down_phase_planes") == (3 if s == "1" else 0), s
        assert launches.count("down_planes") == (3 if s == "9" else 0), s
    assert torch.isfinite(out["9"]).all()
    assert torch.equal(out["1"], out["9"])
