"""The forward's listing (r2dm_forward_listing, the sizing walk) against what a real forward enqueues: the launches per profiling class and the
range sites, in order.  32 x 256 at max_batch 8 is the smallest geometry at which the level-1 layers still take conv_f16x2 and levels 3-4 do not
(conv_f16x2 needs (px_batch / 256) (cout / 64) >= 128), so both 3x3 kernels, the fused and the streaming GroupNorm are in one walk.
(What the listing says for every geometry, mode and switch: tests/test_forward_listing_cpu.py.)"""
import ctypes
import re

import pytest
import torch

from conftest import rnd, synthetic_ckpt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RES = (32, 256)


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("B", [2, 8])
def test_a_real_forward_enqueues_what_the_listing_says(precision, B):
    import r2dm_amd
    from r2dm_amd import _lib

    ddpm, _, _ = r2dm_amd.setup_model(synthetic_ckpt(resolution=RES), device=DEV, show_info=False, max_batch=8, precision=precision)
    net = ddpm.model
    x, c = rnd(97, B, 2, *RES).to(DEV), torch.linspace(-4.0, 4.0, B).to(DEV)
    net(x, c)  # (the engine exists now; the one-off constant map of in_conv is behind us)
    lines = net._engine.listing(B).splitlines()
    net.profile_convs(True)
    try:
        y = net(x, c)
        got = [n for _, _, _, n in net.read_conv_profile_classes()]
    finally:
        net.profile_convs(False)
    assert torch.isfinite(y).all()
    want = [sum(f" class={k}" in ln for ln in lines) for k in range(3)]
    print(f"{precision} B={B}: launches per class {got}, listing {want}; {len(lines)} launches listed")
    assert got == want
    assert want[0] > 0 and want[1] > 0 and want[2] > 0  # level 1 on conv_f16x2, levels 3-4 on the bf16x3 kernel, the 1x1 / in / out convolutions
    sites = [(ln.split(" | ")[0], int(k), what) for ln in lines for k, what in re.findall(r' site=(\d+):"([^"]*)"', ln)]
    assert [k for _, k, _ in sites] == list(range(1, len(sites) + 1)) and len(sites) > 20
    L = _lib.lib()
    for layer, k, what in sites:
        assert L.r2dm_range_site_name(net._engine.h, k).decode() == f"{layer}: {what}", k
    # ... and the real walk handed out no more than those (a fresh engine: no names left from another walk)
    assert L.r2dm_range_site_name(net._engine.h, len(sites) + 1) == b""
    n = ctypes.c_int32(0)
    _lib.check(L.r2dm_range_sites(net._engine.h, None, 0, ctypes.byref(n)))  # (the forward above checked the range: that read the sites)
    assert n.value == len(sites) + 1  # (+ the shared slot 0)
