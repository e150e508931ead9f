"""Which kernel every layer of a forward dispatches to (r2dm_forward_listing: the sizing walk's launches, host only), against the record in
tests/golden/forward_listing.json.  A pull request that changes dispatch on purpose regenerates the fixture
(python tests/golden/make_forward_listing.py) and moves the numbers below; anything else must leave every listing byte-identical."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location("make_forward_listing", os.path.join(GOLDEN, "make_forward_listing.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(M.FIXTURE))["cases"]


@pytest.fixture(scope="module")
def regenerated():
    return M.generate()["cases"]


def test_the_fixture_covers_every_geometry_mode_and_switch(fixture):
    want = {M.case_name(res, mb, b, mode) for res, mb, b in M.GEOMETRIES for mode in M.MODES}
    want |= {M.case_name(M.DEFAULT, 8, 8, mode, sw) for sw in M.SWITCHES for mode in M.MODES}
    assert set(fixture) == want and len(want) == 3 * (10 + 9)
    for mode in M.MODES:
        assert "listing" in fixture[M.case_name(M.DEFAULT, 8, 8, mode)]


def test_every_listing_is_the_recorded_one(fixture, regenerated):
    assert set(regenerated) == set(fixture)
    for name in sorted(fixture):
        got, want = regenerated[name], fixture[name]
        if "listing" in want and got["listing"] != want["listing"]:  # (the first differing launch says more than two hashes)
            diff = [(a, b) for a, b in zip(got["listing"], want["listing"]) if a != b]
            assert not diff, (name, diff[0])
        assert got == want, (name, {k: (got[k], want[k]) for k in want if k != "listing" and got[k] != want[k]})


def test_every_line_names_its_layer_launch_and_output(fixture):
    launches = {"time_embedding", "ada_proj", "in_conv constant map", "group_norm", "group_norm_finalize", "conv", "attention", "fir_down2",
                "fir_up2", "down_planes", "down_phase_planes", "down_gemm"}
    for mode in M.MODES:
        lines = fixture[M.case_name(M.DEFAULT, 8, 8, mode)]["listing"]
        sites = []
        for ln in lines:
            f = ln.split(" | ")
            assert len(f) >= 3 and f[1] in launches and f[2].startswith("out="), ln
            if f[1] in ("conv", "down_gemm", "in_conv constant map"):
                assert f[3].startswith("algo=") and " tile=" in f[3] and " cin=" in f[3], ln
            sites += [int(s.split(":")[0]) for s in ln.split(" site=")[1:]]
        assert lines[0].split(" | ")[1] == "time_embedding" and lines[-1].startswith("out_conv | conv | out=dst")
        assert sum("first forward after a bind only" in ln for ln in lines) == 1
        assert sites == list(range(1, len(sites) + 1))  # handed out in walk order; mode 3 guards nothing
        assert (len(sites) == 0) == (mode == 3)


def test_the_listing_leaves_the_handle_as_it_was():
    """No site names, no cached workspace size, the same text twice; a short buffer gets a truncated, terminated copy and the full size."""
    import ctypes

    from r2dm_amd import _lib, synthetic
    from r2dm_amd.unet import _Engine

    L = _lib.lib()
    eng = _Engine(synthetic.geometry_from_cfg(synthetic.default_cfg_dict(resolution=(32, 256))), 3)
    first = eng.listing(3)
    assert all(L.r2dm_range_site_name(eng.h, k) == b"" for k in range(1, 256))
    assert eng.listing(3) == first and eng.listing(1) != first
    need, buf = ctypes.c_size_t(0), ctypes.create_string_buffer(b"\xff" * 40, 40)
    _lib.check(L.r2dm_forward_listing(eng.h, 3, buf, 32, ctypes.byref(need)))
    assert need.value == len(first) + 1 and buf.raw[:32] == first.encode()[:31] + b"\0" and buf.raw[32:] == b"\xff" * 8
    assert L.r2dm_forward_listing(eng.h, 0, None, 0, ctypes.byref(need)) == 1


def test_no_layer_of_the_default_model_runs_on_the_bf16x3_kernel(fixture, regenerated):
    """max_batch 8, the default precision: every 3x3 convolution behind a GroupNorm has tiles enough for conv_f16x2."""
    for b in (1, 2, 4, 8):
        name = M.case_name(M.DEFAULT, 8, b, 2)
        assert regenerated[name]["bf16x3"] == 0 and fixture[name]["bf16x3"] == 0, name
    assert not any(" algo=BF16X3 " in ln for ln in regenerated[M.case_name(M.DEFAULT, 8, 8, 2)]["listing"])


@pytest.mark.parametrize("max_batch,want", [(1, 32), (2, 18), (4, 6)])
def test_small_max_batch_models_run_layers_on_the_slower_kernel(fixture, regenerated, max_batch, want):
    """The small-batch hole as a number: a model planned for fewer than 8 samples has too few tiles per layer for conv_f16x2 at the coarse levels and runs
    those layers on the bf16x3 kernel in the DEFAULT precision.  A dispatch change that closes the hole moves these numbers on purpose."""
    name = M.case_name(M.DEFAULT, max_batch, max_batch, 2)
    assert regenerated[name]["bf16x3"] == fixture[name]["bf16x3"] == want
