"""The feature cache (DeepCache) without a GPU: the C ABI's four entries and their refusals, the cached walks' listings against the plain forward's
(r2dm_forward_listing_cached: host only), the full / shallow step plan the sampling loop uses, what the samplers refuse, and -- with the oracle alone --
that the inputs tests/test_hip_cache.py compares shallow forwards on tell a shallow forward from a full one."""
import ctypes
import functools
import os
import re

import pytest
import torch

from conftest import GOLDEN_RES, ROOT, rnd, synthetic_ckpt

import cache_oracle as CO
from oracle import r2dm_oracle as O
from r2dm_amd import _lib, synthetic
from r2dm_amd.unet import _Engine, step_is_full

ENTRIES = ["r2dm_cache_bytes", "r2dm_unet_forward_cached", "r2dm_forward_listing_cached", "r2dm_cache_store"]
MODES = {"fp32": 2, "fp32-bf16x3": 3, "fp16": 1}
# (resolution, max_batch, batch)
GEOMETRIES = [((64, 1024), 8, 1), ((64, 1024), 8, 8), (GOLDEN_RES, 2, 2)]
DEPTHS = [1, 2, 3]


@functools.lru_cache(maxsize=None)
def engine(res, max_batch):
    return _Engine(synthetic.geometry_from_cfg(synthetic.default_cfg_dict(resolution=res)), max_batch)


def listings(res, max_batch, B, precision, depth):
    """(plain, store, reuse) listings as lists of lines"""
    eng = engine(res, max_batch)
    _lib.check(_lib.lib().r2dm_set_conv_pieces(eng.h, MODES[precision]))
    return eng.listing(B).splitlines(), eng.listing_cached(B, depth, 1).splitlines(), eng.listing_cached(B, depth, 2).splitlines()


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_library_exports_the_four_entries():
    header = open(os.path.join(ROOT, "include", "r2dm_hip.h")).read()
    L = _lib.lib()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name


def test_cache_bytes_holds_the_tensor_and_grows_with_the_batch():
    L = _lib.lib()
    eng = engine((64, 1024), 8)
    for depth, (C, H, W) in zip(DEPTHS, [(64, 64, 1024), (128, 32, 512), (256, 16, 256)]):
        sizes = [int(L.r2dm_cache_bytes(eng.h, B, depth)) for B in (1, 2, 8)]
        assert all(n >= B * C * H * W * 4 and n % 256 == 0 for n, B in zip(sizes, (1, 2, 8))), (depth, sizes)
        assert sizes[0] < sizes[1] < sizes[2]
        assert eng.cached_tensor(2, depth) == ((C, H, W), torch.float32)
    assert L.r2dm_cache_bytes(eng.h, 1, 0) == 0 and L.r2dm_cache_bytes(eng.h, 1, 4) == 0 and L.r2dm_cache_bytes(eng.h, 0, 1) == 0


def test_the_entries_refuse_by_status_and_message():
    """Every refusal comes before anything is read or enqueued: the pointers here are never dereferenced."""
    L = _lib.lib()
    eng = engine(GOLDEN_RES, 2)
    need = int(L.r2dm_cache_bytes(eng.h, 2, 1))
    p = 1 << 20  # (a 256-byte aligned address that is not null)

    def fwd(B=2, cache=p, cache_bytes=need, depth=1, mode=1, drift=None):
        rc = L.r2dm_unet_forward_cached(eng.h, p, p, p, B, p, 1 << 30, None, cache, cache_bytes, depth, mode, drift)
        return rc, L.r2dm_last_error().decode()

    for kw, word in [(dict(depth=0), "depth"), (dict(depth=4), "depth"), (dict(mode=0), "mode"), (dict(mode=3), "mode"), (dict(cache_bytes=need - 1), "too small"),
                     (dict(cache=p + 16), "aligned"), (dict(B=3), "max_batch"), (dict(B=0), "batch"), (dict(cache=None), "null")]:
        rc, msg = fwd(**kw)
        assert rc != 0 and word in msg, (kw, rc, msg)
    rc, msg = fwd()  # (everything in order but the weights: this handle has none)
    assert rc != 0 and "weights not loaded" in msg
    n = ctypes.c_size_t(0)
    for B, depth, mode, word in [(2, 0, 1, "depth"), (2, 4, 2, "depth"), (2, 1, 0, "mode"), (2, 1, 3, "mode"), (3, 1, 1, "max_batch"), (0, 1, 1, "batch")]:
        assert L.r2dm_forward_listing_cached(eng.h, B, depth, mode, None, 0, ctypes.byref(n)) != 0 and word in L.r2dm_last_error().decode(), (B, depth, mode)
    assert L.r2dm_forward_listing_cached(eng.h, 2, 1, 1, None, 0, None) != 0
    d = ctypes.c_double(0)

    def store(fresh=p, cached=2 * p, B=2, n=64, f16=0, partial=ctypes.addressof(d), sums=ctypes.addressof(d)):
        rc = L.r2dm_cache_store(fresh, cached, B, n, f16, partial, sums, None)
        return rc, L.r2dm_last_error().decode()

    for kw, word in [(dict(fresh=None), "null"), (dict(sums=None), "null"), (dict(B=0), "batch"), (dict(n=0), "n_per_sample"), (dict(f16=2), "f16"),
                     (dict(cached=p), "same tensor"), (dict(fresh=p + 4), "aligned"), (dict(cached=2 * p + 8), "aligned")]:
        rc, msg = store(**kw)
        assert rc != 0 and word in msg, (kw, rc, msg)


# ---- the listings -------------------------------------------------------------------------------------------------------------------------
CASES = [(res, mb, B, prec, d) for res, mb, B in GEOMETRIES for prec in MODES for d in DEPTHS]


def fields(line):
    return line.split(" | ")


@pytest.mark.parametrize("res,max_batch,B,precision,depth", CASES)
def test_the_store_listing_is_the_forwards_but_for_the_cached_tensors_address(res, max_batch, B, precision, depth):
    plain, store, _ = listings(res, max_batch, B, precision, depth)
    assert len(store) == len(plain)
    differ = [(a, b) for a, b in zip(plain, store) if a != b]
    assert len(differ) == 1, differ
    a, b = (fields(ln) for ln in differ[0])
    assert a[0] == b[0] == f"u_block{depth + 1}.upsample" and a[1] == b[1] == "conv" and b[2] == "out=cache" and a[2] != b[2]
    assert a[3:] == b[3:]  # the same kernel, fusions, range sites and profiling class
    assert sum("out=cache" in ln for ln in store) == 1 and not any("out=cache" in ln for ln in plain)


def normalised(line):
    """a listing line without what a reuse walk may change: where the launch writes, and which way a conv_f16x2 launch walks its tiles"""
    f = fields(line)
    f[2] = "out=*" if f[2] != "out=dst" else f[2]
    if len(f) > 3:
        f[3] = re.sub(r" rev\b", "", f[3])
    return " | ".join(f)


def live_layers(depth):
    names = ["-", "in_conv", "out_conv"] + [f"{side}_block{lv}" for lv in range(1, depth + 1) for side in "du"]
    return lambda line: fields(line)[0].split(".")[0] in names


@pytest.mark.parametrize("res,max_batch,B,precision,depth", CASES)
def test_the_reuse_listing_is_the_forwards_lines_of_the_live_layers(res, max_batch, B, precision, depth):
    plain, _, reuse = listings(res, max_batch, B, precision, depth)
    live = live_layers(depth)
    assert all(live(ln) for ln in reuse), [ln for ln in reuse if not live(ln)][:1]  # no line names a skipped stage
    want = [normalised(ln) for ln in plain if live(ln)]
    # the same layers, launches, ConvParams texts (fold= / stat= in them) and site= labels, in the forward's order: only out= and rev may differ
    assert [normalised(ln) for ln in reuse] == want
    assert 0 < len(reuse) < len(plain) and not any("out=cache" in ln for ln in reuse)
    skipped = {"attention"} if depth < 3 else set()  # (depth 3 keeps d_block3 / u_block3 live: whether they carry attention is the geometry's)
    assert not skipped & {fields(ln)[1] for ln in reuse}
    if precision != "fp32-bf16x3":  # the range sites a shallow walk hands out carry the full walk's numbers: fewer of them, never renumbered
        sites = lambda lines: [s.split(":")[0] for ln in lines for s in ln.split(" site=")[1:]]
        got, full = sites(reuse), sites(plain)
        assert got and len(got) < len(full) and set(got) < set(full) and len(set(got)) == len(got)
        assert [int(s) for s in got] != list(range(1, len(got) + 1))


def test_the_folded_norm_case_of_the_gpu_test_is_one():
    """32 x 512 at batch 2 in the default precision: the first convolution behind the join folds its GroupNorm -- the one that reads the cached statistics."""
    _, _, reuse = listings((32, 512), 2, 2, "fp32", 1)
    line = next(ln for ln in reuse if ln.startswith("u_block1.residual_blocks.0.conv1 | conv"))
    assert " fold=" in line
    _, _, small = listings(GOLDEN_RES, 2, 2, "fp32", 1)
    assert " fold=" not in next(ln for ln in small if ln.startswith("u_block1.residual_blocks.0.conv1 | conv"))  # (there the finalize launch reads them)


def test_the_cached_listings_leave_the_handle_as_it_was():
    L = _lib.lib()
    eng = _Engine(synthetic.geometry_from_cfg(synthetic.default_cfg_dict(resolution=GOLDEN_RES)), 2)
    before = eng.listing(2)
    first = eng.listing_cached(2, 2, 2)
    assert all(L.r2dm_range_site_name(eng.h, k) == b"" for k in range(1, 256))
    assert eng.listing_cached(2, 2, 2) == first and eng.listing(2) == before


# ---- the step plan ------------------------------------------------------------------------------------------------------------------------
def test_the_step_plan():
    T, F = True, False
    cache_plan = lambda num_steps, interval: [step_is_full(i, interval, i > 0) for i in range(num_steps)]  # (a loop nothing interrupts: valid after step 0)
    assert cache_plan(8, 2) == [T, F, T, F, T, F, T, F]
    assert cache_plan(8, 3) == [T, F, F, T, F, F, T, F]
    assert cache_plan(7, 5) == [T, F, F, F, F, T, F]
    assert cache_plan(4, 1) == [T, T, T, T] and cache_plan(0, 2) == [] and cache_plan(1, 9) == [T]
    # full again whenever there is nothing valid to reuse: the loop's start, after a replay has gone back, after a precision switch
    assert step_is_full(3, 2, False) and step_is_full(5, 3, False) and not step_is_full(3, 2, True) and step_is_full(4, 2, True)
    # a loop of 6 at interval 3 whose step 4 is replayed from a checkpoint at step 2 (the cache is dropped there): 2 runs full although 2 % 3 != 0
    ran, valid, i, replayed = [], False, 0, False
    while i < 6:
        full = step_is_full(i, 3, valid)
        ran.append((i, full))
        valid = True
        if i == 4 and not replayed:
            i, valid, replayed = 2, False, True
        else:
            i += 1
    assert ran == [(0, T), (1, F), (2, F), (3, T), (4, F), (2, T), (3, T), (4, F), (5, F)]


def test_what_the_samplers_and_the_cache_refuse():
    import r2dm_amd

    ddpm, _, _ = r2dm_amd.setup_model(synthetic_ckpt(resolution=GOLDEN_RES), device="cpu", show_info=False, max_batch=2)
    known, mask = torch.zeros(2, 2, *GOLDEN_RES), torch.zeros(2, 1, *GOLDEN_RES)
    with pytest.raises(ValueError, match="jumps back in time"):
        ddpm.repaint(known, mask, 4, cache_interval=2)
    with pytest.raises(ValueError, match="jumps back in time"):
        ddpm.complete(known, mask, 4, num_resample_steps=2, cache_interval=2)
    for kw in (dict(cache_interval=0), dict(cache_interval=2.0), dict(cache_interval=True), dict(cache_interval=2, cache_depth=0), dict(cache_depth=4)):
        with pytest.raises(ValueError, match="cache_"):
            ddpm.sample(2, 4, progress=False, **kw)
        with pytest.raises(ValueError, match="cache_"):
            ddpm.sample_dpm(2, 4, progress=False, **kw)
    assert "cache_interval" not in ddpm.invert.__code__.co_varnames  # (not exposed there)
    disc = r2dm_amd.DiscreteTimeGaussianDiffusion(ddpm.model, num_training_steps=10)
    with pytest.raises(ValueError, match="continuous-time samplers"):
        disc.sample(2, 4, progress=False, cache_interval=2)
    net = ddpm.model
    for kw in (dict(depth=0), dict(depth=4), dict(batch=0), dict(batch=3)):
        with pytest.raises(ValueError):
            net.new_cache(**{"batch": 2, **kw})
    cache = net.new_cache(2, depth=2, drift=True)
    assert (cache.batch, cache.depth, cache.valid, cache.usable()) == (2, 2, False, False) and cache.drift().shape == (0, 2)
    with pytest.raises(_lib.R2DMError, match="holds nothing"):
        cache.features()
    with pytest.raises(_lib.R2DMError, match="no drift"):
        net.new_cache(2).drift()
    # what moves the model's generation: a cache filled before any of these is stale
    g0 = net._generation
    net.set_precision("fp16")
    g1 = net._generation
    net.invalidate()
    g2 = net._generation
    net.load_state_dict(net.state_dict())
    assert g0 < g1 < g2 < net._generation
    net.set_precision("fp32")


# ---- the GPU test's inputs tell a shallow forward from a full one -----------------------------------------------------------------------------
def cache_case(res, B=2):
    """(x, cond) the cache is stored at and (x', cond') it is reused at (tests/test_hip_cache.py): conditions -9 and 4; the stored input carries an offset,
    which moves the deep features far enough for the fp16 mode's bar at every depth."""
    return (rnd(301, B, 2, *res) + 8.0, torch.full((B,), -9.0)), (rnd(302, B, 2, *res), torch.full((B,), 4.0))


FORWARD_BAR = 2e-5      # tests/test_hip_unet.py::test_unet_golden: max |delta| of a forward
FORWARD_BAR_FP16 = 3e-3  # tests/test_hip_fp16_mode.py::test_unet_and_sampler_tolerance_class: relative rms of a forward in the "fp16" precision


@functools.lru_cache(maxsize=None)
def oracle_case(res, B=2):
    """In float64 on the CPU, once: per depth the cached tensor, the shallow output at (x', cond') and the full forward there."""
    sd = {k: v.double() for k, v in O.strip_prefix(synthetic_ckpt(resolution=res)["ema_weights"]).items()}
    cfg = O.UNetConfig(resolution=res)
    (x, c), (x2, c2) = cache_case(res, B)
    out = {"full": O.unet_forward(sd, cfg, x2.double(), c2.double())}
    for d in DEPTHS:
        f = CO.cached_feature(sd, cfg, x.double(), c.double(), d)
        out[d] = (f, CO.shallow_forward(sd, cfg, x2.double(), c2.double(), f, d))
    return out


def rel_rms(a, ref):
    return ((a.double() - ref.double()).pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt()).item()


@pytest.mark.parametrize("res", [GOLDEN_RES, (32, 512)])
def test_the_shallow_oracle_is_far_from_the_full_forward_and_exact_on_its_own_features(res):
    case = oracle_case(res)
    for d in DEPTHS if res == GOLDEN_RES else [1]:
        shallow = case[d][1]
        assert (shallow - case["full"]).abs().max().item() >= 100 * FORWARD_BAR, d
        assert rel_rms(shallow, case["full"]) >= 100 * FORWARD_BAR_FP16, d
    if res == GOLDEN_RES:  # fed the features of its own input, the shallow composition is the forward
        sd = {k: v.double() for k, v in O.strip_prefix(synthetic_ckpt(resolution=res)["ema_weights"]).items()}
        cfg = O.UNetConfig(resolution=res)
        x, c = (t.double() for t in cache_case(res)[1])
        for d in DEPTHS:
            assert torch.equal(CO.shallow_forward(sd, cfg, x, c, CO.cached_feature(sd, cfg, x, c, d), d), case["full"])
