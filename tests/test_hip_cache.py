"""-m gpu: the feature cache (DeepCache) -- ``EfficientUNet.forward_cached`` / ``r2dm_unet_forward_cached`` and ``r2dm_cache_store`` (r2dm_amd/csrc/cache.hip,
forward.hip) against their contract in float64 (tests/cache_oracle.py): a store forward is the plain forward bit for bit, the tensor it caches, the shallow
forward at another input and condition for every depth and precision and behind a folded GroupNorm, the samplers under ``cache_interval`` on a noise tape,
the range guard's replay and site numbering across both walks, and the store kernel through its own entry.

Bars: a forward's, as the existing tests state them -- max |delta| < 2e-5 in the parity precisions (tests/test_hip_unet.py::test_unet_golden), relative rms
< 3e-3 in "fp16" (tests/test_hip_fp16_mode.py); the DDPM loop within 1e-4 per step and end to end (test_hip_unet.py's sampling bar), ``sample_dpm`` within
the relative bar of its own GPU test (tests/test_hip_latent.py::relative_bar).  The inputs are tests/test_cache_cpu.py's, where the oracle alone shows that
a shallow forward on them is at least 100 bars from the full one."""
import ctypes
import functools
import warnings

import pytest
import torch

from conftest import GOLDEN_RES, max_abs, rnd, synthetic_ckpt

import cache_oracle as CO
import dpm_oracle as DO
import test_cache_cpu as CC  # (the shared inputs, their float64 oracle results and the bars)
import test_hip_latent as TL  # (relative_bar)
import test_hip_range as TR  # (_edited: the checkpoint that trips the range guard)

import r2dm_amd
from oracle import r2dm_oracle as O
from r2dm_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRECISIONS = ["fp32", "fp32-bf16x3", "fp16"]
DEPTHS = [1, 2, 3]
FOLD_RES = (32, 512)


@functools.lru_cache(maxsize=None)
def model(res=GOLDEN_RES, precision="fp32", max_batch=2):
    return r2dm_amd.setup_model(synthetic_ckpt(resolution=res), device=DEV, show_info=False, max_batch=max_batch, precision=precision)[0]


def case_on_device(res):
    (x, c), (x2, c2) = CC.cache_case(res)
    return (x.to(DEV), c.to(DEV)), (x2.to(DEV), c2.to(DEV))


def within_the_forward_bar(name, got, want, precision):
    mx, rr = max_abs(got.cpu(), want), CC.rel_rms(got.cpu(), want)
    print(f"{name} [{precision}]: max |hip - fp64| {mx:.3e}, relative rms {rr:.3e}")
    assert torch.isfinite(got).all()
    if precision == "fp16":
        assert rr < CC.FORWARD_BAR_FP16, (name, rr)
    else:
        assert mx < CC.FORWARD_BAR, (name, mx)


# ---- 1. store mode is forward -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drift", [False, True])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_store_forward_is_the_forward_bit_for_bit(precision, drift):
    net = model(precision=precision).model
    (x, c), (x2, c2) = case_on_device(GOLDEN_RES)
    want, want2 = net(x, c), net(x2, c2)
    for depth in DEPTHS:
        cache = net.new_cache(2, depth, drift=drift)
        assert torch.equal(net.forward_cached(x, c, cache, refresh=True), want), depth
        assert cache.valid and cache.usable() and cache.precision == precision
        assert torch.equal(net.forward_cached(x2, c2, cache, refresh=True), want2), depth  # (with drift: this one goes through r2dm_cache_store)
        assert torch.equal(net(x, c), want)  # the plain forward after cached ones
        if drift:
            d = cache.drift()
            assert d.shape == (2, 2) and d[0].isnan().all() and (d[1] > 0).all() and torch.isfinite(d[1]).all()


# ---- 2. the cached tensor -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drift", [False, True])
@pytest.mark.parametrize("precision", ["fp32", "fp32-bf16x3"])
def test_the_cached_tensor_vs_fp64(precision, drift):
    net = model(precision=precision).model
    (x, c), _ = case_on_device(GOLDEN_RES)
    oracle = CC.oracle_case(GOLDEN_RES)
    for depth in DEPTHS:
        cache = net.new_cache(2, depth, drift=drift)
        for _ in range(2 if drift else 1):  # (with drift the second store is the one that goes through r2dm_cache_store)
            net.forward_cached(x, c, cache, refresh=True)
        f = cache.features()
        assert f.shape == oracle[depth][0].shape and f.dtype == torch.float32
        e = max_abs(f.cpu(), oracle[depth][0])
        print(f"cached tensor depth {depth} [{precision}, drift {drift}]: max |hip - fp64| {e:.3e} (max |f| {oracle[depth][0].abs().max().item():.2f})")
        assert e < CC.FORWARD_BAR, (depth, e)


def test_the_cached_tensor_in_fp16_storage():
    """The "fp16" precision stores the full-resolution levels as fp16: the depth-1 and depth-2 features are float16 views, depth 3 stays float32."""
    net = model(precision="fp16").model
    (x, c), _ = case_on_device(GOLDEN_RES)
    oracle = CC.oracle_case(GOLDEN_RES)
    for depth in DEPTHS:
        cache = net.new_cache(2, depth)
        net.forward_cached(x, c, cache, refresh=True)
        f = cache.features()
        assert f.shape == oracle[depth][0].shape and f.dtype == net._engine.cached_tensor(2, depth)[1]
        assert f.dtype == (torch.float16 if any(" y16" in ln for ln in net._engine.listing(2).splitlines() if ln.startswith(f"u_block{depth + 1}.upsample | conv")) else torch.float32)
        assert torch.isfinite(f).all() and CC.rel_rms(f.cpu(), oracle[depth][0]) < 0.05  # (the same tensor, not a forward's bar: that is check 3's)


# ---- 3. the shallow forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_shallow_forward_vs_fp64(precision, depth):
    """Stored at (x, -9), reused at (x', 4): against the oracle's shallow forward from the oracle's cached tensor."""
    net = model(precision=precision).model
    (x, c), (x2, c2) = case_on_device(GOLDEN_RES)
    oracle = CC.oracle_case(GOLDEN_RES)
    cache = net.new_cache(2, depth)
    net.forward_cached(x, c, cache, refresh=True)
    got = net.forward_cached(x2, c2, cache, refresh=False)
    within_the_forward_bar(f"shallow forward depth {depth}", got, oracle[depth][1], precision)
    assert torch.equal(got, net.forward_cached(x2, c2, cache, refresh=False))  # reproducible, and the cache is not consumed
    assert max_abs(got.cpu(), oracle["full"]) >= 100 * CC.FORWARD_BAR  # (it is the shallow network that ran)
    # through the drift path the cache holds the same bits
    cache_d = net.new_cache(2, depth, drift=True)
    net.forward_cached(x2, c2, cache_d, refresh=True)
    net.forward_cached(x, c, cache_d, refresh=True)
    assert torch.equal(cache_d.features(), cache.features())
    assert torch.equal(net.forward_cached(x2, c2, cache_d, refresh=False), got)


def test_a_shallow_forward_needs_a_valid_cache_of_this_model():
    net = model().model
    other = r2dm_amd.setup_model(synthetic_ckpt(resolution=GOLDEN_RES), device=DEV, show_info=False, max_batch=2)[0].model
    (x, c), _ = case_on_device(GOLDEN_RES)
    cache = other.new_cache(2)
    with pytest.raises(_lib.R2DMError, match="empty or stale"):
        other.forward_cached(x, c, cache, refresh=False)
    other.forward_cached(x, c, cache, refresh=True)
    other.forward_cached(x, c, cache, refresh=False)
    with pytest.raises(ValueError, match="this model"):
        net.forward_cached(x, c, cache, refresh=False)
    with pytest.raises(ValueError, match="batch 2"):
        other.forward_cached(x[:1], c[:1], cache, refresh=True)
    with pytest.raises(ValueError, match="expected"):
        other.forward_cached(x[:, :1], c, cache, refresh=True)
    other.set_precision("fp32-bf16x3")
    with pytest.raises(_lib.R2DMError, match="empty or stale"):
        other.forward_cached(x, c, cache, refresh=False)
    other.forward_cached(x, c, cache, refresh=True)
    other.invalidate()
    with pytest.raises(_lib.R2DMError, match="empty or stale"):
        other.forward_cached(x, c, cache, refresh=False)


# ---- 4. the folded-norm path --------------------------------------------------------------------------------------------------------------------
def test_the_shallow_forward_behind_a_folded_groupnorm_vs_fp64():
    """32 x 512 at batch 2: the convolution behind the join folds its GroupNorm, i.e. reads the cached statistics slots itself."""
    net = model(res=FOLD_RES).model
    net(*case_on_device(FOLD_RES)[0])  # (the engine exists from the first forward on)
    line = next(ln for ln in net._engine.listing_cached(2, 1, 2).splitlines() if ln.startswith("u_block1.residual_blocks.0.conv1 | conv"))
    assert " fold=" in line, line
    (x, c), (x2, c2) = case_on_device(FOLD_RES)
    oracle = CC.oracle_case(FOLD_RES)
    cache = net.new_cache(2, 1)
    assert torch.equal(net.forward_cached(x, c, cache, refresh=True), net(x, c))
    within_the_forward_bar("cached tensor, 32 x 512", cache.features(), oracle[1][0], "fp32")
    got = net.forward_cached(x2, c2, cache, refresh=False)
    within_the_forward_bar("shallow forward behind a folded norm", got, oracle[1][1], "fp32")
    assert max_abs(got.cpu(), oracle["full"]) >= 100 * CC.FORWARD_BAR


# ---- 5. the samplers ------------------------------------------------------------------------------------------------------------------------------
class Tape:
    """tests/test_hip_unet.py's: feeds recorded draws to ``ddpm.randn``"""

    def __init__(self, ddpm, noise):
        self.noise, self.i = noise, 0
        ddpm.randn = self

    def __call__(self, *shape, rng=None, **kw):
        z = self.noise[self.i].to(DEV)
        self.i += 1
        assert tuple(z.shape) == tuple(shape)
        return z


def spy_on(net):
    flags, inner = [], net.forward_cached
    net.forward_cached = lambda *a, **k: (flags.append(k["refresh"]), inner(*a, **k))[1]
    return flags


@functools.lru_cache(maxsize=None)
def oracle_weights(dtype):
    sd = O.strip_prefix(synthetic_ckpt(resolution=GOLDEN_RES)["ema_weights"])
    return {k: v.to(DEV, dtype) for k, v in sd.items()}, O.UNetConfig(resolution=GOLDEN_RES)


def test_interval_1_is_the_sampler_without_the_keyword():
    ddpm = r2dm_amd.setup_model(synthetic_ckpt(resolution=GOLDEN_RES), device=DEV, show_info=False, max_batch=2)[0]
    flags = spy_on(ddpm.model)
    rng = lambda: r2dm_amd.setup_rng([3, 4], DEV)
    assert torch.equal(ddpm.sample(2, 6, progress=False, rng=rng(), cache_interval=1), ddpm.sample(2, 6, progress=False, rng=rng()))
    assert torch.equal(ddpm.sample_dpm(2, 6, progress=False, rng=rng(), cache_interval=1, cache_depth=2), ddpm.sample_dpm(2, 6, progress=False, rng=rng()))
    assert not flags  # the existing code path: the cached entry is never called
    assert not torch.equal(ddpm.sample(2, 6, progress=False, rng=rng(), cache_interval=2), ddpm.sample(2, 6, progress=False, rng=rng()))
    assert flags == [True, False] * 3


PLANS = {2: [True, False] * 4, 3: [True, False, False, True, False, False, True, False]}


@pytest.mark.parametrize("interval", [2, 3])
def test_sample_under_a_cache_interval_vs_fp64(interval, golden):
    """8 DDPM steps on a noise tape, depth 1: the same loop in float64 with the oracle's step and cache_oracle's denoiser, within 1e-4 at every step and end
    to end.  The tape is tests/test_hip_unet.py::test_sample_golden's own (tests/golden/sample_ddpm.npz), the one its 1e-4 was stated on: at t ~ 1 the
    estimate of x_0 amplifies the denoiser's fp32 roundoff ~1800 times on the few pixels that escape the clamp, so the first steps' maximum is a lottery over
    the draw (that test's docstring), whatever runs the network -- step 0 is a full step, and on a fresh tape (seeds 400..408) the FIRST step, which the cache
    has not touched and which is the plain sampler's bit for bit, came out 1.04e-4 from float64, the next two 2.0e-4 and 1.1e-4, the last 4.1e-5 (measured on
    the MI355X).  The plain loop's and the float32 oracle's own distances on the same tape are printed beside the cached loop's; measured on this tape: at most
    7.7e-5 (step 1, all three loops alike: 7.7e-5 / 7.0e-5 / 7.7e-5), 3.2e-6 and 3.6e-6 at the end for intervals 2 and 3."""
    ddpm = r2dm_amd.setup_model(synthetic_ckpt(resolution=GOLDEN_RES), device=DEV, show_info=False, max_batch=2)[0]
    noise = list(golden("sample_ddpm")["noise"])
    assert len(noise) == 9 and tuple(noise[0].shape) == (2, 2, *GOLDEN_RES)
    flags = spy_on(ddpm.model)
    Tape(ddpm, noise)
    out = ddpm.sample(2, 8, progress=False, rng=None, return_all=True, cache_interval=interval, cache_drift=True)
    assert flags == PLANS[interval]
    drift = ddpm.last_cache_drift
    net64 = CO.CachedNet(*oracle_weights(torch.float64), interval)
    loop = lambda net, dtype: O.sample_continuous(net, (2, 2, *GOLDEN_RES), 8, noises=noise, return_all=True, device=DEV, dtype=dtype)
    truth = loop(net64, torch.float64)
    assert net64.calls == 8 and out.shape == truth.shape
    errs = [max_abs(out[i], truth[i]) for i in range(9)]
    ref32 = loop(CO.CachedNet(*oracle_weights(torch.float32), interval), torch.float32)
    plain64 = loop(lambda x, c: O.unet_forward(*oracle_weights(torch.float64), x, c), torch.float64)
    Tape(ddpm, noise)
    plain = ddpm.sample(2, 8, progress=False, rng=None, return_all=True)
    fmt = lambda es: " ".join(f"{e:.2e}" for e in es)
    print(f"sample, cache_interval {interval}: max |hip - fp64| per step " + fmt(errs))
    print("   the oracle's float32 loop vs fp64:      " + fmt(max_abs(ref32[i], truth[i]) for i in range(9)))
    print("   the plain sampler vs the plain fp64 loop: " + fmt(max_abs(plain[i], plain64[i]) for i in range(9)))
    assert torch.equal(out[1], plain[1])  # (step 0 is a full step)
    assert all(e < 1e-4 for e in errs), errs  # per step, and (the last one) end to end
    Tape(ddpm, noise)
    assert torch.equal(ddpm.sample(2, 8, progress=False, rng=None, cache_interval=interval), out[-1])
    assert max_abs(truth[-1], plain64[-1]) > 1e-2  # (the cached loop is another sampler: the bar above is not met by running the full network)
    assert drift.shape == (sum(PLANS[interval]), 2) and drift.dtype == torch.float64 and drift[0].isnan().all() and (drift[1:] > 0).all()


@pytest.mark.parametrize("interval", [2, 3])
def test_sample_dpm_under_a_cache_interval_vs_fp64(interval):
    """8 steps of DPM-Solver++(2M) from a taped start, depth 1, under the end-to-end bar of tests/test_hip_dpm.py::test_sample_dpm_vs_fp64_oracle."""
    ddpm = r2dm_amd.setup_model(synthetic_ckpt(resolution=GOLDEN_RES), device=DEV, show_info=False, max_batch=2)[0]
    start = rnd(420, 2, 2, *GOLDEN_RES)
    flags = spy_on(ddpm.model)
    Tape(ddpm, [start])
    got = ddpm.sample_dpm(2, 8, progress=False, rng=None, cache_interval=interval)
    assert flags == PLANS[interval]
    ref32 = DO.sample_dpm(CO.CachedNet(*oracle_weights(torch.float32), interval), start.to(DEV), DO.table(8, 2, "logsnr"), "eps", 1.0)
    truth = DO.sample_dpm(CO.CachedNet(*oracle_weights(torch.float64), interval), start.to(DEV).double(), DO.table(8, 2, "logsnr", dtype=torch.float64), "eps", 1.0)
    TL.relative_bar(f"sample_dpm, cache_interval {interval}", got, ref32, truth)
    plain = DO.sample_dpm(lambda x, c: O.unet_forward(*oracle_weights(torch.float64), x, c), start.to(DEV).double(), DO.table(8, 2, "logsnr", dtype=torch.float64), "eps", 1.0)
    assert max_abs(truth, plain) > 1e-2


# ---- 6. guard and replay ----------------------------------------------------------------------------------------------------------------------------
def test_a_tripped_guard_replays_the_cached_loop_on_the_wide_split():
    """The 3e4-gain checkpoint of tests/test_hip_range.py trips the guard at step 0 of a 10-step loop: one warning, the loop goes back to its start with the
    cache dropped, and the result is the wide-range model's on the same tape and interval, bit for bit."""

    def edit(w):
        k = next(k for k in w if k.endswith("d_block1.residual_blocks.0.norm1.weight"))
        w[k] = torch.full_like(w[k], 3.0e4)

    ck = TR._edited(synthetic_ckpt(), edit)
    noise = [rnd(440 + i, 2, 2, 64, 1024) for i in range(11)]
    wide = r2dm_amd.setup_model(ck, device=DEV, show_info=False, max_batch=2, precision="fp32-bf16x3")[0]
    f_wide = spy_on(wide.model)
    Tape(wide, noise)
    s_wide = wide.sample(2, 10, progress=False, rng=None, cache_interval=2)
    assert f_wide == [True, False] * 5
    a = r2dm_amd.setup_model(ck, device=DEV, show_info=False, max_batch=2)[0]
    f_a = spy_on(a.model)
    Tape(a, noise)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        s = a.sample(2, 10, progress=False, rng=None, cache_interval=2)
    assert sum(issubclass(i.category, RuntimeWarning) for i in w) == 1
    assert a.model.precision == "fp32-bf16x3" and a.model.range_fallbacks == 1
    assert f_a == [True] + [True, False] * 5  # step 0 again, as a full step
    assert torch.equal(s, s_wide)


def test_range_sites_keep_their_names_across_both_walks():
    (x, c), (x2, c2) = case_on_device(GOLDEN_RES)
    plain = r2dm_amd.setup_model(synthetic_ckpt(resolution=GOLDEN_RES), device=DEV, show_info=False, max_batch=2)[0]
    plain.model(x, c)
    names = [n for n, _ in plain.model.range_report()]
    assert len(names) > 20 and len(set(names)) == len(names)
    mixed = r2dm_amd.setup_model(synthetic_ckpt(resolution=GOLDEN_RES), device=DEV, show_info=False, max_batch=2)[0]
    mixed.sample(2, 5, progress=False, rng=r2dm_amd.setup_rng([1, 2], DEV), cache_interval=2)
    assert [n for n, _ in mixed.model.range_report()] == names
    # ... also where the handle's first walk is a shallow one's superset only later: plain forward, then a mixed loop at another depth, then plain again
    plain.sample(2, 5, progress=False, rng=r2dm_amd.setup_rng([1, 2], DEV), cache_interval=3, cache_depth=2)
    assert [n for n, _ in plain.model.range_report()] == names
    plain.model(x2, c2)
    assert [n for n, _ in plain.model.range_report()] == names


# ---- 7. the store kernel through its own entry ---------------------------------------------------------------------------------------------------------
def cache_store(fresh, cached, n):
    B = fresh.shape[0]
    partial = torch.full((B * 512 * 2 + 8,), -7.0, dtype=torch.float64, device=DEV)
    sums = torch.full((B, 2), -7.0, dtype=torch.float64, device=DEV)
    _lib.check(_lib.lib().r2dm_cache_store(fresh.data_ptr(), cached.data_ptr(), B, n, int(fresh.dtype == torch.float16), partial.data_ptr(), sums.data_ptr(),
                                           _lib.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    assert (partial[-8:] == -7.0).all()
    return sums


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("n", [1, 63, 64, 4097, 2 * 16 * 128])
@pytest.mark.parametrize("B", [1, 3])
def test_cache_store_copies_bits_and_sums_in_float64(B, n, dtype):
    guard = 64  # elements in front of and behind the cached tensor that must stay as they are
    fresh = (3.0 * rnd(500 + n, B, n)).to(DEV, dtype)
    old = (3.0 * rnd(600 + n, B, n) + 0.5).to(DEV, dtype)
    bits = torch.int32 if dtype == torch.float32 else torch.int16

    def padded(t):
        buf = torch.full((guard + B * n + guard,), 42.0, dtype=dtype, device=DEV)
        buf[guard:guard + B * n] = t.flatten()
        return buf, buf[guard:guard + B * n].view(B, n)

    buf, cached = padded(old)
    sums = cache_store(fresh, cached, n)
    assert torch.equal(cached.view(bits), fresh.view(bits))
    assert (buf[:guard] == 42.0).all() and (buf[-guard:] == 42.0).all()
    f64, o64 = fresh.double(), old.double()
    want = torch.stack([(f64 - o64).pow(2).sum(1), o64.pow(2).sum(1)], dim=1)
    assert ((sums - want).abs() <= 1e-12 * want).all(), (sums, want)
    buf2, cached2 = padded(old)
    assert torch.equal(cache_store(fresh, cached2, n).view(torch.int64), sums.view(torch.int64))  # the same bits from call to call
    again = cache_store(fresh, cached2, n)  # fresh == old now
    assert (again[:, 0] == 0).all() and ((again[:, 1] - f64.pow(2).sum(1)).abs() <= 1e-12 * f64.pow(2).sum(1)).all()


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_two_stores_of_the_same_input_record_no_drift(precision):
    net = model(precision=precision).model
    (x, c), (x2, c2) = case_on_device(GOLDEN_RES)
    cache = net.new_cache(2, 1, drift=True)
    for xi, ci in ((x, c), (x, c), (x2, c2), (x2, c2)):
        net.forward_cached(xi, ci, cache, refresh=True)
    d = cache.drift()
    assert d.shape == (4, 2) and d[0].isnan().all() and (d[1] == 0).all() and (d[2] > 0.01).all() and (d[3] == 0).all(), d
    f = cache.features().double()
    want = CC.oracle_case(GOLDEN_RES)[1][0]
    got = d[2].cpu()
    net.forward_cached(x, c, cache, refresh=True)
    # the recorded drift is the one of the tensors themselves: sqrt(sum (fresh - old)^2 / sum old^2) of the cached features, here against torch in float64
    old = cache.features().double()
    ref = ((f - old).pow(2).sum((1, 2, 3)) / old.pow(2).sum((1, 2, 3))).sqrt().cpu()
    assert want.shape == old.shape and ((got - ref).abs() <= 1e-9 * ref).all(), (got, ref)
