"""-m gpu: completion and stochastic sampling on DPM-Solver++(2M) -- ``r2dm_dpm_step_known`` (r2dm_amd/csrc/posterior.hip) against its contract
in torch ops (tests/dpm_known_oracle.py), its identities with ``r2dm_dpm_step``, what the entry refuses, ``_dpm_table(..., eta)`` against the
oracle's table, ``complete_dpm`` with a denoiser that is itself torch ops against the oracle's float32 loop bit for bit, ``complete_dpm`` and
``sample_dpm(eta=1)`` with the U-Net against the oracle in float64, the tie to ``complete(mode="ddpm")``, the identities and draw counts, the
range guard's replay with history AND recorded noise, and the scripts' new method.

Bars: the kernel and the loop with a torch denoiser are exact (one IEEE rounding per operation, no contraction, in the contract's order).
With the U-Net the bar is the project's relative one (``relative_bar`` of tests/test_hip_latent.py, as tests/test_hip_complete.py uses it):
the distance to the float64 oracle within 2x of the float32 oracle's own in rms and at the 99th percentile, within 4x at the worst element."""
import functools
import json
import subprocess
import sys
import warnings

import pytest
import torch

from conftest import GOLDEN_RES, ROOT, synthetic_ckpt

import complete_oracle as CO
import dpm_known_oracle as KO
import dpm_oracle as DO
import latent_oracle as LO
import test_hip_complete as TCo  # (its scan, its noise tape)
import test_hip_completion as TC  # (its two small scans)
import test_hip_dpm as TD  # (clamped_start, tripping)
import test_hip_latent as TL  # (the cached models and oracle nets, relative_bar, AnalyticDenoiser)

import r2dm_amd
from oracle import r2dm_oracle as O
from r2dm_amd import _lib, completion

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 3
H, W = GOLDEN_RES
SHAPE = (B, 2, H, W)
OBJECTIVES = ["eps", "v", "x_0"]
GRIDS = ["logsnr", "time"]
C = 2
# 4096: one pass of four blocks.  1024 blocks x 256 threads x 4 elements is one pass of the capped grid: 4 KiB more is a second pass
PER_SAMPLE = [4096, 1024 * 256 * 4 + 4096]


# ---- 1. r2dm_dpm_step_known against its contract ----------------------------------------------------------------------------------------------------
def kernel_rows(which):
    """three rows of the real 8-step table of eta = 1, one per sample (the choice of tests/test_hip_dpm.py): "first" -- the step from t = 1,
    one in between, the first-order last one; "second" -- without ``lower_order_final``: three rows with c_1 != 0.  c_z != 0 in all."""
    ddpm = TL.model()[0]
    _, coef, second = ddpm._dpm_table(8, 1, 2, "logsnr", 1.0, which == "first", DEV, eta=1.0)
    rows = coef[[0, 4, 7] if which == "first" else [1, 4, 7], 0]
    assert (rows[:, 5] > 0).all() and not rows[:, 6:].any()
    if which == "first":
        assert rows[0, 0] < 6e-4 and not second[0] and not second[7] and rows[0, 4] == 0 and rows[1, 4] != 0
    else:
        assert second[1] and second[7] and (rows[:, 4] != 0).all()
    return rows.contiguous()


def kernel_case(per_sample, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    plane = per_sample // C
    x, pr, z, h, y = (torch.randn(B, C, plane, generator=g, device=DEV) for _ in range(5))
    masks = {0: None}
    for mask_c in (1, C):
        m = torch.empty(B, mask_c, plane, device=DEV)
        m[0] = (torch.rand(mask_c, plane, generator=g, device=DEV) < 0.5).float()  # binary
        m[1] = 0.25  # the weight form
        m[2] = torch.rand(mask_c, plane, generator=g, device=DEV)  # any weight in [0, 1)
        masks[mask_c] = m
    return x, pr, z, torch.tanh(h), torch.tanh(y), masks


@pytest.mark.parametrize("per_sample", PER_SAMPLE)
@pytest.mark.parametrize("which", ["first", "second"])
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_dpm_step_known_bit_exact_vs_torch_ops(objective, which, per_sample):
    """every objective x {first, second order} x {noise, none} x {no measurement, 1-channel mask, C-channel mask} x {clamp, none}"""
    coef = kernel_rows(which)
    x, pr, z, h, y, masks = kernel_case(per_sample, per_sample % 1000 + 10 * OBJECTIVES.index(objective) + (which == "second"))
    obj_id = OBJECTIVES.index(objective)
    k = [coef[:, j][:, None, None] for j in range(6)]
    results = {}
    for clip in (1.0, -1.0):
        for prev in (None, h):
            for noise in (None, z):
                for mask_c, m in masks.items():
                    known = None if m is None else y
                    got_x, got_x0 = _lib.dpm_step_known(x, pr, prev, noise, known, m, coef, obj_id, clip)
                    want_x, want_x0 = KO.dpm_step_known(x, pr, prev, noise, known, m, *k, objective, clip)  # (one rounding per torch op)
                    case = (clip, prev is not None, noise is not None, mask_c)
                    assert got_x.dtype == got_x0.dtype == torch.float32 and got_x.shape == got_x0.shape == x.shape
                    assert torch.isfinite(got_x).all() and torch.isfinite(got_x0).all()
                    assert torch.equal(got_x0, want_x0), (case, (got_x0 - want_x0).abs().max().item())
                    assert torch.equal(got_x, want_x), (case, (got_x - want_x).abs().max().item())
                    results[case] = got_x
                    if m is not None:
                        assert torch.equal(got_x0[1], 0.25 * y[1] + (1.0 - 0.25) * _lib.dpm_step(x, pr, None, coef, obj_id, clip)[1][1])
        # x0 written over x0_prev's own buffer: the row with every operand
        buf = h.clone()
        alias_x, alias_x0 = _lib.dpm_step_known(x, pr, buf, z, y, masks[1], coef, obj_id, clip, x0_out=buf)
        full_x, full_x0 = _lib.dpm_step_known(x, pr, h, z, y, masks[1], coef, obj_id, clip)
        assert alias_x0.data_ptr() == buf.data_ptr() and torch.equal(alias_x, full_x) and torch.equal(buf, full_x0)
    # every operand changes the result (c_z != 0; c_1 != 0 on the second-order rows)
    base = results[1.0, which == "second", False, 0]
    assert not torch.equal(results[1.0, which == "second", True, 0], base) and not torch.equal(results[1.0, which == "second", False, 1], base)
    assert not torch.equal(results[1.0, which == "second", False, C], results[1.0, which == "second", False, 1])
    if which == "second":
        assert not torch.equal(results[1.0, False, False, 0], base)


# ---- 2. its identities ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_sample", PER_SAMPLE)
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_dpm_step_known_identities(objective, per_sample):
    obj_id = OBJECTIVES.index(objective)
    x, pr, z, h, y, masks = kernel_case(per_sample, 77 + obj_id)
    for which in ("first", "second"):
        coef = kernel_rows(which)
        quiet = coef.clone()
        quiet[:, 5] = 0.0
        for clip in (1.0, -1.0):
            for prev in (None, h):
                plain = _lib.dpm_step(x, pr, prev, coef, obj_id, clip)
                # no noise and no measurement: r2dm_dpm_step
                bare = _lib.dpm_step_known(x, pr, prev, None, None, None, coef, obj_id, clip)
                assert torch.equal(bare[0], plain[0]) and torch.equal(bare[1], plain[1])
                # an all-zero mask: the no-measurement call, with and without noise
                for noise in (None, z):
                    free = _lib.dpm_step_known(x, pr, prev, noise, None, None, coef, obj_id, clip)
                    for mask_c in (1, C):
                        got = _lib.dpm_step_known(x, pr, prev, noise, y, torch.zeros_like(masks[mask_c]), coef, obj_id, clip)
                        assert torch.equal(got[0], free[0]) and torch.equal(got[1], free[1])
                # noise with c_z = 0: the no-noise call, with and without a measurement
                for mask_c in (0, 1, C):
                    known = None if mask_c == 0 else y
                    a = _lib.dpm_step_known(x, pr, prev, z, known, masks[mask_c], quiet, obj_id, clip)
                    b = _lib.dpm_step_known(x, pr, prev, None, known, masks[mask_c], quiet, obj_id, clip)
                    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # all known (mask of ones): the estimate is the measurement whatever the prediction
    ones = torch.ones_like(masks[1])
    a, b = (_lib.dpm_step_known(x, q, None, z, y, ones, coef, obj_id, 1.0) for q in (pr, pr.flip(-1)))
    assert torch.equal(a[1], y) and torch.equal(a[0], b[0])


# ---- 3. what it refuses -------------------------------------------------------------------------------------------------------------------------------
def test_dpm_step_known_refusals():
    """each refusal is a non-zero status with its message in ``r2dm_last_error``; nothing is launched (the outputs keep their fill, the inputs
    their zeros), nothing faults"""
    L = _lib.lib()
    n = 4096
    buf = torch.zeros(2 * n + 4, device=DEV)
    ok, off = buf[:2 * n], buf[1:1 + 2 * n]
    assert off.data_ptr() % 16 == 4
    pr, h, z, y, m = (torch.zeros(2 * n, device=DEV) for _ in range(5))
    coef = torch.ones(2, 8, device=DEV)
    out, est = torch.full((2 * n + 4,), 7.0, device=DEV), torch.full((2 * n + 4,), 7.0, device=DEV)
    stream = _lib.stream_ptr(torch.device(DEV, 0))

    def call(x=ok, pr=pr, h=h, z=z, y=y, m=m, k=coef, o=out[:2 * n], e=est[:2 * n], batch=2, per_sample=n, channels=2, mask_c=1, objective=0):
        p = lambda t: None if t is None else t.data_ptr()
        return L.r2dm_dpm_step_known(p(x), p(pr), p(h), p(z), p(y), p(m), p(k), p(o), p(e), batch, per_sample, channels, mask_c, objective, 1.0, stream)

    def refused(text, **kw):
        assert call(**kw) != 0, kw
        msg = L.r2dm_last_error().decode()
        assert msg.startswith("dpm_step_known: ") and text in msg, (kw, msg)

    # everything r2dm_dpm_step refuses
    for name in ("x", "pr", "h", "z", "y", "m", "o", "e"):
        refused("16-byte aligned", **{name: (out if name == "o" else est)[1:1 + 2 * n] if name in ("o", "e") else off})
    odd = coef.view(torch.uint8).flatten()[1:]
    assert odd.data_ptr() % 4 == 1
    refused("4-byte aligned", k=odd)
    refused("multiple of 4", per_sample=4098)
    refused("[4, 2^40", per_sample=2)
    refused("objective", objective=3)
    refused("objective", objective=-1)
    refused("batch", batch=0)
    refused("batch", batch=65536)
    for name in ("x", "pr", "k", "o", "e"):
        refused("null", **{name: None})
    refused("alias", o=ok)  # x_s == x_t
    refused("alias", o=pr)
    refused("alias", o=h)
    refused("alias", e=ok)
    refused("alias", e=pr)
    refused("alias", o=est[:2 * n])  # x_s == x0
    # what r2dm_posterior_step_known refuses about known, mask, channels and mask_channels
    refused("multiple of 4", per_sample=4092, channels=2)  # a plane of 2046
    refused("divide into", channels=3)
    refused("divide into", channels=0)
    refused("mask_channels", mask_c=3)
    refused("mask_channels", mask_c=0)
    refused("mask_channels", mask_c=3, y=None, m=None)  # (with or without a measurement)
    # exactly one of known / mask
    refused("together", y=None)
    refused("together", m=None)
    # an output over noise, known or mask
    for name in ("z", "y", "m"):
        refused("alias", **{name: out[:2 * n]})
        refused("alias", **{name: est[:2 * n]})
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (est == 7.0).all() and not buf.any() and not any(t.any() for t in (pr, h, z, y, m))
    # what it takes: every operand, none of the optional ones, x0 over the history, a C-channel mask
    assert call() == 0 and call(h=None, z=None, y=None, m=None) == 0 and call(e=h) == 0 and call(mask_c=2, objective=2) == 0
    torch.cuda.synchronize()
    assert (out[2 * n:] == 7.0).all() and (est[2 * n:] == 7.0).all()
    # the wrapper: operands of one shape, a (B,8) row, known and mask together
    x4 = torch.zeros(2, 2, 16, 64, device=DEV)
    m4 = torch.zeros(2, 1, 16, 64, device=DEV)
    with pytest.raises(ValueError):
        _lib.dpm_step_known(x4, x4[:, :1], None, None, None, None, coef, 0, 1.0)
    with pytest.raises(ValueError):
        _lib.dpm_step_known(x4, x4, None, x4[:1], None, None, coef, 0, 1.0)
    with pytest.raises(ValueError):
        _lib.dpm_step_known(x4, x4, None, None, x4, m4, coef[:, :4], 0, 1.0)
    with pytest.raises(ValueError):
        _lib.dpm_step_known(x4, x4, None, None, x4, None, coef, 0, 1.0)
    with pytest.raises(_lib.R2DMError, match="multiple of 4"):
        _lib.dpm_step_known(*([torch.zeros(2, 1, 4098, device=DEV)] * 2), None, None, None, None, coef, 0, 1.0)
    with pytest.raises(_lib.R2DMError):
        _lib.dpm_step_known(x4.cpu(), x4.cpu(), None, None, None, None, coef.cpu(), 0, 1.0)
    torch.cuda.synchronize()


# ---- 4. the sampler's table against the oracle's --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t_start", [1.0, 0.5])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("grid", GRIDS)
def test_the_samplers_table_with_eta_is_the_oracles(grid, order, eta, t_start):
    """as tests/test_hip_dpm.py::test_the_samplers_table_is_the_oracles: the conditions, alpha_t and sigma_t equal, the solver's scalars
    (c_z among them) within one float32 ulp.  At eta = 0 the table is the cached object of the call without the keyword."""
    ddpm = TL.model()[0]
    for S in (4, 20):
        cond, coef, second = ddpm._dpm_table(S, B, order, grid, t_start, True, DEV, eta=eta)
        assert cond.shape == (S, B) and coef.shape == (S, B, 8) and second.shape == (S,) and cond.is_cuda and coef.is_cuda and not second.is_cuda
        o_cond, o_coef, o_second = KO.table(S, order, grid, t_start, True, eta)
        assert second.tolist() == o_second
        cond, coef = cond.cpu(), coef.cpu()
        for b in range(B):
            assert torch.equal(cond[:, b], o_cond) and torch.equal(coef[:, b, :2], o_coef[:, :2]) and not coef[:, b, 6:].any()
            assert torch.equal(coef[:, b], coef[:, 0])
        ulps = (coef[:, 0, 2:6].contiguous().view(torch.int32) - o_coef[:, 2:6].contiguous().view(torch.int32)).abs()
        print(f"{grid} order {order} eta {eta} S={S} t_start={t_start}: {int((ulps != 0).sum())} of {ulps.numel()} solver scalars differ, at most {int(ulps.max())} ulp")
        assert ulps.max().item() <= 1
        assert ((coef[:, 0, 5] > 0).all() if eta > 0 else not coef[:, 0, 5].any())
        plain = ddpm._dpm_table(S, B, order, grid, t_start, True, DEV)
        if eta == 0:
            assert ddpm._dpm_table(S, B, order, grid, t_start, True, DEV, eta=0.0) is plain
            d_cond, d_coef, d_second = DO.table(S, order, grid, t_start, True)
            assert torch.equal(plain[0][:, 0].cpu(), d_cond) and d_second == plain[2].tolist()
        else:
            assert torch.equal(plain[0].cpu(), cond) and torch.equal(plain[1][..., :2].cpu(), coef[..., :2]) and not torch.equal(plain[1].cpu(), coef)
    assert len(ddpm.__dict__["_dpm_tables"]) <= 8


# ---- the inputs the sampler tests share ---------------------------------------------------------------------------------------------------------------
def tape_of(seeds, n):
    return TCo.tape_of(seeds, n)


@functools.lru_cache(maxsize=None)
def scan_for(objective, seed0):
    """``test_hip_complete.scan()`` -- (known, mask (B,1,H,W)) -- for a run whose start at t = 1 is the first draw of ``setup_rng(range(seed0,
    seed0 + B))``.  For ``eps`` the mask also holds the few pixels at which the FIRST step's estimate (x - sigma_1 eps) / alpha_1 falls inside
    the clamp (|estimate| < 4 in the float64 oracle, either channel), so that the measurement is written over them.

    Why: 1 / alpha_1 is 1800.  At a pixel whose estimate is inside the clamp at t = 1 the last bits of the denoiser's output arrive in the
    sample multiplied by that, and one such pixel (about 4 in 10^4 of an N(0, 1) tensor) then decides rms and max of the comparison on BOTH
    sides -- the float32 oracle's own distance to float64 moved 18 x between runs (tests/test_hip_dpm.py::clamped_start, which conditions
    the start tensor for the same reason; here the start is the generator's draw, so the mask is what can be chosen).  Only the float64
    oracle is consulted, never the code under test.  Computed once, left unchanged."""
    known, mask = TCo.scan()
    if objective != "eps":
        return known, mask
    x = tape_of(list(range(seed0, seed0 + B)), 1)[0].double()
    _, net64 = TL.nets(objective)
    lam = DO.log_snr_grid(1, "time", 1.0, torch.float64)[:1].to(DEV).expand(B)
    a, s = O.alpha_sigma(lam[:, None, None, None])
    inside = (((x - s * net64(x, lam)) / a).abs() < 4).any(dim=1, keepdim=True)
    assert int(inside.sum()) < 100
    return known, torch.where(inside, torch.ones_like(mask), mask)


# ---- 5. with a denoiser in torch ops: the oracle's float32 loop, bit for bit -----------------------------------------------------------------------
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("order", [1, 2])
def test_complete_dpm_with_the_analytic_denoiser_is_the_oracles_loop(order, grid, eta):
    ddpm = r2dm_amd.ContinuousTimeGaussianDiffusion(TL.AnalyticDenoiser(), prediction_type="eps", noise_schedule="cosine").to(DEV)
    ddpm.set_schedule_on("device")  # (the start from ``init``: q_step_from_x_0's scalars where the oracle evaluates them)
    known, mask = TCo.scan()
    S = 5
    seeds = list(range(120, 120 + B))
    tape = tape_of(seeds, KO.num_draws(S, eta))
    tab = ddpm._dpm_table(S, B, order, grid, 1.0, True, DEV, eta=eta)
    got = ddpm.complete_dpm(known, mask, S, order=order, grid=grid, eta=eta, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV), return_all=True)
    want = KO.complete_dpm(LO.analytic_eps, known, mask, (tab[0], tab[1], tab[2].tolist()), tape, eta, return_all=True)
    assert got.shape == (S + 1, *SHAPE) and torch.equal(got[0], tape[0])
    assert torch.equal(got, want), (got - want).abs().max().item()
    # from a partially noised start, unclamped, without the final projection, under a weight mask
    tab = ddpm._dpm_table(S, B, order, grid, 0.5, True, DEV, eta=eta)
    soft = 0.75 * mask
    got = ddpm.complete_dpm(known, soft, S, order=order, grid=grid, eta=eta, t_start=0.5, init=0.5 * known, exact_known=False, clip=False,
                            progress=False, rng=r2dm_amd.setup_rng(seeds, DEV))
    want = KO.complete_dpm(LO.analytic_eps, known, soft, (tab[0], tab[1], tab[2].tolist()), tape, eta, t_start=0.5, init=0.5 * known, clip=None,
                           exact_known=False)
    assert torch.equal(got, want), (got - want).abs().max().item()


# ---- 6. against the oracle in float64 on the synthetic U-Net ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("S", [4, 6])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_complete_dpm_vs_fp64_oracle(objective, grid, S, eta):
    """Order 2, the model's clamp, from noise at t = 1 and from ``init`` noised to t = 0.5; the oracle's loops run on its own tables (float32 /
    float64) on the tape of the generators.  Measured on the MI355X: see DESIGN.md section 4, 'Completion on DPM-Solver++'."""
    ddpm = TL.model(objective)[0]
    net32, net64 = TL.nets(objective)
    seeds = list(range(90, 90 + B))
    known, mask = scan_for(objective, seeds[0])
    tape = tape_of(seeds, KO.num_draws(S, eta))
    for t_start, init in ((1.0, None), (0.5, 0.5 * known)):
        got = ddpm.complete_dpm(known, mask, S, grid=grid, eta=eta, t_start=t_start, init=init, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV))
        assert got.shape == SHAPE and got.dtype == torch.float32
        kw = dict(t_start=t_start, objective=objective)
        ref32 = KO.complete_dpm(net32, known, mask, KO.table(S, 2, grid, t_start, True, eta), tape, eta, init=init, **kw)
        truth = KO.complete_dpm(net64, known.double(), mask.double(), KO.table(S, 2, grid, t_start, True, eta, torch.float64), tape, eta,
                                init=None if init is None else init.double(), **kw)
        TL.relative_bar(f"complete_dpm {objective} {grid} S={S} eta={eta} t_start={t_start}", got, ref32, truth)
        on = mask.expand_as(known) == 1
        assert torch.equal(got[on], known[on])


@pytest.mark.parametrize("S", [4, 6])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_sample_dpm_with_eta_1_vs_fp64_oracle(objective, grid, S):
    """SDE-DPM-Solver++(2M): order 2, eta = 1, from ``clamped_start`` of tests/test_hip_dpm.py at t = 1 and from a scan-like tensor at t = 0.5,
    the steps' noise from the generators"""
    ddpm = TL.model(objective)[0]
    net32, net64 = TL.nets(objective)
    seeds = list(range(100, 100 + B))
    tape = tape_of(seeds, S)
    for t_start, x in ((1.0, TD.clamped_start(objective)), (0.5, TL.scan_like())):
        got = ddpm.sample_dpm(B, S, grid=grid, x_t=x, t_start=t_start, eta=1.0, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV))
        assert got.shape == SHAPE and got.dtype == torch.float32
        ref32 = KO.run(net32, x, KO.table(S, 2, grid, t_start, True, 1.0), tape, objective=objective)
        truth = KO.run(net64, x.double(), KO.table(S, 2, grid, t_start, True, 1.0, torch.float64), tape, objective=objective)
        TL.relative_bar(f"sample_dpm eta=1 {objective} {grid} S={S} t_start={t_start}", got, ref32, truth)


# ---- 7. order 1, eta = 1 on the time grid is complete's ancestral step ------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_order_1_eta_1_on_the_time_grid_vs_the_ancestral_completion(objective):
    """``c_x x + m x0 + c_z z`` is ``complete(mode="ddpm")``'s update in another operation order: on the same generators both sit within the
    bar of the oracle's ancestral completion in float64"""
    ddpm = TL.model(objective)[0]
    net32, net64 = TL.nets(objective)
    S = 4
    seeds = list(range(110, 110 + B))
    known, mask = scan_for(objective, seeds[0])
    tape = tape_of(seeds, CO.num_draws(S))
    assert CO.num_draws(S) == KO.num_draws(S, 1.0)
    got = ddpm.complete_dpm(known, mask, S, order=1, grid="time", eta=1.0, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV))
    anc = ddpm.complete(known, mask, S, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV))
    truth = CO.complete(net64, known.double(), mask.double(), S, tape, objective=objective)
    ref32 = CO.complete(net32, known, mask, S, tape, objective=objective)
    TL.relative_bar(f"complete_dpm order 1 eta 1, time grid vs ancestral completion {objective}", got, ref32, truth)
    TL.relative_bar(f"complete(mode=ddpm) vs ancestral completion {objective}", anc, ref32, truth)


# ---- 8. equalities and draw counts --------------------------------------------------------------------------------------------------------------------
def states(gens):
    return [g.get_state() for g in gens]


def same_states(a, b):
    return all(torch.equal(s, t) for s, t in zip(a, b))


def states_after(seeds, draws):
    g = r2dm_amd.setup_rng(seeds, DEV)
    for _ in range(draws):
        O.draw_noise(SHAPE, g, DEV, torch.float32)
    return states(g)


def test_complete_dpm_with_nothing_known_is_sample_dpm():
    ddpm = TL.model()[0]
    known, _ = TCo.scan()
    zero = torch.zeros(B, 1, H, W, device=DEV)
    S = 5
    seeds = list(range(50, 50 + B))
    for kw in (dict(), dict(order=1, grid="time"), dict(lower_order_final=False, clip=False)):
        for eta in (0.0, 1.0):
            g1, g2 = r2dm_amd.setup_rng(seeds, DEV), r2dm_amd.setup_rng(seeds, DEV)
            want = ddpm.sample_dpm(B, S, progress=False, rng=g1, return_all=True, eta=eta, **kw)
            got = ddpm.complete_dpm(known, zero, S, eta=eta, progress=False, rng=g2, return_all=True, **kw)
            assert got.shape == (S + 1, *SHAPE) and torch.equal(got, want), (kw, eta)
            # the generators stand 1 + S draws on (eta > 0), one draw on (eta = 0) -- in both samplers
            assert same_states(states(g1), states(g2)) and same_states(states(g2), states_after(seeds, 1 + S if eta > 0 else 1)), (kw, eta)
    # from an init: one draw for q_step_from_x_0, then the steps'
    g1, g2 = r2dm_amd.setup_rng(seeds, DEV), r2dm_amd.setup_rng(seeds, DEV)
    x_t, _ = ddpm.q_step_from_x_0(known, torch.full((B,), 0.5), rng=g1)
    want = ddpm.sample_dpm(B, S, x_t=x_t, t_start=0.5, eta=1.0, progress=False, rng=g1)
    got = ddpm.complete_dpm(known, zero, S, t_start=0.5, init=known, progress=False, rng=g2)  # (eta = 1 is the default)
    assert torch.equal(got, want) and same_states(states(g1), states(g2)) and same_states(states(g2), states_after(seeds, 1 + S))
    # a single generator
    one = torch.Generator(device=DEV).manual_seed(3)
    a = ddpm.complete_dpm(known, zero, S, progress=False, rng=one)
    ref = torch.Generator(device=DEV).manual_seed(3)
    assert torch.equal(a, ddpm.sample_dpm(B, S, eta=1.0, progress=False, rng=ref)) and torch.equal(one.get_state(), ref.get_state())


def test_sample_dpm_without_eta_is_the_parents_loop():
    """``sample_dpm(...)`` with its arguments of before: ``r2dm_dpm_step`` composed by hand on the eta-less table, bit for bit, one draw"""
    for objective in OBJECTIVES:
        ddpm = TL.model(objective)[0]
        S = 5
        seeds = list(range(55, 55 + B))
        g = r2dm_amd.setup_rng(seeds, DEV)
        got = ddpm.sample_dpm(B, S, progress=False, rng=g)
        assert same_states(states(g), states_after(seeds, 1))
        cond, coef, second = ddpm._dpm_table(S, B, 2, "logsnr", 1.0, True, DEV)
        x, hist = tape_of(seeds, 1)[0], None
        for i in range(S):
            x, hist = _lib.dpm_step(x, ddpm.model(x, cond[i]), hist if second[i] else None, coef[i], OBJECTIVES.index(objective), 1.0)
        assert torch.equal(got, x)
        assert torch.equal(got, ddpm.sample_dpm(B, S, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV), eta=0.0))
        assert not torch.equal(got, ddpm.sample_dpm(B, S, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV), eta=1.0))


def test_complete_dpm_is_batch_independent_reproducible_and_exact_on_the_mask():
    ddpm = TL.model()[0]
    known, mask = TCo.scan()
    S = 4
    seeds = list(range(70, 70 + B))
    on = mask.expand_as(known) == 1
    for eta in (1.0, 0.0):
        run = lambda **kw: ddpm.complete_dpm(known, mask, S, eta=eta, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV), **kw)
        got = run()
        assert torch.equal(got, run())
        alone = ddpm.complete_dpm(known[1:2], mask[1:2], S, eta=eta, progress=False, rng=r2dm_amd.setup_rng(seeds[1:2], DEV))
        assert torch.equal(alone[0], got[1])
        assert torch.equal(got[on], known[on]) and not torch.equal(got[~on], known[~on])
        # a (B,C,H,W) mask and a (1,1,H,W) one are the same masks spelled out
        assert torch.equal(ddpm.complete_dpm(known, mask.expand(-1, 2, -1, -1), S, eta=eta, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV)), got)
        one = ddpm.complete_dpm(known, mask[1:2], S, eta=eta, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV))
        assert torch.equal(one[1], got[1])
        g = r2dm_amd.setup_rng(seeds, DEV)
        stack = ddpm.complete_dpm(known, mask, S, eta=eta, progress=False, rng=g, return_all=True)
        assert stack.shape == (S + 1, *SHAPE) and torch.equal(stack[-1], got) and torch.equal(stack[0], tape_of(seeds, 1)[0])
        assert same_states(states(g), states_after(seeds, 1 + S if eta > 0 else 1))
        # without the final projection the last step's sigma(0)-sized terms stay on the known pixels; the unknown ones are the same
        raw = run(exact_known=False)
        assert torch.equal(raw[~on], got[~on]) and (raw - known)[on].abs().max().item() < 0.05
        if eta > 0:
            assert not torch.equal(raw[on], known[on])
    # the options change the result
    base = ddpm.complete_dpm(known, mask, S, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV))
    for kw in (dict(order=1), dict(grid="time"), dict(eta=0.0), dict(eta=0.5), dict(lower_order_final=False)):
        assert not torch.equal(ddpm.complete_dpm(known, mask, S, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV), **kw), base), kw
    with pytest.raises(r2dm_amd.diffusion.NoCPUFallback):
        ddpm.complete_dpm(known.cpu(), mask.cpu(), S, progress=False)


# ---- 9. a range-guard trip goes back with the history and the recorded noise -------------------------------------------------------------------------
def test_a_tripped_range_guard_replays_the_completion_with_history_and_noise():
    """A 40-step eta = 1 completion is checked after steps 0, 31 and 39.  The bound is raised behind denoiser call 35 (step 34): the check at the
    end trips -- ONE RuntimeWarning, the model switches to 'fp32-bf16x3' -- and the loop goes back to step 32 with the checkpointed pair
    (x_32, the PROJECTED estimate of step 31) and runs steps 32..39 again on the noise it drew for them the first time: 48 denoiser calls, the
    generators 1 + 40 draws on, no exception.  As in tests/test_hip_dpm.py the result is, bit for bit, steps 0..31 of the default model
    followed by steps 32..39 of the wide model, built here from the public pieces."""
    S = 40
    ck = synthetic_ckpt(resolution=GOLDEN_RES)
    known, mask = TCo.scan()
    seeds = list(range(140, 140 + B))
    tape = tape_of(seeds, 1 + S)
    wide = r2dm_amd.setup_model(ck, device=DEV, show_info=False, max_batch=B, precision="fp32-bf16x3")[0]
    base = r2dm_amd.setup_model(ck, device=DEV, show_info=False, max_batch=B)[0]
    stack = base.complete_dpm(known, mask, S, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV), return_all=True, exact_known=False)
    cond, coef, second = base._dpm_table(S, B, 2, "logsnr", 1.0, True, DEV, eta=1.0)
    assert second[32] and second[31] and torch.equal(stack[0], tape[0])
    # (the projected estimate depends neither on the history nor on the noise)
    _, hist = _lib.dpm_step_known(stack[31], base.model(stack[31], cond[31]), None, None, known, mask, coef[31], 0, 1.0)
    xs = stack[32]
    for i in range(32, S):
        xs, hist = _lib.dpm_step_known(xs, wide.model(xs, cond[i]), hist if second[i] else None, tape[1 + i], known, mask, coef[i], 0, 1.0)
    want = _lib.repaint_blend(known, known, xs, mask, torch.tensor([[1.0, 0.0]], device=DEV).repeat(B, 1))
    assert base.model.precision != "fp32-bf16x3" and base.model.range_fallbacks == 0

    def run_watched(ddpm, **kw):
        g = r2dm_amd.setup_rng(seeds, DEV)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            got = ddpm.complete_dpm(known, mask, S, progress=False, rng=g, **kw)
        assert same_states(states(g), states_after(seeds, 1 + S))  # (a replay draws nothing)
        return got, sum(issubclass(i.category, RuntimeWarning) and "fp32-bf16x3" in str(i.message) for i in w)

    ddpm, calls = TD.tripping(ck, 35)
    got, warned = run_watched(ddpm)
    assert warned == 1 and len(calls) == 48 and ddpm.model.precision == "fp32-bf16x3" and ddpm.model.range_fallbacks == 1
    assert torch.isfinite(got).all()
    print(f"tripped completion: max |x - untripped default run| {(got - base.complete_dpm(known, mask, S, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV))).abs().max().item():.3e}")
    assert torch.equal(got, want), (got - want).abs().max().item()
    # the switched model's next call, and a trip at the first check: the wide model's whole run
    want_wide = wide.complete_dpm(known, mask, S, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV))
    again, warned = run_watched(ddpm)
    assert warned == 0 and torch.equal(again, want_wide)
    early, calls = TD.tripping(ck, 1)
    got, warned = run_watched(early, return_all=True)
    assert warned == 1 and len(calls) == 41 and got.shape == (S + 1, *SHAPE) and torch.equal(got[-1], want_wide)
    strict, _ = TD.tripping(ck, 35, strict_range=True)
    with pytest.raises(_lib.R2DMRangeError):
        strict.complete_dpm(known, mask, S, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV))


# ---- 10. the scripts -------------------------------------------------------------------------------------------------------------------------------------
KINDS = ("beams:4", "random_points:0.5")
METHODS = ("dpmpp", "linear")
SEED = 5


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("complete_dpm")
    ckpt = tmp / "synthetic.pth"
    torch.save(synthetic_ckpt(resolution=GOLDEN_RES), ckpt)
    for k, s in enumerate(TC.small_scans()):
        d = tmp / "scans" / f"seq_{k}"
        d.mkdir(parents=True)
        s.tofile(d / f"{k:010d}.bin")
    return tmp, ckpt


def test_completion_eval_with_the_dpmpp_method(files):
    tmp, ckpt = files
    args = ["--ckpt", str(ckpt), "--real_scans", str(tmp / "scans"), "--methods", *METHODS, "--num_steps", "2", "--batch_size", "2", "--seed", str(SEED),
            "--save_dir", str(tmp / "kept"), "--out", str(tmp / "kept" / "completion.json")]
    for kind in KINDS:
        args += ["--corruption", kind]
    r = subprocess.run([sys.executable, f"{ROOT}/completion_eval.py", *args], cwd=tmp, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert any("dpmpp: MAE depth" in line for line in r.stdout.splitlines()), r.stdout
    doc = json.loads((tmp / "kept" / "completion.json").read_text())
    info = doc["info"]
    assert info["methods"] == list(METHODS) and (info["dpmpp_eta"], info["dpmpp_order"], info["dpmpp_init"], info["dpmpp_t_start"]) == (1.0, 2, "none", 1.0)
    assert not any(k.startswith("ddnm") for k in info)  # (a method's settings are echoed only when it is used)
    ddpm, lidar, _ = r2dm_amd.setup_model(str(ckpt), device=DEV, show_info=False, max_batch=2)
    for kind in KINDS:
        e = doc["results"][kind]
        assert set(e["dpmpp"]) == {"counts", "sums", "micro", "macro"} and e["dpmpp"]["counts"]["evaluated"] > 100
        k = torch.load(tmp / "kept" / (kind.replace(":", "_") + ".pt"))
        x_in, mask, x_out = k["x_in"].to(DEV), k["mask"].to(DEV), k["x_out"]["dpmpp"].to(DEV)
        rng = r2dm_amd.setup_rng([completion.scan_seed(SEED, i) for i in range(2)], DEV)
        assert torch.equal(x_out, ddpm.complete_dpm(x_in, mask, 2, progress=False, rng=rng))
        on = mask.expand_as(x_in) == 1
        assert torch.equal(x_out[on], x_in[on])
        assert torch.equal(lidar.postprocess(x_out.clamp(-1, 1)).cpu(), k["pred"]["dpmpp"])
    assert "skipped" in doc["results"]["random_points:0.5"]["linear"] and "skipped" not in doc["results"]["random_points:0.5"]["dpmpp"]
    # the settings reach the sampler, with ddnm's init rules (the script's ``main`` in this process)
    import completion_eval

    doc = completion_eval.main(args[:-4] + ["--save_dir", str(tmp / "init"), "--out", str(tmp / "init" / "completion.json"), "--dpmpp_init", "linear",
                                            "--dpmpp_t_start", "0.5", "--dpmpp_eta", "0.5", "--dpmpp_order", "1", "--corruption", "beams:4",
                                            "--corruption", "random_points:0.5"])
    assert (doc["info"]["dpmpp_eta"], doc["info"]["dpmpp_order"], doc["info"]["dpmpp_init"], doc["info"]["dpmpp_t_start"]) == (0.5, 1, "linear", 0.5)
    skipped = doc["results"]["random_points:0.5"]["dpmpp"]
    assert set(skipped) == {"skipped"} and "whole rows" in skipped["skipped"]
    k = torch.load(tmp / "init" / "beams_4.pt")
    x_in, mask, x_out = k["x_in"].to(DEV), k["mask"].to(DEV), k["x_out"]["dpmpp"].to(DEV)
    init = completion.fill_beams(x_in, completion.rows_of_mask(mask), "linear", nodata=-1.0)
    rng = r2dm_amd.setup_rng([completion.scan_seed(SEED, i) for i in range(2)], DEV)
    assert torch.equal(x_out, ddpm.complete_dpm(x_in, mask, 2, order=1, eta=0.5, t_start=0.5, init=init, progress=False, rng=rng))
    with pytest.raises(ValueError):
        completion.evaluate_completion(ddpm, lidar, torch.zeros(1, 6, H, W, device=DEV), ["beams:4"], methods=("dpmpp",), dpmpp_t_start=0.5)
    with pytest.raises(ValueError):
        completion.evaluate_completion(ddpm, lidar, torch.zeros(1, 6, H, W, device=DEV), ["beams:4"], methods=("dpmpp",), dpmpp_order=3)


def test_completion_demo_with_the_dpmpp_method(files):
    tmp, ckpt = files
    (tmp / "demo").mkdir()
    scan_file = next((tmp / "scans").rglob("*.bin"))
    r = subprocess.run([sys.executable, f"{ROOT}/completion_demo.py", "--ckpt", str(ckpt), "--scan", str(scan_file), "--method", "dpmpp", "--num_steps", "2",
                        "--seed", "3"], cwd=tmp / "demo", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    # the default name with the method's own prefix; the size of the RePaint run's image
    assert TL._png_size(tmp / "demo" / "dpmpp_completion_T-0002_r-0016_j-0001.png") == (4 * (W + 2) + 2, 4 * H + 2 * W + 4)
    state = torch.load(tmp / "demo" / "completion.pt")
    on = state["mask"] == 1
    assert state["x_out"].shape == (4, 2, H, W) and torch.equal(state["x_out"][on], state["x_in"][on].clamp(-1, 1))


def test_generate_with_dpm_eta(files):
    tmp, ckpt = files
    out = tmp / "gen.pt"
    r = subprocess.run([sys.executable, f"{ROOT}/generate.py", "--ckpt", str(ckpt), "--batch_size", "1", "--sampling_steps", "2", "--mode", "dpmpp",
                        "--dpm_eta", "1", "--output", str(out)], cwd=tmp, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = torch.load(out)
    assert d["frames"].shape == (3, 1, 2, H, W) and d["points"].shape == (1, 5, H, W)
    assert d["frames"].min() >= 0 and d["frames"].max() <= 1
