"""DPM-Solver++(2M) without a GPU: the oracle of ``ContinuousTimeGaussianDiffusion.sample_dpm`` (tests/dpm_oracle.py) -- its table against DDIM
and the solver's defining coefficients, its convergence on a denoiser with a closed-form solution -- and what ``sample_dpm`` refuses before
anything reaches a kernel.

What convergence is asserted, and why no more.  The denoiser is ``LO.analytic_eps`` (x_0 ~ N(0, 0.5^2 I)); the exact solution of the
probability-flow ODE from t = 1 to t = 0 is ``LO.analytic_target`` run backwards.  RMS error of the float64 oracle, unclipped:

    grid, lower_order_final=True   N = 8      16        32        64
    logsnr, order 1                1.91e-1    1.04e-1   5.52e-2   2.84e-2
    logsnr, order 2                1.86e-2    1.81e-2   6.30e-3   1.68e-3
    time,   order 1                8.83e-2    4.59e-2   2.34e-2   1.19e-2
    time,   order 2                3.82e-2    1.42e-3   2.85e-3   1.48e-3

The second-order error is not monotone in N at these step sizes (8 -> 16 barely moves on the log-SNR grid, 16 -> 32 doubles on the time
grid), so a ratio of 4 per doubling is NOT asserted.  Asserted, each with a factor 2 of margin on the figures above: on both grids at
N = 32 and 64 order 2 is at least 4 x closer than order 1; on the log-SNR grid the order-2 error at 64 is at most half the one at 32, and
at N = 16 order 2 is at least 3 x closer than order 1.
Recorded, not a bar: with ``lower_order_final=False`` the time grid is WORSE than order 1 (err_1 / err_2 = 0.29, 0.38, 0.67 at N = 8, 16,
32) -- the last log-SNR step of that grid is several times the one before it; that is why the default is True."""
import os

import pytest
import torch

from conftest import GOLDEN_RES, ROOT, rnd, synthetic_ckpt

import dpm_oracle as DO
import latent_oracle as LO

from oracle import r2dm_oracle as O

B = 3
SHAPE = (B, 2, *GOLDEN_RES)
F64 = torch.float64


def rms(a, b):
    return (a.double() - b.double()).pow(2).mean().sqrt().item()


# ---- the table --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t_start", [1.0, 0.5])
@pytest.mark.parametrize("clip", [None, 1.0])
def test_order_1_on_the_time_grid_is_ddim_with_eta_0(t_start, clip):
    """``c_x x + m x0 = alpha_s x0 + sigma_s (x - alpha_t x0) / sigma_t``: the whole float64 loop against the oracle's DDIM loop"""
    S = 8
    x = rnd(11, *SHAPE).double()
    tab = DO.table(S, order=1, grid="time", t_start=t_start, dtype=F64)
    assert not any(tab[2])
    got = DO.sample_dpm(LO.analytic_eps, x, tab, clip=clip, return_all=True)
    want = LO.sample_from(LO.analytic_eps, x, S, t_start, None, "ddim", 0.0, "eps", clip=clip, return_all=True)
    assert got.dtype == F64 and got.shape == (S + 1, *SHAPE)
    for i in range(1, S + 1):
        assert (got[i] - want[i]).abs().max().item() <= 1e-12 * want[i].abs().max().item(), i
    # ... and row by row on the coefficients: c_0 = alpha_s - sigma_s alpha_t / sigma_t
    lam = DO.log_snr_grid(S, "time", t_start, F64)
    a, s = O.alpha_sigma(lam)
    cond, coef, _ = tab
    assert torch.equal(cond, lam[:-1]) and torch.equal(coef[:, 0], a[:-1]) and torch.equal(coef[:, 1], s[:-1])
    torch.testing.assert_close(coef[:, 2], s[1:] / s[:-1], rtol=1e-12, atol=0)
    torch.testing.assert_close(coef[:, 3], a[1:] - s[1:] * a[:-1] / s[:-1], rtol=0, atol=1e-12)
    assert not coef[:, 4:].any()


def test_which_rows_are_first_order():
    S = 6
    for grid in ("logsnr", "time"):
        assert DO.table(S, 2, grid)[2] == [False, True, True, True, True, False]
        assert DO.table(S, 2, grid, lower_order_final=False)[2] == [False, True, True, True, True, True]
        assert DO.table(S, 1, grid)[2] == [False] * S
        assert DO.table(1, 2, grid)[2] == [False] and DO.table(2, 2, grid)[2] == [False, False]
        _, coef, second = DO.table(S, 2, grid, dtype=F64)
        for i in range(S):
            assert (coef[i, 4] != 0) == second[i]
    with pytest.raises(ValueError):
        DO.table(S, 3)
    with pytest.raises(ValueError):
        DO.table(S, 2, "sigma")


def test_a_uniform_log_snr_grid_gives_the_adams_bashforth_pair():
    """r = 1: c_0 = 1.5 m, c_1 = -0.5 m, with m the first-order row's c_0"""
    S = 16
    lam = DO.log_snr_grid(S, "logsnr", dtype=F64)
    assert lam[0].item() == pytest.approx(-15.0, abs=1e-9) and lam[-1].item() == pytest.approx(15.0, abs=1e-9)
    torch.testing.assert_close(lam[1:] - lam[:-1], torch.full((S,), 30.0 / S, dtype=F64), rtol=1e-12, atol=0)
    _, k1, _ = DO.table(S, 1, "logsnr", dtype=F64)
    _, k2, second = DO.table(S, 2, "logsnr", lower_order_final=False, dtype=F64)
    rows = torch.tensor(second)
    assert rows.sum() == S - 1
    m = k1[:, 3]
    torch.testing.assert_close(k2[rows, 3], 1.5 * m[rows], rtol=1e-12, atol=0)
    torch.testing.assert_close(k2[rows, 4], -0.5 * m[rows], rtol=1e-12, atol=0)
    assert torch.equal(k2[:, :3], k1[:, :3]) and torch.equal(k2[0], k1[0])
    # the float32 table: the same numbers rounded once
    _, k32, _ = DO.table(S, 2, "logsnr", lower_order_final=False)
    assert k32.dtype == torch.float32 and (k32.double() - k2).abs().max().item() < 1e-5


def test_the_time_grids_conditions_are_the_reference_samplers():
    """``grid="time"``: the network conditions of ``sample_from`` over ``linspace(t_start, 0, S + 1)``"""
    for t_start in (1.0, 0.5):
        cond, _, _ = DO.table(4, 2, "time", t_start)
        steps = torch.linspace(t_start, 0.0, 5)
        assert torch.equal(cond, torch.cat([O.log_snr_cosine(steps[i:i + 1]) for i in range(4)]))


# ---- convergence on the analytic denoiser ----------------------------------------------------------------------------------------------------
def errors(lower_order_final=True):
    x_0 = (LO.PRIOR_STD * rnd(7, *SHAPE)).double()
    x_1 = DO.exact_start(x_0)
    err = {}
    for grid in ("logsnr", "time"):
        for order in (1, 2):
            for n in (8, 16, 32, 64):
                tab = DO.table(n, order, grid, 1.0, lower_order_final, dtype=F64)
                err[grid, order, n] = rms(DO.sample_dpm(LO.analytic_eps, x_1, tab, clip=None), x_0)
    return err


def check_convergence(err):
    """the conditions of this module's docstring (tests/test_hip_dpm.py applies the N = 32, 64 ones to the float32 run on the GPU)"""
    for grid in ("logsnr", "time"):
        for n in (32, 64):
            assert err[grid, 2, n] <= err[grid, 1, n] / 4, (grid, n, err[grid, 2, n], err[grid, 1, n])
    assert err["logsnr", 2, 64] <= err["logsnr", 2, 32] / 2, err
    if ("logsnr", 2, 16) in err:
        assert err["logsnr", 2, 16] <= err["logsnr", 1, 16] / 3, err


def test_second_order_beats_first_order_on_the_analytic_denoiser():
    err = errors()
    for grid in ("logsnr", "time"):
        for order in (1, 2):
            print(f"{grid}, order {order}: " + "  ".join(f"N={n} {err[grid, order, n]:.3e}" for n in (8, 16, 32, 64)))
    check_convergence(err)
    # recorded, not a bar (the reason for lower_order_final=True)
    raw = errors(lower_order_final=False)
    print("lower_order_final=False, time grid: err_1 / err_2 = " + "  ".join(f"N={n} {raw['time', 1, n] / raw['time', 2, n]:.2f}" for n in (8, 16, 32, 64)))


# ---- what sample_dpm refuses -----------------------------------------------------------------------------------------------------------------
def cpu_model():
    import r2dm_amd

    return r2dm_amd.setup_model(synthetic_ckpt(resolution=GOLDEN_RES), device="cpu", show_info=False)[0]


def test_sample_dpm_on_a_cpu_model_raises_no_cpu_fallback():
    import r2dm_amd
    from r2dm_amd.diffusion import NoCPUFallback

    ddpm = cpu_model()
    state = torch.get_rng_state()
    for kw in ({}, dict(order=1, grid="time"), dict(x_t=torch.zeros(2, 2, *GOLDEN_RES), t_start=0.5, clip=False)):
        with pytest.raises(NoCPUFallback, match="no CPU fallback"):
            ddpm.sample_dpm(2, 4, progress=False, **kw)
    assert torch.equal(torch.get_rng_state(), state)  # (refused before anything is drawn)
    discrete = r2dm_amd.DiscreteTimeGaussianDiffusion(ddpm.model, num_training_steps=10)
    with pytest.raises(NotImplementedError, match="continuous time only"):
        discrete.sample_dpm(2, 4)


def test_sample_dpm_refuses_malformed_arguments():
    ddpm = cpu_model()
    x = torch.zeros(2, 2, *GOLDEN_RES)
    bad = [dict(order=0), dict(order=3), dict(order="2"), dict(grid="sigma"), dict(grid="karras"), dict(num_steps=0), dict(num_steps=-2),
           dict(num_steps=2.5), dict(t_start=0.0, x_t=x), dict(t_start=1.5, x_t=x), dict(t_start=-0.5, x_t=x),
           dict(t_start=0.5),  # (no x_t)
           dict(batch_size=3, x_t=x), dict(x_t=x[0]), dict(batch_size=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            ddpm.sample_dpm(**{"batch_size": 2, "num_steps": 4, "progress": False, **kw})


def test_the_header_declares_the_entry_and_the_scripts_take_the_mode():
    from r2dm_amd import _lib

    header = open(os.path.join(ROOT, "include", "r2dm_hip.h")).read()
    assert "int r2dm_dpm_step(" in header and "r2dm_dpm_step" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["r2dm_dpm_step"][1]) == 11
    import generate
    import interpolate
    import sample_and_save

    assert generate.parser().parse_args(["--ckpt", "c.pth"]).mode == "ddpm"
    assert generate.parser().parse_args(["--ckpt", "c.pth", "--mode", "dpmpp", "--sampling_steps", "20"]).mode == "dpmpp"
    assert sample_and_save.parser().parse_args([]).mode == "ddpm"
    assert sample_and_save.parser().parse_args(["--mode", "dpmpp", "--num_steps", "20"]).mode == "dpmpp"
    assert interpolate.parser().parse_args(["--ckpt", "c.pth"]).decoder == "ddim"
    assert interpolate.parser().parse_args(["--ckpt", "c.pth", "--decoder", "dpmpp"]).decoder == "dpmpp"
    for p in (generate.parser(), sample_and_save.parser()):
        with pytest.raises(SystemExit):
            p.parse_args(["--ckpt", "c.pth", "--mode", "dpm3"])
