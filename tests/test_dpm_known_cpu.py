"""CPU: the contract of completion and stochastic sampling on DPM-Solver++(2M) as tests/dpm_known_oracle.py states it -- the table's two
identities, the EXACT output variance of the stochastic solver on a Gaussian prior (the loop is linear: its variance is read off a basis,
no sampling error), and the wiring (header, ``_lib.SIGNATURES``, ``completion.METHODS``, the scripts' options, what ``complete_dpm`` refuses
before it needs a GPU).

Exact variance.  With ``latent_oracle.analytic_eps`` (the optimal denoiser of x_0 ~ N(0, 0.25 I)) and no clamp every step is linear in
(x, x0_prev, z), so the result is ``g_0 x_1 + sum_j g_j z_j`` per element and its variance under a unit-variance start and unit noises is
``v = sum g^2``; the true marginal at t = 0 has variance ~0.25.  ``e(S) = |v / 0.25 - 1|`` is the solver's error in the one statistic a
Gaussian has.  Found, float64, eta = 1 on the log-SNR grid: e_2 = 0.061, 0.018, 0.0046 at S = 32, 64, 128 against e_1 = 0.35, 0.20, 0.11; the
successive ratios of e_2 are 3.4-3.9 at every eta (second order: 4 in the limit), asserted with a factor 2."""
import os

import pytest
import torch

from conftest import GOLDEN_RES, ROOT, synthetic_ckpt

import complete_oracle as CO
import dpm_known_oracle as KO
import dpm_oracle as DO
import latent_oracle as LO

ETAS = [0.0, 0.5, 1.0]
STEPS = [16, 32, 64, 128]


# ---- a. the table's identities ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("grid", ["logsnr", "time"])
@pytest.mark.parametrize("order", [1, 2])
def test_the_eta_0_table_is_dpm_oracles(order, grid, dtype):
    for S, t_start, lof in ((4, 1.0, True), (9, 0.5, False)):
        got, want = KO.table(S, order, grid, t_start, lof, 0.0, dtype), DO.table(S, order, grid, t_start, lof, dtype)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2] == want[2] and not got[1][:, 5:].any()
        # ... and eta only moves the solver's scalars: conditions, alpha_t, sigma_t and the choice of rows stay
        moved = KO.table(S, order, grid, t_start, lof, 1.0, dtype)
        assert torch.equal(moved[0], want[0]) and torch.equal(moved[1][:, :2], want[1][:, :2]) and moved[2] == want[2]
        assert (moved[1][:, 5] > 0).all() and not moved[1][:, 6:].any() and (moved[1][:, 2] < want[1][:, 2]).all()


@pytest.mark.parametrize("t_start", [1.0, 0.5])
def test_order_1_eta_1_rows_are_the_ancestral_posteriors_scalars(t_start):
    """float64, the time grid (the ancestral sampler's).  With c = 1 - exp(-2 h) = -expm1(lambda_t - lambda_s): c_x = alpha_s (1 - c) / alpha_t,
    m = alpha_s c, c_z = sigma_s sqrt(c).  Tolerance: m and c_z are products of a few correctly rounded float64 values -- 1e-14 relative;
    the ancestral form of c_x goes through ``1 - c``, which carries up to an ulp of ONE whatever its size (c -> 1 on the last step), so it
    is compared within 4 ulp of one times alpha_s / alpha_t on top of that."""
    S = 8
    _, coef, second = KO.table(S, 1, "time", t_start, True, 1.0, torch.float64)
    assert not any(second)
    steps = torch.linspace(t_start, 0.0, S + 1, dtype=torch.float64)
    _, k = CO.step_scalars(steps[:-1], steps[1:], "ddpm", 0.0)
    a_t, a_s, c, sd = (k[n].flatten() for n in ("a_t", "a_s", "c", "sd"))
    eps = torch.finfo(torch.float64).eps
    want_cx = a_s * (1.0 - c) / a_t
    err_cx, err_m, err_cz = (coef[:, 2] - want_cx).abs(), (coef[:, 3] / (a_s * c) - 1).abs(), (coef[:, 5] / sd - 1).abs()
    print(f"t_start {t_start}: c_x abs err max {err_cx.max():.2e} (1 - c down to {(1 - c).min():.2e}), m rel {err_m.max():.2e}, c_z rel {err_cz.max():.2e}")
    assert (err_cx <= 4 * eps * a_s / a_t + 1e-14 * want_cx).all()
    assert err_m.max() <= 1e-14 and err_cz.max() <= 1e-14
    assert torch.equal(coef[:, 4], torch.zeros(S, dtype=torch.float64))


# ---- b. exact variance on a Gaussian prior -------------------------------------------------------------------------------------------------------
def output_variance(S, order, grid, eta):
    """the loop on the basis: row 0 carries the unit start, row j the unit noise of step j (rows are independent: every op is per sample)"""
    tab = KO.table(S, order, grid, 1.0, True, eta, torch.float64)
    n = S + 1 if eta > 0 else 1
    x = torch.zeros(n, 1, 1, 1, dtype=torch.float64)
    x[0] = 1.0
    noises = None
    if eta > 0:
        noises = [torch.zeros_like(x) for _ in range(S)]
        for j in range(S):
            noises[j][j + 1] = 1.0
    g = KO.run(LO.analytic_eps, x, tab, noises, objective="eps", clip=None)
    return float((g.flatten() ** 2).sum())


@pytest.fixture(scope="module")
def variance_errors():
    prior = LO.PRIOR_STD ** 2
    return {(grid, eta, order, S): abs(output_variance(S, order, grid, eta) / prior - 1.0)
            for grid in ("logsnr", "time") for eta in ETAS for order in (1, 2) for S in STEPS}


@pytest.mark.parametrize("eta", ETAS)
def test_second_order_halves_the_variance_error_per_doubling_on_the_log_snr_grid(variance_errors, eta):
    e = variance_errors
    for S in STEPS:
        print(f"logsnr eta {eta} S={S}: e_1 {e['logsnr', eta, 1, S]:.4f}  e_2 {e['logsnr', eta, 2, S]:.4f}")
    for S in STEPS:
        assert e["logsnr", eta, 2, S] < e["logsnr", eta, 1, S], S
    assert e["logsnr", eta, 2, 64] < e["logsnr", eta, 2, 32] / 2
    assert e["logsnr", eta, 2, 128] < e["logsnr", eta, 2, 64] / 2


@pytest.mark.parametrize("eta", ETAS)
def test_second_order_beats_first_order_on_the_time_grid(variance_errors, eta):
    e = variance_errors
    for S in STEPS:
        print(f"time eta {eta} S={S}: e_1 {e['time', eta, 1, S]:.4f}  e_2 {e['time', eta, 2, S]:.4f}")
        assert e["time", eta, 2, S] < e["time", eta, 1, S], S


def test_the_oracles_loops_agree_with_each_other():
    """no noise and no measurement is ``dpm_oracle.sample_dpm``; an all-zero mask is no measurement; the tape's length is checked"""
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(2, 2, 4, 8, generator=g, dtype=torch.float64), torch.randn(2, 2, 4, 8, generator=g, dtype=torch.float64).tanh()
    tab = KO.table(5, 2, "logsnr", 1.0, True, 0.0, torch.float64)
    assert torch.equal(KO.run(LO.analytic_eps, x, tab), DO.sample_dpm(LO.analytic_eps, x, tab))
    zero, one = torch.zeros(2, 1, 4, 8, dtype=torch.float64), torch.ones(2, 1, 4, 8, dtype=torch.float64)
    tab1 = KO.table(5, 2, "logsnr", 1.0, True, 1.0, torch.float64)
    tape = [torch.randn(2, 2, 4, 8, generator=g, dtype=torch.float64) for _ in range(6)]
    free = KO.run(LO.analytic_eps, tape[0], tab1, tape[1:])
    assert torch.equal(KO.complete_dpm(LO.analytic_eps, y, zero, tab1, tape, 1.0), free)
    assert torch.equal(KO.complete_dpm(LO.analytic_eps, y, one, tab1, tape, 1.0), y)
    assert not torch.equal(KO.complete_dpm(LO.analytic_eps, y, one, tab1, tape, 1.0, exact_known=False), y)
    with pytest.raises(ValueError):
        KO.complete_dpm(LO.analytic_eps, y, zero, tab1, tape[:-1], 1.0)
    with pytest.raises(ValueError):
        KO.complete_dpm(LO.analytic_eps, y, zero, tab, tape, 0.0)  # (eta = 0 draws once)
    assert KO.num_draws(5, 0.0) == 1 and KO.num_draws(5, 0.5) == 6


# ---- c. wiring ----------------------------------------------------------------------------------------------------------------------------------
def cpu_model():
    import r2dm_amd

    return r2dm_amd.setup_model(synthetic_ckpt(resolution=GOLDEN_RES), device="cpu", show_info=False)[0]


def test_the_header_declares_the_entry_and_the_callers_take_the_method():
    from r2dm_amd import _lib, completion

    header = open(os.path.join(ROOT, "include", "r2dm_hip.h")).read()
    assert "int r2dm_dpm_step_known(" in header
    decl = header[header.index("int r2dm_dpm_step_known("):]
    assert decl[:decl.index(";")].count(",") == 15
    assert len(_lib.SIGNATURES["r2dm_dpm_step_known"][1]) == 16 and len(_lib.SIGNATURES["r2dm_dpm_step"][1]) == 11
    assert "dpmpp" in completion.METHODS and {"repaint", "ddnm"} <= set(completion.METHODS)
    import completion_demo
    import completion_eval
    import generate
    import sample_and_save

    a = completion_eval.build_parser().parse_args(["--ckpt", "c.pth", "--real_scans", "d"])
    assert "dpmpp" not in a.methods and completion_eval.dpmpp_settings(a) == {"dpmpp_eta": 1.0, "dpmpp_order": 2, "dpmpp_init": "none", "dpmpp_t_start": 1.0}
    a = completion_eval.build_parser().parse_args(["--ckpt", "c.pth", "--real_scans", "d", "--methods", "dpmpp", "linear", "--dpmpp_eta", "0.5", "--dpmpp_order", "1"])
    assert a.methods == ["dpmpp", "linear"] and completion_eval.dpmpp_settings(a) == {"dpmpp_eta": 0.5, "dpmpp_order": 1, "dpmpp_init": "none", "dpmpp_t_start": 1.0}
    with pytest.raises(SystemExit):
        completion_eval.build_parser().parse_args(["--ckpt", "c.pth", "--dpmpp_order", "3"])
    a = completion_demo.parser().parse_args(["--ckpt", "c.pth", "--scan", "s.bin", "--method", "dpmpp", "--dpmpp_eta", "0"])
    assert a.method == "dpmpp" and a.dpmpp_eta == 0.0
    assert completion_demo.parser().parse_args(["--ckpt", "c.pth", "--scan", "s.bin"]).method == "repaint"
    for mod, base in ((generate, ["--ckpt", "c.pth"]), (sample_and_save, [])):
        assert mod.parser().parse_args(base).dpm_eta == 0.0
        assert mod.parser().parse_args(base + ["--mode", "dpmpp", "--dpm_eta", "1"]).dpm_eta == 1.0


def test_complete_dpm_refuses_malformed_arguments_before_it_refuses_the_cpu():
    import r2dm_amd
    from r2dm_amd.diffusion import NoCPUFallback

    ddpm = cpu_model()
    H, W = GOLDEN_RES
    known, mask = torch.zeros(2, 2, H, W), torch.ones(2, 1, H, W)
    state = torch.get_rng_state()
    bad = [dict(known=known[0]), dict(known=known[:, :1]), dict(mask=mask[0]), dict(mask=torch.ones(3, 1, H, W)), dict(mask=torch.ones(2, 3, H, W)),
           dict(mask=mask[..., :-1]), dict(num_steps=0), dict(num_steps=2.5), dict(order=3), dict(order=0), dict(grid="sigma"), dict(eta=-0.5),
           dict(eta=float("nan")), dict(eta=float("inf")), dict(t_start=0.0, init=known), dict(t_start=1.5, init=known), dict(t_start=0.5),
           dict(init=known[:1])]
    for kw in bad:
        with pytest.raises(ValueError):
            ddpm.complete_dpm(**{"known": known, "mask": mask, "num_steps": 4, "progress": False, **kw})
    with pytest.raises(TypeError):
        ddpm.complete_dpm(known, mask, 4, num_resample_steps=2)  # (no resampling on the multistep solver)
    for kw in ({}, dict(eta=0.0, order=1, grid="time"), dict(t_start=0.5, init=known)):
        with pytest.raises(NoCPUFallback, match="no CPU fallback"):
            ddpm.complete_dpm(known, mask, 4, progress=False, **kw)
    for kw in (dict(eta=-1.0), dict(eta=float("nan"))):
        with pytest.raises(ValueError):
            ddpm.sample_dpm(2, 4, progress=False, **kw)
    with pytest.raises(NoCPUFallback):
        ddpm.sample_dpm(2, 4, progress=False, eta=1.0)
    assert torch.equal(torch.get_rng_state(), state)  # (refused before anything is drawn)
    discrete = r2dm_amd.DiscreteTimeGaussianDiffusion(ddpm.model, num_training_steps=10)
    with pytest.raises(NotImplementedError, match="continuous time only"):
        discrete.complete_dpm(known, mask, 4)


def test_the_samplers_table_takes_eta_and_keeps_its_eta_0_rows():
    """the host table needs no GPU: eta = 0 is the table of before (the same call without the keyword: one cached object per key), and the eta
    rows are the oracle's within one float32 ulp"""
    ddpm = cpu_model()
    for grid in ("logsnr", "time"):
        for order in (1, 2):
            base = ddpm._dpm_table(6, 2, order, grid, 1.0, True, "cpu")
            assert len(base) == 3 and ddpm._dpm_table(6, 2, order, grid, 1.0, True, "cpu", eta=0.0) is base
            o = DO.table(6, order, grid)
            assert torch.equal(base[1][:, 0, :2], o[1][:, :2]) and not base[1][..., 5:].any()
            assert (base[1][:, 0, 2:5].contiguous().view(torch.int32) - o[1][:, 2:5].contiguous().view(torch.int32)).abs().max() <= 1
            for eta in (0.5, 1.0):
                cond, coef, second = ddpm._dpm_table(6, 2, order, grid, 1.0, True, "cpu", eta=eta)
                assert coef is not base[1] and torch.equal(cond, base[0]) and torch.equal(second, base[2])
                ko = KO.table(6, order, grid, 1.0, True, eta)
                assert torch.equal(coef[:, 0, :2], ko[1][:, :2]) and torch.equal(coef[:, 0], coef[:, 1]) and not coef[..., 6:].any()
                ulps = (coef[:, 0, 2:6].contiguous().view(torch.int32) - ko[1][:, 2:6].contiguous().view(torch.int32)).abs()
                assert ulps.max().item() <= 1, (grid, order, eta, ulps)
