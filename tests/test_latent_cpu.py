"""CPU tests of the latent-space feature: the oracle (tests/latent_oracle.py) against closed forms, and the host-side refusals of
``invert`` / ``sample_from`` / ``slerp``.  (The kernels: tests/test_hip_latent.py, -m gpu.)"""
import math

import numpy as np
import pytest
import torch

from conftest import GOLDEN_RES, rnd, synthetic_ckpt

import latent_oracle as LO

from r2dm_amd import latent  # noqa: E402


def rms(a, b):
    return (a.double() - b.double()).pow(2).mean().sqrt().item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_oracle_inversion_converges_at_first_order(dtype):
    """DDIM inversion is Euler's method on the probability-flow ODE.  With the optimal denoiser of x_0 ~ N(0, s^2 I), s = 0.5, the ODE's
    solution is known (latent_oracle.analytic_target), so the loop's error must fall like 1/N: a factor of 4 from 16 to 64 steps;
    asserted: at least 3.  Measured on this input, in float32 and float64 alike: rms 0.0919 at N = 16, 0.0237 at N = 64, ratio 3.87."""
    x_0 = (LO.PRIOR_STD * rnd(7, 3, 2, *GOLDEN_RES)).to(dtype)
    want = LO.analytic_target(x_0)
    e16, e64 = (rms(LO.invert(LO.analytic_eps, x_0, n), want) for n in (16, 64))
    print(f"{dtype}: rms {e16:.4f} at N = 16, {e64:.4f} at N = 64, ratio {e16 / e64:.2f}")
    assert e64 <= e16 / 3, (e16, e64)
    assert 0.01 < e64 < e16 < 0.2  # (neither zero nor off the scale of the data: the target is the one the loop approaches)


def test_oracle_inversion_and_decoding_are_inverse_to_first_order():
    """``sample_from(mode="ddim", clip=None)`` runs the same ODE back, again with Euler steps: the round trip is not exact, its error
    falls at first order too (measured: rms 0.0877 at N = 16, 0.0235 at N = 64)."""
    x_0 = LO.PRIOR_STD * rnd(8, 2, 2, *GOLDEN_RES).double()
    err = []
    for n in (16, 64):
        z = LO.invert(LO.analytic_eps, x_0, n)
        err.append(rms(LO.sample_from(LO.analytic_eps, z, n, mode="ddim", clip=None), x_0))
    assert err[1] <= err[0] / 3, err


def test_slerp_oracle_endpoints_fallback_and_norm():
    """w = 0 gives a and w = 1 gives b up to the float32 rounding of the coefficients; equal and zero inputs take the lerp pair; for
    |a| = |b| every frame has that norm.

    The norm bound: with exact coefficients |c_a a + c_b b|^2 = r^2 (c_a^2 + c_b^2 + 2 c_a c_b cos) = r^2 exactly (the slerp identity).
    The float32 coefficients are off by at most 2^-24 relatively and each output element is two float32 products and one sum, at most
    3 * 2^-24 relative to |c_a a_i| + |c_b b_i|; so |out - exact|_2 <= 4 * 2^-24 (|c_a| + |c_b|) r, and the norms differ by at most
    that (triangle inequality).  The float64 sums behind the coefficients add errors of order 1e-13: nothing next to 2^-24."""
    a, b = LO.slerp_inputs()
    sums = LO.slerp_sums(a.numpy(), b.numpy())
    coef, cos = LO.slerp_coefficients(sums, [0.3])
    assert np.all(np.abs(cos) <= 0.9) and np.allclose(cos, LO.SLERP_COS, atol=0.05), cos  # (what the GPU test's bound needs)
    out, coef = LO.slerp(a.numpy(), b.numpy(), [0.0, 1.0])
    assert np.allclose(coef[0], [1.0, 0.0], atol=1e-15) and np.allclose(coef[1], [0.0, 1.0], atol=1e-15)
    assert np.abs(out[0] - a.numpy()).max() <= 2.0 ** -23 * np.abs(a.numpy()).max() + 1e-12
    assert np.abs(out[1] - b.numpy()).max() <= 2.0 ** -23 * np.abs(b.numpy()).max() + 1e-12
    # the lerp fallback
    w = [0.25, 1.5]
    out, coef = LO.slerp(a.numpy(), a.numpy(), w)
    assert np.array_equal(coef, np.broadcast_to(np.array([[0.75, 0.25], [-0.5, 1.5]])[:, None], coef.shape))
    zero = np.zeros_like(a.numpy())
    for pair in ((zero, b.numpy()), (a.numpy(), zero), (a.numpy(), -a.numpy())):
        assert np.array_equal(LO.slerp(*pair, w)[1], coef)
    # norm preservation
    r = np.sqrt(sums[:, 1])
    b_n = b.numpy() * (r / np.sqrt(sums[:, 2])).astype(np.float32).reshape(-1, 1, 1, 1)
    weights = np.linspace(0.0, 1.0, 7)
    out, coef = LO.slerp(a.numpy(), b_n, weights)
    r_b = np.sqrt(LO.slerp_sums(b_n, b_n)[:, 1])
    assert np.allclose(r_b, r, rtol=1e-6)
    norms = np.sqrt((out.astype(np.float64) ** 2).reshape(len(weights), len(a), -1).sum(-1))
    exact = np.sqrt(coef[..., 0] ** 2 * r ** 2 + coef[..., 1] ** 2 * r_b ** 2 + 2 * coef[..., 0] * coef[..., 1] * LO.slerp_sums(a.numpy(), b_n)[:, 0])
    bound = 4 * 2.0 ** -24 * np.abs(coef).sum(-1) * np.maximum(r, r_b)
    assert np.all(np.abs(norms - exact) <= bound), (np.abs(norms - exact) / bound).max()
    assert np.all(np.abs(exact - r) <= 2e-6 * r)  # (|b| was matched to |a| in float32: r_b = r within 1e-6)


def test_host_refusals():
    """What is refused before anything reaches a kernel: steps outside (0, 1], a non-finite weight, CPU tensors, discrete time."""
    import r2dm_amd
    from r2dm_amd._lib import R2DMError
    from r2dm_amd.diffusion import NoCPUFallback

    x = torch.zeros(1, 2, *GOLDEN_RES)
    ddpm, _, _ = r2dm_amd.setup_model(synthetic_ckpt(resolution=GOLDEN_RES), device="cpu", show_info=False)
    for call in (lambda: ddpm.invert(x, 2, progress=False), lambda: ddpm.sample_from(x, 2, progress=False)):
        with pytest.raises(NoCPUFallback, match="no CPU fallback"):
            call()
    assert issubclass(NoCPUFallback, R2DMError)
    for call in (lambda: latent.ddim_transfer(x, x, torch.zeros(1, 4), "eps"), lambda: latent.slerp(x, x, [0.5]),
                 lambda: latent.interpolate(ddpm, x, x, 3, 2), lambda: latent.reconstruct(ddpm, x, 2)):
        with pytest.raises(R2DMError, match="no CPU fallback"):
            call()
    # the range of t: checked ahead of the device (a fake CUDA model is not needed: the CPU refusal comes first, so patch it away)
    ddpm._refuse_cpu = lambda what, t: None
    for t in (0.0, -0.5, 1.5, math.nan):
        with pytest.raises(ValueError, match="t_end"):
            ddpm.invert(x, 2, t_end=t, progress=False)
        with pytest.raises(ValueError, match="t_start"):
            ddpm.sample_from(x, 2, t_start=t, progress=False)
    for w in ([0.5, math.nan], [math.inf], []):
        with pytest.raises(ValueError):
            latent.slerp(x, x, w)
    with pytest.raises(ValueError):
        latent.interpolate(ddpm, x, x[:, :1], 3, 2)
    disc, _, _ = r2dm_amd.setup_model(synthetic_ckpt(resolution=GOLDEN_RES, timestep_type="discrete", num_training_steps=1000, noise_schedule="linear"), device="cpu", show_info=False)
    assert isinstance(disc, r2dm_amd.DiscreteTimeGaussianDiffusion)
    for call in (lambda: disc.invert(x, 2), lambda: disc.sample_from(x, 2)):
        with pytest.raises(NotImplementedError, match="continuous time"):
            call()


def test_sample_tables_keep_their_keys_and_gain_t_start():
    """``sample``'s table cache keys are what they were; a ``sample_from`` at another ``t_start`` gets a table of its own whose steps start there."""
    import r2dm_amd

    ddpm, _, _ = r2dm_amd.setup_model(synthetic_ckpt(resolution=GOLDEN_RES), device="cpu", show_info=False)
    key = ddpm._table_key(4, 2, "ddim", 0.0, "cpu")
    assert key == ddpm._table_key(4, 2, "ddim", 0.0, "cpu", 1.0) and len(key) == 10
    assert ddpm._table_key(4, 2, "ddim", 0.0, "cpu", 0.5) != key
    row1, _ = ddpm._table_rows(4, 2, "ddim", 0.0, "cpu")
    row5, _ = ddpm._table_rows(4, 2, "ddim", 0.0, "cpu", 0.5)
    c1, c5 = [row1(i)[1] for i in range(4)], [row5(i)[1] for i in range(4)]
    assert torch.equal(torch.stack(c1), ddpm._sample_tables(4, 2, "ddim", 0.0, "cpu")[1])
    want = ddpm._alpha_sigma_rows(torch.linspace(0.5, 0.0, 5))
    assert torch.equal(torch.stack(c5)[:, 0, :2], want[:-1]) and torch.equal(torch.stack(c5)[:, 0, 2:4], want[1:])
    cond, coef = ddpm._transfer_table(torch.linspace(0.0, 0.5, 5), 2, "cpu")
    up = ddpm._alpha_sigma_rows(torch.linspace(0.0, 0.5, 5))
    assert cond.shape == (4, 2) and torch.equal(coef[:, 1], torch.cat([up[:-1], up[1:]], dim=-1))
    assert torch.equal(cond[:, 0], ddpm._log_snr_of_steps(torch.linspace(0.0, 0.5, 5)[:-1]))
