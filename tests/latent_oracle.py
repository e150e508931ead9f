"""The contract of the latent-space operators restated in plain torch / numpy (dtype-generic: the dtype of the inputs is the dtype of
the run), on top of the oracle's U-Net, schedules and ``p_step_continuous`` (``oracle/r2dm_oracle.py``, used as it is):

- ``ddim_transfer``   x_t -> x_u along the deterministic DDIM line, x_0 and eps in the direct form of each objective, unclipped
- ``invert``          DDIM inversion over ``linspace(0, t_end, S + 1)``
- ``sample_from``     the reverse loop from a given tensor at ``t_start``, via ``O.p_step_continuous``
- ``slerp``           spherical interpolation per sample with the three sums by ``math.fsum``
- ``slerp_inputs``    the pairs the slerp tests share, and ``analytic_eps`` / ``analytic_target``, the closed-form denoiser of a Gaussian prior"""
import math

import numpy as np
import torch

from conftest import rnd
from oracle import r2dm_oracle as O


def ddim_transfer(x, pr, a_t, s_t, a_u, s_u, objective):
    if objective == "eps":
        e, x0 = pr, (x - s_t * pr) / a_t
    elif objective == "v":
        x0, e = a_t * x - s_t * pr, s_t * x + a_t * pr
    elif objective == "x_0":
        x0, e = pr, (x - a_t * pr) / s_t
    else:
        raise ValueError(objective)
    return a_u * x0 + s_u * e


def invert(denoise, x_0, num_steps, t_end=1.0, objective="eps", log_snr=O.log_snr_cosine, return_all=False):
    B = x_0.shape[0]
    steps = torch.linspace(0.0, t_end, num_steps + 1, device=x_0.device, dtype=x_0.dtype)[None].repeat_interleave(B, dim=0)
    x, out = x_0, [x_0]
    for i in range(num_steps):
        lt, lu = log_snr(steps[:, i]), log_snr(steps[:, i + 1])
        a_t, s_t = O.alpha_sigma(lt[:, None, None, None])
        a_u, s_u = O.alpha_sigma(lu[:, None, None, None])
        x = ddim_transfer(x, denoise(x, lt), a_t, s_t, a_u, s_u, objective)
        out.append(x)
    return torch.stack(out) if return_all else x


def sample_from(denoise, x_t, num_steps, t_start=1.0, noises=None, mode="ddpm", ddim_eta=0.0, objective="eps", clip=1.0,
                log_snr=O.log_snr_cosine, return_all=False):
    """``noises``: the S noise tensors of the steps (None: zeros, for DDIM with eta = 0); ``clip=None``: no clamp."""
    B = x_t.shape[0]
    steps = torch.linspace(t_start, 0.0, num_steps + 1, device=x_t.device, dtype=x_t.dtype)[None].repeat_interleave(B, dim=0)
    x, out = x_t, [x_t]
    for i in range(num_steps):
        noise = torch.zeros_like(x) if noises is None else noises[i].to(device=x.device, dtype=x.dtype)
        x = O.p_step_continuous(denoise, x, steps[:, i], steps[:, i + 1], noise, mode, ddim_eta, objective, log_snr, clip)
        out.append(x)
    return torch.stack(out) if return_all else x


def slerp_sums(a, b):
    """per sample (<a,b>, <a,a>, <b,b>, sum |a_i b_i|): the float32 products, added exactly (math.fsum)"""
    a, b = (np.ascontiguousarray(v, dtype=np.float32).reshape(len(v), -1) for v in (a, b))
    rows = []
    for x, y in zip(a, b):
        ab = (x * y).astype(np.float64)
        rows.append((math.fsum(ab), math.fsum((x * x).astype(np.float64)), math.fsum((y * y).astype(np.float64)), math.fsum(np.abs(ab))))
    return np.array(rows, dtype=np.float64)


def slerp_coefficients(sums, weights):
    """(K,B,2) float64 (c_a, c_b) and (B,) cos from the rows of ``slerp_sums``"""
    coef, cos = np.empty((len(weights), len(sums), 2)), np.zeros(len(sums))
    for j, (ab, aa, bb, _) in enumerate(sums):
        lerp = not (aa > 0.0 and bb > 0.0)
        if not lerp:
            cos[j] = min(1.0, max(-1.0, ab / math.sqrt(aa * bb)))
            lerp = 1.0 - cos[j] * cos[j] < 1e-10
        for k, w in enumerate(weights):
            w = float(np.float32(w))
            if lerp:
                coef[k, j] = 1.0 - w, w
            else:
                omega = math.acos(cos[j])
                coef[k, j] = math.sin((1.0 - w) * omega) / math.sin(omega), math.sin(w * omega) / math.sin(omega)
    return coef, cos


def slerp(a, b, weights):
    """-> out (K,B,...) float32 = fl32(c_a) * a + fl32(c_b) * b, coef64 (K,B,2)"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    coef, _ = slerp_coefficients(slerp_sums(a, b), weights)
    c = coef.astype(np.float32).reshape(len(weights), len(a), 2, *([1] * (a.ndim - 1)))
    return c[:, :, 0] * a[None] + c[:, :, 1] * b[None], coef


SLERP_COS = (0.0, 0.6, -0.8)  # the cosines the three samples of ``slerp_inputs`` are built around


def slerp_inputs(shape=(3, 2, 16, 128), seed=40):
    """(a, b) float32 CPU tensors with cos(a_j, b_j) near SLERP_COS[j]: b = c a + sqrt(1 - c^2) n with an independent n"""
    a, n = rnd(seed, *shape), rnd(seed + 1, *shape)
    c = torch.tensor([SLERP_COS[j % len(SLERP_COS)] for j in range(shape[0])]).reshape(-1, *([1] * (len(shape) - 1)))
    return a, c * a + (1 - c * c).sqrt() * n


# ---- the optimal denoiser of x_0 ~ N(0, s^2 I): the probability-flow ODE has a closed form -----------------------------------
PRIOR_STD = 0.5


def analytic_eps(x, log_snr, s=PRIOR_STD):
    """eps* = sigma_t x / (alpha_t^2 s^2 + sigma_t^2)  (``log_snr``: (B,), the network condition)"""
    a2, s2 = log_snr.sigmoid()[:, None, None, None], (-log_snr).sigmoid()[:, None, None, None]
    return s2.sqrt() * x / (a2 * s * s + s2)


def analytic_target(x_0, t_end=1.0, s=PRIOR_STD, log_snr=O.log_snr_cosine):
    """The exact solution of the inversion ODE under ``analytic_eps``: x scales with the marginal's standard deviation,
    x(t_end) = x_0 sqrt((alpha_1^2 s^2 + sigma_1^2) / (alpha_0^2 s^2 + sigma_0^2)), evaluated in float64"""
    l0, l1 = (log_snr(torch.tensor([t], dtype=torch.float64)) for t in (0.0, t_end))
    var = lambda l: l.sigmoid() * s * s + (-l).sigmoid()
    return x_0.double() * (var(l1) / var(l0)).sqrt().item()
