"""The contract of the DPM-Solver++(2M) sampler (``ContinuousTimeGaussianDiffusion.sample_dpm``, ``r2dm_dpm_step``) restated in plain torch ops
(dtype-generic: the dtype of the inputs is the dtype of the run), on top of the oracle's schedule (``oracle/r2dm_oracle.py``, used as it is):

- ``dpm_step``     one update: the clamped estimate of x_0, then ``c_x x + c_0 x0 [+ c_1 x0_prev]``; one torch op per float32 operation
- ``log_snr_grid`` the S + 1 log-SNR values of a run, uniform in log-SNR or in time
- ``table``        the rows ``(alpha_t, sigma_t, c_x, c_0, c_1, 0, 0, 0)`` and which of them are second-order
- ``sample_dpm``   the loop on a table that is passed in (the oracle's own or the sampler's)
- ``exact_start``  the start tensor whose probability-flow ODE solution under ``latent_oracle.analytic_eps`` is known in closed form"""
import torch

import latent_oracle as LO
from oracle import r2dm_oracle as O


def dpm_step(x, pr, x0_prev, a_t, s_t, c_x, c_0, c_1, objective, clip=1.0):
    """x_t, prediction, the previous estimate (None: a first-order row) and the row's scalars (broadcastable tensors) -> (x_s, x0)"""
    if objective == "eps":
        x0 = (x - s_t * pr) / a_t
    elif objective == "v":
        x0 = a_t * x - s_t * pr
    elif objective == "x_0":
        x0 = pr
    else:
        raise ValueError(objective)
    if clip is not None and clip >= 0:
        x0 = x0.clamp(-clip, clip)
    x_s = c_x * x + c_0 * x0
    if x0_prev is not None:
        x_s = x_s + c_1 * x0_prev
    return x_s, x0


def _rowwise(f, t):
    """``f`` on 1-element tensors, one row at a time: torch's CPU kernels round the last bit differently in their SIMD body and in their
    scalar tail, and the sampler's host tables are evaluated this way (``_coefficients``)"""
    return torch.cat([f(t[i:i + 1]) for i in range(t.numel())])


def log_snr_grid(num_steps, grid="logsnr", t_start=1.0, dtype=torch.float32, log_snr=O.log_snr_cosine):
    if grid == "time":
        return _rowwise(log_snr, torch.linspace(t_start, 0.0, num_steps + 1, dtype=dtype))
    if grid == "logsnr":
        ends = _rowwise(log_snr, torch.tensor([t_start, 0.0], dtype=dtype))
        return torch.linspace(ends[0].item(), ends[1].item(), num_steps + 1, dtype=dtype)
    raise ValueError(grid)


def table(num_steps, order=2, grid="logsnr", t_start=1.0, lower_order_final=True, dtype=torch.float32, log_snr=O.log_snr_cosine):
    """-> (cond (S,), coef (S,8), second: list of S bools).  alpha_t, sigma_t: the oracle's ``alpha_sigma`` of the log-SNR in ``dtype``; the
    solver's scalars: from those log-SNR values in float64, rounded once to ``dtype``."""
    if order not in (1, 2):
        raise ValueError(order)
    S = num_steps
    lam = log_snr_grid(S, grid, t_start, dtype, log_snr)
    a_t, s_t = (_rowwise(lambda l, k=k: O.alpha_sigma(l)[k], lam[:-1]) for k in (0, 1))
    l64 = lam.double()
    alpha64, sigma64 = l64.sigmoid().sqrt(), (-l64).sigmoid().sqrt()
    h = (l64[1:] - l64[:-1]) / 2
    c_x = sigma64[1:] / sigma64[:-1]
    m = -alpha64[1:] * torch.special.expm1(-h)
    second = [order == 2 and i > 0 and not (lower_order_final and i == S - 1) for i in range(S)]
    c_0, c_1 = m.clone(), torch.zeros_like(m)
    for i in range(S):
        if second[i]:
            r = h[i - 1] / h[i]
            c_0[i] = m[i] * (1 + 1 / (2 * r))
            c_1[i] = -m[i] / (2 * r)
    zero = torch.zeros(S, dtype=dtype)
    coef = torch.stack([a_t, s_t, c_x.to(dtype), c_0.to(dtype), c_1.to(dtype), zero, zero, zero], dim=-1)
    return lam[:-1], coef, second


def sample_dpm(denoise, x, tab, objective="eps", clip=1.0, return_all=False):
    """``tab``: (cond (S,) | (S,B), coef (S,8) | (S,B,8), second) -- ``table``'s, or the sampler's ``_dpm_table``.  ``clip=None``: no clamp."""
    cond, coef, second = tab
    B, kw = x.shape[0], dict(device=x.device, dtype=x.dtype)
    out, x0_prev = [x], None
    for i in range(len(second)):
        c = cond[i].to(**kw).expand(B)
        k = coef[i].to(**kw).expand(B, 8)
        a_t, s_t, c_x, c_0, c_1 = (k[:, j][:, None, None, None] for j in range(5))
        x, x0_prev = dpm_step(x, denoise(x, c), x0_prev if second[i] else None, a_t, s_t, c_x, c_0, c_1, objective, clip)
        out.append(x)
    return torch.stack(out) if return_all else x


def exact_start(x_0, t_start=1.0):
    """x(t_start) of the probability-flow ODE through ``x_0`` at t = 0 under ``LO.analytic_eps`` (float64): ``LO.analytic_target``, whose
    solution run backwards from there ends in ``x_0``"""
    return LO.analytic_target(x_0, t_start)
