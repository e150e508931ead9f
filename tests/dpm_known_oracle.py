"""The contract of completion and stochastic sampling on DPM-Solver++(2M) (``ContinuousTimeGaussianDiffusion.complete_dpm``,
``sample_dpm(eta=...)``, ``r2dm_dpm_step_known``) restated in plain torch ops (dtype-generic: the dtype of the inputs is the dtype of the run),
on top of ``dpm_oracle`` and the oracle's schedule and forward process (``oracle/r2dm_oracle.py``), both used as they are:

- ``dpm_step_known``  one update: the clamped estimate of x_0, the measurement written over it, ``c_x x + c_0 x0 [+ c_1 x0_prev] [+ c_z z]``;
                      one torch op per float32 operation
- ``table``           ``dpm_oracle.table`` with ``eta``: the rows ``(alpha_t, sigma_t, c_x, c_0, c_1, c_z, 0, 0)``
- ``run``             the loop on a table that is passed in, with the steps' noise tensors and the measurement (either may be None)
- ``complete_dpm``    the completion on an explicit noise tape: one draw for the start, one per step when ``eta > 0``
- ``num_draws``       how many that is"""
import torch

import dpm_oracle as DO
from oracle import r2dm_oracle as O


def dpm_step_known(x, pr, x0_prev, z, y, m, a_t, s_t, c_x, c_0, c_1, c_z, objective, clip=1.0):
    """x_t, prediction, the previous estimate (None: a first-order row), noise (None: none), known and mask (both None: no measurement) and
    the row's scalars (broadcastable tensors) -> (x_s, x0).  The clamp precedes the projection; x0 is the estimate after it."""
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
    if (y is None) != (m is None):
        raise ValueError("known and mask go together")
    if y is not None:
        x0 = m * y + (1.0 - m) * x0
    x_s = c_x * x + c_0 * x0
    if x0_prev is not None:
        x_s = x_s + c_1 * x0_prev
    if z is not None:
        x_s = x_s + c_z * z
    return x_s, x0


def table(num_steps, order=2, grid="logsnr", t_start=1.0, lower_order_final=True, eta=0.0, dtype=torch.float32, log_snr=O.log_snr_cosine):
    """-> (cond (S,), coef (S,8), second) as ``dpm_oracle.table``, whose conditions, alpha_t, sigma_t and choice of second-order rows are
    kept; with ``eta != 0`` the solver's scalars are formed anew from the same log-SNR values in float64, rounded once to ``dtype``:
    c_x = (sigma_s / sigma_t) exp(-eta h), m = -alpha_s expm1(-(1 + eta) h), c_z = sigma_s sqrt(-expm1(-2 eta h)) in slot 5."""
    cond, coef, second = DO.table(num_steps, order, grid, t_start, lower_order_final, dtype, log_snr)
    if eta == 0:
        return cond, coef, second
    l64 = DO.log_snr_grid(num_steps, grid, t_start, dtype, log_snr).double()
    alpha64, sigma64 = l64.sigmoid().sqrt(), (-l64).sigmoid().sqrt()
    h = (l64[1:] - l64[:-1]) / 2
    c_x = sigma64[1:] / sigma64[:-1] * torch.exp(-eta * h)
    m = -alpha64[1:] * torch.special.expm1(-(1 + eta) * h)
    c_z = sigma64[1:] * (-torch.special.expm1(-2 * eta * h)).sqrt()
    c_0, c_1 = m.clone(), torch.zeros_like(m)
    for i in range(num_steps):
        if second[i]:
            r = h[i - 1] / h[i]
            c_0[i] = m[i] * (1 + 1 / (2 * r))
            c_1[i] = -m[i] / (2 * r)
    coef = coef.clone()
    coef[:, 2], coef[:, 3], coef[:, 4], coef[:, 5] = c_x.to(dtype), c_0.to(dtype), c_1.to(dtype), c_z.to(dtype)
    return cond, coef, second


def run(denoise, x, tab, noises=None, known=None, mask=None, objective="eps", clip=1.0, return_all=False):
    """``tab``: (cond (S,) | (S,B), coef (S,8) | (S,B,8), second) -- ``table``'s, or the sampler's ``_dpm_table``.  ``noises``: the S noise
    tensors of the steps, or None (no noise operand: the deterministic solver).  ``clip=None``: no clamp."""
    cond, coef, second = tab
    B, kw = x.shape[0], dict(device=x.device, dtype=x.dtype)
    if noises is not None and len(noises) != len(second):
        raise ValueError(f"{len(second)} steps, {len(noises)} noise tensors")
    out, x0_prev = [x], None
    for i in range(len(second)):
        c = cond[i].to(**kw).expand(B)
        k = coef[i].to(**kw).expand(B, 8)
        a_t, s_t, c_x, c_0, c_1, c_z = (k[:, j][:, None, None, None] for j in range(6))
        z = None if noises is None else noises[i].to(**kw)
        x, x0_prev = dpm_step_known(x, denoise(x, c), x0_prev if second[i] else None, z, known, mask, a_t, s_t, c_x, c_0, c_1, c_z, objective, clip)
        out.append(x)
    return torch.stack(out) if return_all else x


def num_draws(num_steps, eta):
    """the start, and one per step when eta > 0"""
    return 1 + (num_steps if eta > 0 else 0)


def complete_dpm(denoise, known, mask, tab, tape, eta, t_start=1.0, init=None, objective="eps", clip=1.0, exact_known=True, return_all=False,
                 log_snr=O.log_snr_cosine):
    """-> the completed batch; with ``return_all`` the (S+1) stack from the start, the last entry projected like the result.  ``tab`` must be
    the table of ``eta`` and ``t_start``.  ``tape``: a list of noise tensors, consumed in draw order; a tape of another length than
    ``num_draws`` raises ``ValueError``."""
    if init is None and t_start != 1.0:
        raise ValueError("t_start < 1 needs init")
    S = len(tab[2])
    if len(tape) != num_draws(S, eta):
        raise ValueError(f"the loop draws {num_draws(S, eta)} times, the tape holds {len(tape)}")
    B, kw = known.shape[0], dict(device=known.device, dtype=known.dtype)
    first = tape[0].to(**kw)
    x = first if init is None else O.q_step_from_x_0(init, torch.full((B,), t_start, **kw), first, log_snr)
    out = run(denoise, x, tab, list(tape[1:]) if eta > 0 else None, known, mask, objective, clip, return_all=True)
    if exact_known:
        out[-1] = mask * known + (1.0 - mask) * out[-1]
    return out if return_all else out[-1]
