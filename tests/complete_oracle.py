"""The contract of data-consistent completion (``ContinuousTimeGaussianDiffusion.complete``, ``r2dm_posterior_step_known``) restated in plain
torch ops (dtype-generic: the dtype of the inputs is the dtype of the run), on top of the oracle's schedule and forward process
(``oracle/r2dm_oracle.py``, used as it is):

- ``posterior_known``   one reverse update with the measurement written over the clamped x_0 estimate; one torch op per float32 operation
- ``p_step_known``      the denoiser call at log-SNR(t) and that update
- ``complete``          the loop on an explicit noise tape: RePaint's schedule over ``linspace(t_start, 0, S + 1)``, one draw for the start,
                        one per denoiser call, one per forward sub-step; the tape must hold exactly the draws the loop makes
- ``num_draws``         how many that is"""
import torch

from oracle import r2dm_oracle as O


def posterior_known(x, pr, z, y, m, a_t, s_t, a_s, c, sd, c1, c2, mode, objective, clip=1.0):
    """x_t, prediction, noise, known, mask and the step's scalars (broadcastable tensors) -> x_s.  The clamp precedes the projection."""
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
    x0 = m * y + (1.0 - m) * x0
    if mode == "ddpm":
        return a_s * (x * (1.0 - c) / a_t + c * x0) + sd * z
    if mode == "ddim":
        return a_s * x0 + c1 * z + c2 * ((x - a_t * x0) / s_t)
    raise ValueError(mode)


def step_scalars(step_t, step_s, mode, ddim_eta, log_snr=O.log_snr_cosine):
    """(log-SNR(t) (B,), the scalars of ``posterior_known`` as (B,1,1,1) tensors), with the expressions of ``O.p_step_continuous``"""
    v4 = lambda t: t[:, None, None, None]
    lt, ls = v4(log_snr(step_t)), v4(log_snr(step_s))
    a_t, s_t = O.alpha_sigma(lt)
    a_s, s_s = O.alpha_sigma(ls)
    zero = torch.zeros_like(lt)
    if mode == "ddpm":
        c = -torch.special.expm1(lt - ls)
        return lt[:, 0, 0, 0], dict(a_t=a_t, s_t=s_t, a_s=a_s, c=c, sd=s_s * c.sqrt(), c1=zero, c2=zero)
    if mode == "ddim":
        c1 = ddim_eta * s_s / s_t * (1 - a_t**2 / a_s**2).sqrt()
        c2 = (1 - a_s**2 - c1**2).sqrt()
        return lt[:, 0, 0, 0], dict(a_t=a_t, s_t=s_t, a_s=a_s, c=zero, sd=zero, c1=c1, c2=c2)
    raise ValueError(mode)


def p_step_known(denoise, x_t, known, mask, step_t, step_s, noise, mode="ddpm", ddim_eta=0.0, objective="eps", clip=1.0, log_snr=O.log_snr_cosine):
    cond, k = step_scalars(step_t, step_s, mode, ddim_eta, log_snr)
    return posterior_known(x_t, denoise(x_t, cond), noise, known, mask, mode=mode, objective=objective, clip=clip, **k)


def num_draws(num_steps, num_resample_steps=1, jump_length=1):
    """the start, ``jump_length`` per group of reverse sub-steps, ``jump_length`` per travel back (none after a step's last resampling, none
    on the last step)"""
    groups = (num_steps - 1) * num_resample_steps + 1
    return 1 + jump_length * groups + jump_length * (num_steps - 1) * (num_resample_steps - 1)


def complete(denoise, known, mask, num_steps, tape, num_resample_steps=1, jump_length=1, t_start=1.0, init=None, mode="ddpm", ddim_eta=0.0,
             objective="eps", exact_known=True, return_all=False, clip=1.0, log_snr=O.log_snr_cosine):
    """-> the completed batch; with ``return_all`` the stack of the start and the x_s of every resampling, the last one projected like the
    result.  ``tape``: a list of noise tensors, consumed in draw order; a tape of another length than ``num_draws`` raises ``ValueError``."""
    if init is None and t_start != 1.0:
        raise ValueError("t_start < 1 needs init")
    want = num_draws(num_steps, num_resample_steps, jump_length)
    if len(tape) != want:
        raise ValueError(f"the loop draws {want} times, the tape holds {len(tape)}")
    it = iter(tape)
    nxt = lambda: next(it).to(device=known.device, dtype=known.dtype)
    B, kw = known.shape[0], dict(device=known.device, dtype=known.dtype)
    if init is None:
        x_t = nxt()
    else:
        x_t = O.q_step_from_x_0(init, torch.full((B,), t_start, **kw), nxt(), log_snr)
    out = [x_t]
    steps = torch.linspace(t_start, 0.0, num_steps + 1, **kw)[None].repeat_interleave(B, dim=0)
    x_s = x_t
    for i in range(num_steps):
        t, s = steps[:, [i]], steps[:, [i + 1]]
        r = t + torch.linspace(0, 1, jump_length + 1, **kw)[None] * (s - t)
        for j in range(num_resample_steps):
            x = x_t
            for k in range(jump_length):  # t -> s
                x = p_step_known(denoise, x, known, mask, r[:, k], r[:, k + 1], nxt(), mode, ddim_eta, objective, clip, log_snr)
            x_s = x
            out.append(x_s)
            if i == num_steps - 1 or j == num_resample_steps - 1:
                x_t = x
                break
            for k in range(jump_length, 0, -1):  # s -> t
                x = O.q_step(x, r[:, k - 1], r[:, k], nxt(), log_snr)
            x_t = x
    assert next(it, None) is None
    if exact_known:  # the final projection is separate from the loop's last x_s: (known * 1 + known * 0) is known
        x_s = mask * known + (1.0 - mask) * x_s
        out[-1] = x_s
    return torch.stack(out) if return_all else x_s
