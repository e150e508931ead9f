"""Reverse-process samplers with the reference's API surface.

Mirrors (names, arguments, draw order, error behaviour):
  /root/reference/models/diffusion/base.py:8-163            GaussianDiffusion
  /root/reference/models/diffusion/continuous_time.py:66-317 ContinuousTimeGaussianDiffusion
  /root/reference/models/diffusion/discrete_time.py:51-201   DiscreteTimeGaussianDiffusion

MI355X design, not a translation:
  * All per-step schedule scalars (log-SNR, alpha, sigma, c, ...) are evaluated once, on the
    host, with the same float32 torch ops the reference uses, and uploaded as one table; the
    step loop itself launches no scalar kernels and never synchronises.
  * The posterior update ``x_t, prediction, noise -> x_s`` is ONE fused HIP kernel
    (``r2dm_posterior_step``) that replays the reference's float32 operation order with FMA
    contraction off.
  * Noise stays in ``torch.randn(generator=...)`` so that seeds mean what they mean in the
    reference (base.py:71-94).

Every sampler is one of two walks.  ``_run_loop`` is the step loop of ``sample``, ``sample_from``, ``invert``, ``sample_dpm`` and
``complete_dpm``: one denoiser call and one fused update per step (``r2dm_posterior_step``, ``r2dm_ddim_transfer``, ``r2dm_dpm_step[_known]``),
with ``_Replay``'s recovery from a range-guard trip.  ``_resample_walk`` is the RePaint schedule of ``repaint`` and ``complete``
(``r2dm_posterior_step_known``): sub-steps, travel back through ``q_step``, resample.  Host-side schedule scalars all go through ``_rows``.

The denoising loss ``ddpm(x_0, loss_mask)`` (base.py:122-149) is evaluated forward-only: one noising (``r2dm_q_step``), one denoiser
call and one fused HIP reduction (``r2dm_diffusion_loss``); there is no autograd and no optimizer here.
"""
from __future__ import annotations

import contextlib
import math
from functools import partial
from typing import List, Literal, Optional

import os

import torch
from torch import nn
from torch.special import expm1

from . import _lib
from .latent import ddim_transfer as _ddim_transfer
from .unet import step_is_full

try:  # progress bars are optional
    from tqdm.auto import tqdm
except Exception:  # pragma: no cover
    def tqdm(it, **_):
        return it

# posterior kernel modes (csrc/posterior.hip)
_M_CT_DDPM, _M_CT_DDIM, _M_DT_DDPM, _M_DT_DDIM, _M_DT_DDIM_NOISE = 0, 1, 2, 3, 4
_NCOEF = 8
_CRITERIA = ("l2", "l1", "huber")  # base.py:39-44


class NoCPUFallback(_lib.R2DMError, NotImplementedError):
    """The denoising loss, ``invert`` or ``sample_from`` was asked of a model or an image batch that is not on a GPU: an ``R2DMError`` like every other entry point's
    refusal, and a ``NotImplementedError`` for callers of the earlier sampling-only package, whose ``forward`` raised that."""


# --------------------------------------------------------------------------------------
# log-SNR schedules (continuous_time.py:14-63).  Evaluated on the HOST in float32.
# --------------------------------------------------------------------------------------
def _range_guard(model):
    """The denoiser's deferred fp16-range check (EfficientUNet.deferred_range_check) around a sampling loop: one
    synchronising check at the end instead of one per step; a no-op for any other denoiser."""
    guard = getattr(model, "deferred_range_check", None)
    return guard() if callable(guard) else contextlib.nullcontext()


def _early_range_check(model, num_steps: int) -> bool:
    """One synchronising range check after the first denoiser call of a loop (one sync per ``sample`` call).  True = the guard
    tripped and the denoiser switched itself to the wide-range operand split (EfficientUNet.check_range_or_fall_back): the
    caller repeats that call.  With ``strict_range`` a tripped guard raises, and short loops (<= 8 steps) skip the early
    check -- the deferred one at the loop's end reports it."""
    model = getattr(model, "_orig_mod", model)  # (torch.compile wrapper)
    check = getattr(model, "check_range_or_fall_back", None)
    if not callable(check):
        return False
    if getattr(model, "strict_range", False) and num_steps <= 8:
        return False
    return check()


_NO_CACHE_IN_RESAMPLING = ("the resampling walk jumps back in time, and deep features cached at a later noise level are not a neighbouring step's; "
                           "complete_dpm (no resampling) takes a feature cache")

_CHECK_EVERY = 32  # steps between two range checks of a sampling loop: one stream synchronisation each, at most so many steps to replay


class _Replay:
    """Recovery from a range-guard trip at ANY step of a ``sample`` loop (missing #2; the reference samples any
    finite checkpoint, /root/reference/models/diffusion/continuous_time.py:246-257).  The loop keeps ``x`` of the last step whose
    check passed and the noise it has drawn since; after step 0 of a longer loop, every ``_CHECK_EVERY`` steps and at the end the
    denoiser's guard is read (EfficientUNet.check_range_or_fall_back); on a trip the denoiser has switched itself to the wide-range
    operand split (one RuntimeWarning) and the loop goes back to that ``x`` and runs the steps since on the RECORDED noise -- same
    draws, no exception, at most ``_CHECK_EVERY`` steps lost, once per model.  ``strict_range``: the check raises instead (after
    step 0 of loops longer than 8 steps, else at the loop's end).  Any other denoiser: nothing is checked or kept."""

    def __init__(self, model, num_steps: int, every: int = _CHECK_EVERY):
        model = getattr(model, "_orig_mod", model)  # (torch.compile wrapper)
        check = getattr(model, "check_range_or_fall_back", None)
        self.check = check if callable(check) else None
        #  Only modes whose operands pass through fp16 can trip and fall back: a model that already runs the wide-range split
        # ("fp32-bf16x3": its check cannot trip) keeps neither a checkpoint nor the noise of up to 32 steps (0.5 GB at 128 x 2048, batch 8)
        self.record = self.check is not None and getattr(model, "precision", "fp32") != "fp32-bf16x3"
        self.strict = bool(getattr(model, "strict_range", False))
        self.n, self.every = num_steps, every
        self.ck_i, self.ck_x, self.noise, self.replays = 0, None, [], 0

    def start(self, x):
        self.ck_x = x if self.record else None

    def noise_for(self, i: int, draw):
        """The noise of step i: what was drawn for it before a replay, else ``draw()`` (recorded while a guard is watching)."""
        k = i - self.ck_i
        if k < len(self.noise):
            return self.noise[k]
        nz = draw()
        if self.record:
            self.noise.append(nz)
        return nz

    def due(self, i: int) -> bool:
        if self.check is None:
            return False
        early = i == 0 and self.n > 8  # a checkpoint the fp16 operand path cannot run at all: found after one step
        if self.strict:
            return early  # (its loop-end check is the deferred guard's: raises there)
        return early or i == self.n - 1 or (i + 1) % self.every == 0

    def after_step(self, i: int, x):
        """-> (next step, its input): (i + 1, x), or the checkpoint if the guard tripped since it was taken."""
        if not self.due(i):
            return i + 1, x
        if self.check():
            if not self.record:  # (cannot happen: a mode without a fallback raises inside check())
                raise _lib.R2DMError("range guard tripped in a mode that keeps no replay state")
            self.replays += 1
            self.noise = self.noise[: i + 1 - self.ck_i]
            self.record = False  # the model now runs the wide-range split: no second trip -- the recording ends with this replay
            return self.ck_i, self.ck_x
        self.ck_i, self.ck_x, self.noise = i + 1, (x if self.record else None), []
        return i + 1, x


def _cache_opts(what: str, cache_interval, cache_depth, cache_drift, refuse: Optional[str] = None):
    """The feature-cache keywords of a sampler, checked: None for ``cache_interval = 1`` (no cache: the sampler's code path is the one without the
    keywords), else ``(interval, depth, drift)``.  ``refuse``: why ``what`` cannot run with a cache at all."""
    if isinstance(cache_interval, bool) or not isinstance(cache_interval, int) or cache_interval < 1:
        raise ValueError(f"cache_interval must be an integer >= 1 (1: no feature cache), got {cache_interval!r}")
    if isinstance(cache_depth, bool) or cache_depth not in (1, 2, 3):
        raise ValueError(f"cache_depth must be 1, 2 or 3 (the outermost U-Net levels a shallow step runs), got {cache_depth!r}")
    if cache_interval == 1:
        return None
    if refuse:
        raise ValueError(f"{what}: cache_interval = {cache_interval} is not supported: {refuse}")
    return cache_interval, cache_depth, bool(cache_drift)


def _progress_bar(total: int, desc: str, enabled: bool):
    try:
        return tqdm(total=total, desc=desc, leave=False, disable=not enabled)
    except TypeError:  # (the stand-in above: no bar)
        return None


def _rng_snapshot(rng, dev):
    """States of whatever ``GaussianDiffusion.randn`` draws from (base.py:71-94 forms), to repeat a loop on the same draws."""
    if rng is None:
        return torch.cuda.get_rng_state(dev) if torch.device(dev).type == "cuda" else torch.get_rng_state()
    if isinstance(rng, torch.Generator):
        return rng.get_state()
    return [g.get_state() for g in rng]


def _rng_restore(snap, rng, dev):
    if rng is None:
        torch.cuda.set_rng_state(snap, dev) if torch.device(dev).type == "cuda" else torch.set_rng_state(snap)
    elif isinstance(rng, torch.Generator):
        rng.set_state(snap)
    else:
        for g, s in zip(rng, snap):
            g.set_state(s)


def _rows(fn, whole: bool, cols):
    """``fn`` of (N,) tensors -> a tensor, or a tuple of tensors, of N rows: applied to ``cols`` as they are (``whole``: device tensors), or row
    by row to their 1-element slices and concatenated (host tensors).

    Why rows on the host: torch's CPU elementwise kernels round the last bit differently in their SIMD body and in their scalar tail, and the
    reference evaluates the schedule on (B,)-shaped tensors (continuous_time.py:203-206), i.e. on the scalar path for its CPU-runnable batch
    sizes (BASELINE configs[0]: batch 1).  Row-wise evaluation reproduces those values bit for bit and makes a table independent of the
    number of its rows.  A device elementwise kernel computes every element by the same instructions whatever the tensor's shape."""
    if whole:
        return fn(*cols)
    parts = [fn(*(c[i:i + 1] for c in cols)) for i in range(cols[0].numel())]
    return tuple(torch.cat(p) for p in zip(*parts)) if isinstance(parts[0], tuple) else torch.cat(parts)


def _cache_put(cache: dict, key, value):
    """Insert into one of the table caches, which hold 8 entries: the oldest goes first."""
    if len(cache) >= 8:
        cache.pop(next(iter(cache)))
    cache[key] = value
    return value


def _check_count(**named):
    for name, n in named.items():
        if int(n) != n or n < 1:
            raise ValueError(f"{name} must be an integer >= 1, got {n}")


def _check_level(t, name: str = "t_start"):
    if not 0.0 < float(t) <= 1.0:
        raise ValueError(f"{name} must be in (0, 1], got {t}")


def _check_solver(order, grid, eta):
    if order not in (1, 2):
        raise ValueError(f"order must be 1 or 2, got {order!r}")
    if grid not in ("logsnr", "time"):
        raise ValueError(f"grid must be 'logsnr' or 'time', got {grid!r}")
    if not float(eta) >= 0.0 or math.isinf(float(eta)):
        raise ValueError(f"eta must be finite and >= 0, got {eta}")


def _log(t: torch.Tensor, eps: float = 1e-20) -> torch.Tensor:
    return torch.log(t.clamp(min=eps))


def log_snr_linear(t):
    return -_log(expm1(1e-4 + 10 * (t**2)))


def log_snr_cosine(t, logsnr_min: float = -15, logsnr_max: float = 15):
    t_min = math.atan(math.exp(-0.5 * logsnr_max))
    t_max = math.atan(math.exp(-0.5 * logsnr_min))
    return -2 * _log(torch.tan(t_min + t * (t_max - t_min)))


def log_snr_cosine_shifted(t, image_d, noise_d, logsnr_min: float = -15, logsnr_max: float = 15):
    return log_snr_cosine(t, logsnr_min, logsnr_max) + 2 * math.log(noise_d / image_d)


def log_snr_cosine_interpolated(t, image_d, noise_d_low, noise_d_high, logsnr_min: float = -15,
                                logsnr_max: float = 15):
    low = log_snr_cosine_shifted(t, image_d, noise_d_low, logsnr_min, logsnr_max)
    high = log_snr_cosine_shifted(t, image_d, noise_d_high, logsnr_min, logsnr_max)
    return t * low + (1 - t) * high


def log_snr_to_alpha_sigma(log_snr):
    return log_snr.sigmoid().sqrt(), (-log_snr).sigmoid().sqrt()


def discrete_tables(num_training_steps: int, schedule: str):
    """beta / alpha_bar / alpha_bar_prev / snr in float64 -> float32 (discrete_time.py:12-78)."""
    T = num_training_steps
    if schedule == "linear":
        s = 1000 / T
        beta = torch.linspace(s * 0.0001, s * 0.02, T, dtype=torch.float64)
    elif schedule in ("cosine", "sigmoid"):
        t = torch.linspace(0, T, T + 1, dtype=torch.float64) / T
        if schedule == "cosine":
            ab = torch.cos((t + 0.008) / (1 + 0.008) * math.pi * 0.5) ** 2
        else:
            start, end, tau = -3, 3, 1
            v0, v1 = torch.tensor(start / tau).sigmoid(), torch.tensor(end / tau).sigmoid()
            ab = (-((t * (end - start) + start) / tau).sigmoid() + v1) / (v1 - v0)
        ab = ab / ab[0]
        beta = torch.clip(1 - (ab[1:] / ab[:-1]), 0, 0.999)
    else:
        raise ValueError(f"invalid beta schedule {schedule}")
    alpha_bar = torch.cumprod(1 - beta, dim=0)
    alpha_bar_prev = torch.cat([alpha_bar.new_ones(1), alpha_bar[:-1]])
    snr = alpha_bar / (1 - alpha_bar)
    return beta.float(), alpha_bar.float(), alpha_bar_prev.float(), snr.float()


# --------------------------------------------------------------------------------------
class GaussianDiffusion(nn.Module):
    """Common state and RNG plumbing (base.py:8-163)."""

    last_cache_drift = None  # the drift table of the last sampler call with ``cache_drift=True`` (FeatureCache.drift)

    def __init__(
        self,
        model: nn.Module,
        sampling: Literal["ddpm", "ddim"] = "ddpm",
        prediction_type: Literal["eps", "v", "x_0"] = "eps",
        loss_type="l2",
        num_training_steps: Optional[int] = 1000,
        noise_schedule: str = "linear",
        min_snr_loss_weight: bool = True,
        min_snr_gamma: float = 5.0,
        sampling_resolution: Optional[tuple] = None,
        clip_sample: bool = True,
        clip_sample_range: float = 1,
    ):
        super().__init__()
        self.model = model
        self.sampling = sampling
        self.num_training_steps = num_training_steps
        self.objective = prediction_type
        self.noise_schedule = noise_schedule
        self.loss_type = loss_type
        self.min_snr_loss_weight = min_snr_loss_weight
        self.min_snr_gamma = min_snr_gamma
        self.clip_sample = clip_sample
        self.clip_sample_range = clip_sample_range
        if sampling_resolution is None:
            assert hasattr(self.model, "resolution")
            assert hasattr(self.model, "in_channels")
            self.sampling_shape = (self.model.in_channels, *self.model.resolution)
        else:
            assert len(sampling_resolution) == 2
            assert hasattr(self.model, "in_channels")
            self.sampling_shape = (self.model.in_channels, *sampling_resolution)
        self.setup_parameters()
        self.register_buffer("_dummy", torch.tensor([]))

    @property
    def device(self):
        return self._dummy.device

    # -- RNG: identical draw shapes / order to base.py:71-94 -------------------------------
    def randn(self, *shape, rng: List[torch.Generator] | torch.Generator | None = None, **kwargs):
        if rng is None:
            return torch.randn(*shape, **kwargs)
        elif isinstance(rng, torch.Generator):
            return torch.randn(*shape, generator=rng, **kwargs)
        elif isinstance(rng, list):
            assert len(rng) == shape[0]
            # (base.py:81-85 stacks per-sample draws; drawn straight into the rows of the result here -- the same values from the same
            # generator states, one copy kernel and 2 x the bytes less per step)
            if not rng:
                return torch.stack([])  # (the reference's error for an empty batch)
            out = torch.empty(*shape, **kwargs)
            for i, r in enumerate(rng):
                torch.randn(*shape[1:], generator=r, out=out[i])
            return out
        else:
            raise ValueError(f"invalid rng: {rng}")

    def randn_like(self, x, rng=None):
        return self.randn(*x.shape, rng=rng, device=x.device, dtype=x.dtype)

    def _randn_like_ahead(self, x, rng=None):
        """``(noise, event)``: the step's noise drawn on a side stream BEFORE the denoiser call, so that its small kernels (one
        ``torch.randn`` per sample generator plus the stack: nine launches, ~45 us per step in series) fill the gaps of the
        denoiser's stream instead of following it.  Same draws in the same order as base.py:71-94 (the denoiser draws nothing;
        a generator's state advances on the host at launch time); the caller waits for ``event`` before it reads ``noise``.
        ``R2DM_NOISE_STREAM=0`` or a CPU tensor: a plain ``randn_like`` and no event."""
        if x.device.type != "cuda" or os.environ.get("R2DM_NOISE_STREAM", "1") == "0":
            return self.randn_like(x, rng=rng), None
        side = self.__dict__.get("_noise_stream")
        if side is None or side.device != x.device:
            side = self.__dict__["_noise_stream"] = torch.cuda.Stream(device=x.device)
        main = torch.cuda.current_stream(x.device)
        with torch.cuda.stream(side):
            noise = self.randn_like(x, rng=rng)
            event = torch.cuda.Event()
            event.record(side)
        noise.record_stream(main)
        return noise, event

    def setup_parameters(self) -> None:
        raise NotImplementedError

    # Where the schedule scalars are evaluated.  "host" (default): float32 on the CPU, row by row -- bit-identical
    # to the reference's CPU run (tests/golden/schedule.npz) on any machine.  "device": with the same torch ops on the tensors' own device,
    # as the reference does when it itself runs on a GPU (continuous_time.py:203-206,248-249: `linspace(..., device=self.device)`, log_snr,
    # alpha, sigma of device tensors).  The two differ in the last bits of libm; that only matters where a scalar is a rounding residue --
    # DDIM with eta = 1, whose c_2 = sqrt(1 - alpha_s^2 - c_1^2) is one on the first and last step (profiles/r05_fuzz.txt, case 15).
    schedule_on: str = "host"

    def set_schedule_on(self, where: str):
        if where not in ("host", "device"):
            raise ValueError(f"schedule_on must be 'host' or 'device', got {where!r}")
        self.schedule_on = where
        self.__dict__.pop("_tables", None)
        return self

    def _on_device(self, dev) -> bool:
        return self.schedule_on == "device" and torch.device(dev).type == "cuda"

    # -- the denoising loss (base.py:99-149), forward only ------------------------------------
    def sample_timesteps(self, batch_size: int, device) -> torch.Tensor:
        raise NotImplementedError

    def get_network_condition(self, steps):
        raise NotImplementedError

    def get_target(self, x_0, steps, noise):
        raise NotImplementedError

    def get_loss_weight(self, steps):
        raise NotImplementedError

    def _log_snr_of_steps(self, steps) -> torch.Tensor:
        """(B,) log-SNR of per-sample steps, evaluated where ``schedule_on`` says."""
        raise NotImplementedError

    def _loss_coef(self, steps) -> torch.Tensor:
        """(B,2) = (alpha, sigma) of q(x_t | x_0) at per-sample steps: the rows of ``r2dm_q_step`` and of the ``v`` target."""
        raise NotImplementedError

    def _loss_weight_of_snr(self, snr: torch.Tensor) -> torch.Tensor:
        """Min-SNR weighting (continuous_time.py:155-167, discrete_time.py:105-117), the reference's ops on ``snr``."""
        clipped_snr = snr.clone()
        if self.min_snr_loss_weight:
            clipped_snr.clamp_(max=self.min_snr_gamma)
        if self.objective == "eps":
            return clipped_snr / snr
        if self.objective == "x_0":
            return clipped_snr
        if self.objective == "v":
            return clipped_snr / (snr + 1)
        raise ValueError(f"invalid objective {self.objective}")

    def _criterion_name(self) -> str:
        if self.loss_type not in _CRITERIA:  # (base.py:45 also takes an nn.Module: autograd-side code, no HIP kernel for it)
            raise ValueError(f"invalid criterion: {self.loss_type}")
        return self.loss_type

    @torch.inference_mode()
    def loss_terms(self, x_0, steps, loss_mask=None, rng=None, noise=None) -> dict:
        """The value of ``p_loss`` (base.py:122-139) with its pieces; forward only, under ``torch.inference_mode()``: nothing returned
        carries a gradient.  One noising (``r2dm_q_step``), one denoiser call, one fused reduction (``r2dm_diffusion_loss``: target,
        criterion, mask and the float64 sums in one pass).

        ``noise`` (extension): explicit noise instead of a draw; else ``randn_like(x_0, rng)``, ``rng`` as everywhere in this class
        (None: the global generator of ``x_0``'s device, as the reference's ``q_step_from_x_0(x_0, steps)``).
        ``loss_mask``: None (all ones), ``(B,1,H,W)`` or ``(B,C,H,W)``.

        -> ``per_channel`` (B,C): the channel's masked loss sum over the mask's sum (the channels add up to ``per_sample``);
        ``per_sample`` (B,): base.py:135-137, ``float32(sum) / (float32(mask sum) + 1e-8)``; ``weight`` (B,): ``get_loss_weight``;
        ``weighted`` (B,): ``per_sample * weight``; ``log_snr`` (B,); ``loss`` (0-d): base.py:138 as the reference evaluates it.  There
        the (B,1) losses meet the (B,1,1,1) weights, so the product is (B,1,B,1) -- every loss with every weight -- and its mean is
        ``mean(weight) * mean(per_sample)`` up to rounding, not ``mean(weighted)``; the two agree when all steps are equal
        (``r2dm_amd.loss.loss_curve`` evaluates one level at a time).  A sample's entries do not depend on the rest of the batch."""
        if self.device.type != "cuda" or not x_0.is_cuda:
            raise NoCPUFallback(f"the denoising loss runs as HIP kernels on an MI355X (model on {self.device}, x_0 on {x_0.device}): "
                                "r2dm_amd has no CPU fallback")
        objective, criterion = self.objective, self._criterion_name()
        self._objective_id()
        dev = x_0.device
        x_0 = _lib.f32c(x_0)
        B = x_0.shape[0]
        steps = steps.reshape(-1)
        if steps.numel() != B:
            raise ValueError(f"steps must have shape ({B},), got {tuple(steps.shape)}")
        if noise is None:
            noise = self.randn_like(x_0, rng=rng)
        coef = self._loss_coef(steps).to(dev)
        x_t = _lib.q_step(x_0, noise, coef)
        prediction = self.model(x_t, self.get_network_condition(steps).to(dev))  # (a range-guard trip: handled inside EfficientUNet.forward)
        num, den = _lib.diffusion_loss(prediction, x_0, noise, loss_mask, coef, objective, criterion)
        total = num[:, 0].clone()
        for c in range(1, num.shape[1]):  # channel order, whatever the batch
            total += num[:, c]
        den32 = den.float().add(1e-8)
        per_sample = total.float() / den32
        weight = self.get_loss_weight(steps).reshape(B).to(dev)
        loss = (per_sample[:, None] * weight[:, None, None, None]).mean()
        return {"per_channel": num.float() / den32[:, None], "per_sample": per_sample, "weight": weight, "weighted": per_sample * weight,
                "log_snr": self._log_snr_of_steps(steps).reshape(B).to(dev), "loss": loss}

    def p_loss(self, x_0, steps, loss_mask=None, rng=None):
        """base.py:122-139 -> 0-d float32 on the device; ``loss_terms(...)["loss"]``.  Forward only: evaluated under
        ``torch.inference_mode()``, the result carries no gradient (there is no training here)."""
        return self.loss_terms(x_0, steps, loss_mask, rng=rng)["loss"]

    def forward(self, x_0, loss_mask=None, rng=None):
        """base.py:141-149: the denoising loss at freshly drawn steps -- the steps first, then the noise.  Forward only, no gradient
        (see ``p_loss``).  On a model or a batch that is not on a GPU: ``NoCPUFallback``."""
        if self.device.type != "cuda" or not x_0.is_cuda:
            raise NoCPUFallback(f"the denoising loss runs as HIP kernels on an MI355X (model on {self.device}, x_0 on {x_0.device}): "
                                "r2dm_amd has no CPU fallback")
        steps = self.sample_timesteps(x_0.shape[0], x_0.device)
        return self.p_loss(x_0, steps, loss_mask, rng=rng)

    def _objective_id(self) -> int:
        if self.objective not in _lib.OBJECTIVES:
            raise ValueError(f"invalid objective {self.objective}")
        return _lib.OBJECTIVES[self.objective]

    def _clip(self, clip: Optional[bool] = None) -> float:
        """The clamp of the x_0 estimate as the kernels take it (< 0: none).  ``clip``: None -- the model's ``clip_sample`` setting; True / False: on / off for one call."""
        return float(self.clip_sample_range) if (self.clip_sample if clip is None else clip) else -1.0

    def _posterior(self, x_t, pred, noise, coef, mode_id: int, clip: Optional[float] = None):
        """x_s = posterior(x_t, prediction, noise) in one HIP launch (``clip``: None -- the model's setting; < 0: no clamp)."""
        return _lib.posterior_step(x_t, pred, noise, coef, mode_id, self._objective_id(), self._clip() if clip is None else clip)

    def _denoise(self, x, cond, early_check: int = 0):
        """One denoiser call.  ``early_check``: the first call of a loop under the deferred range guard passes the loop's length -- the guard
        is read right after it (``_early_range_check``), and on a trip the call is repeated on the wide-range operand split."""
        prediction = self.model(x, cond)
        if early_check and _early_range_check(self.model, early_check):
            prediction = self.model(x, cond)
        return prediction

    def _twice_on_fallback(self, rng, call):
        """``call()``; a range-guard trip that only shows at the loop's end (``R2DMRangeFallback``) leaves the denoiser switched to the wide-range
        split: the call is then repeated once, from the generator states it started with -- same draws, no exception."""
        snap = _rng_snapshot(rng, self.device)
        try:
            return call()
        except _lib.R2DMRangeFallback:
            _rng_restore(snap, rng, self.device)
            return call()

    def _run_loop(self, x, num_steps: int, row, update, draw, progress: bool, return_all: bool, desc: str = "sampling", cache=None):
        """The step loop every sampler here shares (``sample``, ``sample_from``, ``invert``, ``sample_dpm``, ``complete_dpm``): per step
        ``row(i) -> (cond, coef)``, the step's noise (``draw(x) -> (noise, event)`` ahead of the denoiser call; None: a deterministic update,
        nothing is drawn), one denoiser call, ``update(x, prediction, noise, coef, hist) -> (x, hist)``; under the deferred range guard, with
        ``_Replay``'s recovery.  ``hist`` is what a multistep update hands to its next step beside ``x`` (the previous estimate of x_0; None
        before the first step and for the one-step samplers), and the pair is what ``_Replay`` keeps.  ``_Replay`` only stores the object it
        is given and an update may write ``hist``'s buffer again two steps on, so at a step whose check is due the loop hands on a COPY: the
        checkpoint's history is then a buffer no later step writes.
        ``cache``: ``_cache_opts``' ``(interval, depth, drift)`` -- the denoiser runs through a feature cache (``EfficientUNet.forward_cached``): step i
        is a full step when ``i % interval == 0`` or the cache is not valid (``unet.step_is_full``) -- at the loop's start, after a replay has gone back,
        after a precision switch -- and a shallow one otherwise; with ``drift`` the full steps' drift table lands in ``self.last_cache_drift``.
        -> the last ``x``, or with ``return_all`` the (S+1, ...) stack that starts with the given ``x``."""
        if return_all:
            out = [x]
        fc = None
        if cache is not None:
            interval, depth, drift = cache
            net = getattr(self.model, "_orig_mod", self.model)  # (torch.compile wrapper)
            if not callable(getattr(net, "new_cache", None)):
                raise ValueError(f"cache_interval = {interval} needs a denoiser with a feature cache (r2dm_amd's EfficientUNet), got {type(net).__name__}")
            fc = net.new_cache(x.shape[0], depth, drift)
        rp = _Replay(self.model, num_steps)  # (a range-guard trip at any step: back to the last checked state, on the recorded noise)
        rp.start((x, None))
        hist = None
        bar = _progress_bar(num_steps, desc, progress)
        with _range_guard(self.model):
            i = 0
            while i < num_steps:
                cond_i, coef_i = row(i)
                noise, drawn = rp.noise_for(i, lambda: draw(x)) if draw is not None else (None, None)
                if fc is None:
                    prediction = self.model(x, cond_i)
                else:
                    prediction = net.forward_cached(x, cond_i, fc, refresh=step_is_full(i, interval, fc.usable()))
                if drawn is not None:
                    torch.cuda.current_stream(x.device).wait_event(drawn)
                x_s, hist = update(x, prediction, noise, coef_i, hist)
                if hist is not None and rp.record and rp.due(i):
                    hist = hist.clone()
                nxt, (x, hist) = rp.after_step(i, (x_s, hist))
                if fc is not None and nxt <= i:
                    fc.invalidate()  # (a replay: the cached features belong to a later level than the checkpoint's)
                if return_all:
                    del out[nxt + 1:]  # (after a replay: the steps that are run again; else nothing)
                    if nxt > i:
                        out.append(x)
                if bar is not None:
                    bar.update(nxt - i)
                i = nxt
        if bar is not None:
            bar.close()
        if fc is not None and drift:
            self.last_cache_drift = fc.drift()
        return torch.stack(out) if return_all else x

    def _refuse_cpu(self, what: str, x):
        if self.device.type != "cuda" or not x.is_cuda:
            raise NoCPUFallback(f"{what} runs as HIP kernels on an MI355X (model on {self.device}, input on {x.device}): r2dm_amd has no CPU fallback")


# --------------------------------------------------------------------------------------
class ContinuousTimeGaussianDiffusion(GaussianDiffusion):
    """Variational-diffusion-style continuous-time process (continuous_time.py:66-317)."""

    def __init__(
        self,
        model: nn.Module,
        prediction_type: Literal["eps", "v", "x_0"] = "eps",
        loss_type="l2",
        noise_schedule: Literal["linear", "cosine", "cosine_shifted", "cosine_interpolated"] = "cosine",
        min_snr_loss_weight: bool = True,
        min_snr_gamma: float = 5.0,
        sampling_resolution: Optional[tuple] = None,
        clip_sample: bool = True,
        clip_sample_range: float = 1,
        image_d: float = None,
        noise_d_low: float = None,
        noise_d_high: float = None,
    ):
        self.image_d, self.noise_d_low, self.noise_d_high = image_d, noise_d_low, noise_d_high
        super().__init__(
            model=model,
            sampling="ddpm",
            prediction_type=prediction_type,
            loss_type=loss_type,
            num_training_steps=None,
            noise_schedule=noise_schedule,
            min_snr_loss_weight=min_snr_loss_weight,
            min_snr_gamma=min_snr_gamma,
            sampling_resolution=sampling_resolution,
            clip_sample=clip_sample,
            clip_sample_range=clip_sample_range,
        )

    def setup_parameters(self) -> None:
        if self.noise_schedule == "linear":
            f = log_snr_linear
        elif self.noise_schedule == "cosine":
            f = log_snr_cosine
        elif self.noise_schedule == "cosine_shifted":
            assert self.image_d is not None and self.noise_d_low is not None
            f = partial(log_snr_cosine_shifted, image_d=self.image_d, noise_d=self.noise_d_low)
        elif self.noise_schedule == "cosine_interpolated":
            assert self.image_d is not None and self.noise_d_low is not None and self.noise_d_high is not None
            f = partial(log_snr_cosine_interpolated, image_d=self.image_d, noise_d_low=self.noise_d_low,
                        noise_d_high=self.noise_d_high)
        else:
            raise ValueError(f"invalid beta schedule: {self.noise_schedule}")
        self._log_snr_1d = f

    def log_snr(self, t: torch.Tensor) -> torch.Tensor:
        """(B,) -> (B,1,1,1), as continuous_time.py:14-29."""
        return self._log_snr_1d(t)[:, None, None, None]

    def get_network_condition(self, steps):
        """(B,) per-sample steps -> (B,) log-SNR (continuous_time.py:137-138), with the schedule's torch ops on ``steps`` as they are."""
        return self._log_snr_1d(steps)

    # -- the denoising loss's pieces (continuous_time.py:133-167) --------------------------
    def sample_timesteps(self, batch_size: int, device) -> torch.Tensor:
        return torch.rand(batch_size, device=device, dtype=torch.float32)

    def _placed(self, *steps):
        """``(whole, cols)`` for ``_rows``: the steps as float32 (N,) tensors where ``schedule_on`` says -- on the first one's device, or on the host."""
        whole = self._on_device(steps[0].device)
        return whole, [s.detach().to(steps[0].device if whole else "cpu", torch.float32).reshape(-1) for s in steps]

    def _log_snr_of_steps(self, steps) -> torch.Tensor:
        """(B,) log-SNR where ``schedule_on`` says: on the host row by row (see ``_rows``: the values of the reference's CPU run, and a row does
        not depend on the batch), or with the same ops on the device."""
        return _rows(self._log_snr_1d, *self._placed(steps))

    def _loss_coef(self, steps) -> torch.Tensor:
        return self._alpha_sigma_rows(steps)

    def get_target(self, x_0, step_t, noise):
        """continuous_time.py:140-151, in torch (the fused loss kernel does not call this; the tests compare it with that kernel)."""
        if self.objective == "eps":
            return noise
        if self.objective == "x_0":
            return x_0
        if self.objective == "v":
            coef = self._alpha_sigma_rows(step_t).to(x_0.device)
            alpha, sigma = coef[:, 0][:, None, None, None], coef[:, 1][:, None, None, None]
            return alpha * noise - sigma * x_0
        raise ValueError(f"invalid objective {self.objective}")

    def get_loss_weight(self, steps):
        """(B,1,1,1) min-SNR loss weights (continuous_time.py:153-167), on ``steps``' device."""
        weight = _rows(lambda l: self._loss_weight_of_snr(l.exp()), self._on_device(steps.device), [self._log_snr_of_steps(steps)])
        return weight[:, None, None, None].to(steps.device)

    # -- host-side coefficient table -------------------------------------------------------
    def _coefficient_block(self, t: torch.Tensor, s: torch.Tensor, mode: str, ddim_eta: float):
        """Scalars of continuous_time.py:203-229 for (N,) step pairs, with the reference's own torch expressions, WHERE t lives:
        -> (log-SNR (N,), coefficients (N, 8))."""
        lt, ls = self._log_snr_1d(t), self._log_snr_1d(s)
        a_t, s_t = log_snr_to_alpha_sigma(lt)
        a_s, s_s = log_snr_to_alpha_sigma(ls)
        z = torch.zeros_like(lt)
        if mode == "ddpm":
            c = -expm1(lt - ls)
            return lt, torch.stack([a_t, s_t, a_s, s_s, c, s_s * c.sqrt(), z, z], dim=-1)
        if mode == "ddim":
            c_1 = ddim_eta * s_s / s_t * (1 - a_t**2 / a_s**2).sqrt()
            c_2 = (1 - a_s**2 - c_1**2).sqrt()
            return lt, torch.stack([a_t, s_t, a_s, s_s, z, z, c_1, c_2], dim=-1)
        raise ValueError(f"invalid mode {mode}")

    def _coefficients(self, step_t: torch.Tensor, step_s: torch.Tensor, mode: str, ddim_eta: float):
        """Per-row schedule scalars, float32, where ``schedule_on`` says (on the host row by row: see ``_rows``; on the device (B,)-shaped
        tensors through the same ops, as the reference on a GPU).  Returns (cond (N,), coef (N,8), kernel mode)."""
        if mode not in ("ddpm", "ddim"):
            raise ValueError(f"invalid mode {mode}")
        whole, cols = self._placed(step_t, step_s)
        memo = {}  # (host rows: the samples of a batch share one (t, s) pair -- evaluated once)

        def block(t, s):
            if whole:
                return self._coefficient_block(t, s, mode, ddim_eta)
            key = (t.item(), s.item())
            if key not in memo:
                memo[key] = self._coefficient_block(t, s, mode, ddim_eta)
            return memo[key]

        lt, coef = _rows(block, whole, cols)
        return lt, coef.contiguous(), (_M_CT_DDPM if mode == "ddpm" else _M_CT_DDIM)

    def _sample_tables(self, num_steps: int, batch_size: int, mode: str, ddim_eta: float, dev):
        """(cond (S, B), coef (S, B, 8), kernel mode) of a whole ``sample`` call on the device: ``_table_rows`` walked to its
        end (ONE implementation builds, caches and evicts the tables -- the one ``sample`` uses)."""
        row, mode_id = self._table_rows(num_steps, batch_size, mode, ddim_eta, dev)
        for i in range(num_steps):
            row(i)
        cond, coef, _ = self.__dict__["_tables"][self._table_key(num_steps, batch_size, mode, ddim_eta, dev)]
        return cond, coef, mode_id

    def _table_key(self, num_steps, batch_size, mode, ddim_eta, dev, t_start: float = 1.0):
        key = (num_steps, batch_size, mode, float(ddim_eta), str(torch.device(dev)), self.noise_schedule, self.image_d, self.noise_d_low, self.noise_d_high,
               self.schedule_on)
        return key if t_start == 1.0 else key + (("t_start", float(t_start)),)  # (``sample``'s keys are what they were)

    def _table_rows(self, num_steps: int, batch_size: int, mode: str, ddim_eta: float, dev, t_start: float = 1.0):
        """``row(i) -> (cond (B,), coef (B, 8))`` and ``mode_id`` for a ``sample`` call (``sample_from``: the steps start at ``t_start``).  A cached table is indexed; a new one is
        built ROW BY ROW while the loop runs: each row is ~0.3 ms of host work (about thirty 1-element torch ops), 80 ms for 256
        steps -- with the whole table built up front that was 4.5 % of a cold 256-step call with the GPU idle (round 3:
        scripts/step_times.py, profiles/r03_step_times.txt), whereas one row per step hides under the ~6 ms the GPU needs per
        step.  Rows travel through pinned host memory (an asynchronous copy on the sampling stream: the host never waits for the
        GPU) into the device table, which enters the cache when its last row is in."""
        dev = torch.device(dev)
        key = self._table_key(num_steps, batch_size, mode, ddim_eta, dev, t_start)
        cache = self.__dict__.setdefault("_tables", {})
        hit = cache.get(key)
        if hit is not None:
            cond, coef, mode_id = hit
            return (lambda i: (cond[i], coef[i])), mode_id
        if mode not in ("ddpm", "ddim"):
            raise ValueError(f"invalid mode {mode}")
        mode_id = _M_CT_DDPM if mode == "ddpm" else _M_CT_DDIM
        if self._on_device(dev):
            # the whole table at once, on the device: `steps` is the reference's own device linspace (continuous_time.py:248), and a device
            # elementwise kernel computes every element by the same instructions whatever the tensor's shape -- (S,) here, (B,) per step there
            steps = torch.linspace(float(t_start), 0.0, num_steps + 1, device=dev)
            lt, k = self._coefficient_block(steps[:-1], steps[1:], mode, ddim_eta)
            cond = lt[:, None].repeat_interleave(batch_size, dim=1).contiguous()
            coef = k[:, None, :].repeat_interleave(batch_size, dim=1).contiguous()
            _cache_put(cache, key, (cond, coef, mode_id))
            return (lambda i: (cond[i], coef[i])), mode_id
        steps = torch.linspace(float(t_start), 0.0, num_steps + 1)
        pin = dev.type == "cuda"
        h_cond = torch.empty(num_steps, batch_size, pin_memory=pin)
        h_coef = torch.empty(num_steps, batch_size, _NCOEF, pin_memory=pin)
        cond = torch.empty(num_steps, batch_size, device=dev)
        coef = torch.empty(num_steps, batch_size, _NCOEF, device=dev)

        def row(i):
            c, k, _ = self._coefficients(steps[i:i + 1], steps[i + 1:i + 2], mode, ddim_eta)
            h_cond[i] = c
            h_coef[i] = k[0]
            cond[i].copy_(h_cond[i], non_blocking=True)
            coef[i].copy_(h_coef[i], non_blocking=True)
            if i == num_steps - 1:
                _cache_put(cache, key, (cond, coef, mode_id))
            return cond[i], coef[i]

        return row, mode_id

    @torch.inference_mode()
    def p_step(self, x_t, step_t, step_s, rng=None, mode: Literal["ddpm", "ddim"] = "ddpm",
               ddim_eta: float = 0.0, _early_check: int = 0):
        """One reverse step p(z_s | z_t), 0 <= s < t <= 1 (continuous_time.py:192-232).
        (``_early_check``: internal -- the first step of a loop under the deferred range guard passes its step count.)"""
        self._objective_id()
        dev = x_t.device
        if self._on_device(dev):
            step_t, step_s = step_t.to(dev), step_s.to(dev)
        cond, coef, mode_id = self._coefficients(step_t, step_s, mode, ddim_eta)
        prediction = self._denoise(x_t, cond.to(dev), _early_check)
        noise = self.randn_like(x_t, rng=rng)
        return self._posterior(x_t, prediction, noise, coef.to(dev), mode_id)

    @torch.inference_mode()
    def sample(self, batch_size: int, num_steps: int, progress: bool = True, rng=None,
               return_all: bool = False, mode: Literal["ddpm", "ddim"] = "ddpm", ddim_eta: float = 0.0,
               cache_interval: int = 1, cache_depth: int = 1, cache_drift: bool = False):
        """Ancestral / DDIM sampling from t=1 to t=0 (continuous_time.py:234-258).
        ``cache_interval = n > 1`` (not in the reference; DeepCache, Ma et al. 2024): only every n-th step runs the whole U-Net; the steps between run its
        ``cache_depth`` outermost levels and reuse the deep features of the last full step (``EfficientUNet.forward_cached``) -- an approximation whose cost
        in sample quality depends on the checkpoint; ``cache_drift`` records how far those features moved between full steps
        (``self.last_cache_drift``: (full steps, B), NaN where nothing valid was replaced).  The default, 1, is the sampler without a cache."""
        dev = self.device
        self._objective_id()
        cache = _cache_opts("sample", cache_interval, cache_depth, cache_drift)
        x = self.randn(batch_size, *self.sampling_shape, rng=rng, device=dev)
        return self._reverse_loop(x, num_steps, 1.0, progress, rng, return_all, mode, ddim_eta, cache=cache)

    def _reverse_loop(self, x, num_steps, t_start, progress, rng, return_all, mode, ddim_eta, clip: Optional[float] = None, cache=None):
        """The reverse process from ``x`` at ``t_start`` to t = 0 over ``linspace(t_start, 0, num_steps + 1)``: ``sample`` and ``sample_from``
        (``clip``: None -- the model's setting, else ``_posterior``'s override)."""
        row, mode_id = self._table_rows(num_steps, x.shape[0], mode, ddim_eta, x.device, t_start)
        return self._run_loop(x, num_steps, row, lambda x, pred, noise, coef, _: (self._posterior(x, pred, noise, coef, mode_id, clip), None),
                              lambda x: self._randn_like_ahead(x, rng=rng), progress, return_all, cache=cache)

    @torch.inference_mode()
    def sample_from(self, x_t, num_steps: int, t_start: float = 1.0, progress: bool = True, rng=None, return_all: bool = False,
                    mode: Literal["ddpm", "ddim"] = "ddpm", ddim_eta: float = 0.0, clip: Optional[bool] = None,
                    cache_interval: int = 1, cache_depth: int = 1, cache_drift: bool = False):
        """``sample``'s reverse loop started from a given ``x_t`` (B,C,H,W) at noise level ``t_start`` instead of a fresh draw at t = 1,
        over ``linspace(t_start, 0, num_steps + 1)``: decodes a latent of ``invert`` or an interpolated one, or -- after
        ``q_step_from_x_0(x_0, t_start)`` -- denoises a partially noised scan.  With ``x_t = randn(B, ...)`` from the same generators and
        ``t_start = 1`` it is ``sample``, bit for bit.  ``clip``: None keeps the model's ``clip_sample`` setting, False switches the clamp
        of the predicted x_0 off for this call only (a round trip through ``invert`` needs that), True switches it on.
        ``cache_interval``, ``cache_depth``, ``cache_drift``: the feature cache, as in ``sample``."""
        cache = _cache_opts("sample_from", cache_interval, cache_depth, cache_drift)
        self._refuse_cpu("sample_from", x_t)
        _check_level(t_start)
        if x_t.dim() != 4 or x_t.shape[0] < 1:
            raise ValueError(f"x_t must be (B,C,H,W) with B >= 1, got {tuple(x_t.shape)}")
        self._objective_id()
        return self._reverse_loop(_lib.f32c(x_t), num_steps, float(t_start), progress, rng, return_all, mode, ddim_eta, self._clip(clip), cache=cache)

    # -- DPM-Solver++(2M): a second-order multistep solver of the probability-flow ODE on the log-SNR axis (not in the reference) ------------
    def _dpm_table(self, num_steps: int, batch_size: int, order: int, grid: str, t_start: float, lower_order_final: bool, dev, eta: float = 0.0):
        """``(cond (S,B), coef (S,B,8) on the device, second (S,) bool on the host)`` of a ``sample_dpm`` call; rows of ``r2dm_dpm_step``:
        ``(alpha_t, sigma_t, c_x, c_0, c_1, 0, 0, 0)``, with ``eta > 0`` of ``r2dm_dpm_step_known``: ``(alpha_t, sigma_t, c_x, c_0, c_1, c_z, 0, 0)``.

        The log-SNR values lambda_0 .. lambda_S in float32: ``grid="logsnr"`` is ``linspace(lambda(t_start), lambda(0), S + 1)``, ``grid="time"`` is
        ``lambda(linspace(t_start, 0, S + 1))`` evaluated row by row as ``_coefficients`` does, so its ``cond`` rows are ``sample_from``'s bit for
        bit.  ``cond[i] = lambda_i``; alpha_t, sigma_t are ``log_snr_to_alpha_sigma(lambda_i)`` in float32 (what the estimate of x_0 is formed
        with everywhere else).  The solver's own scalars come from those float32 lambdas in float64 on the host, rounded once: with the half
        log-SNR step ``h_i = (lambda_{i+1} - lambda_i) / 2``, ``c_x = sigma_s / sigma_t`` and ``m = -alpha_s expm1(-h_i)``; a first-order row has
        ``c_0 = m, c_1 = 0`` (this is DDIM with eta = 0 written in x_0: ``c_x x + m x0 = alpha_s x0 + sigma_s (x - alpha_t x0) / sigma_t``), a
        second-order row with ``r = h_{i-1} / h_i`` has ``c_0 = m (1 + 1/(2r))``, ``c_1 = -m / (2r)``.  Row 0 is first-order (there is no
        history), every row is with ``order=1``, and with ``lower_order_final`` so is the last one.

        ``eta`` (>= 0) is the share of the step's noise that is drawn anew (SDE-DPM-Solver++(2M) at eta = 1): ``c_x = (sigma_s / sigma_t)
        exp(-eta h_i)``, ``m = -alpha_s expm1(-(1 + eta) h_i)`` and ``c_z = sigma_s sqrt(-expm1(-2 eta h_i))`` in slot 5, c_0 and c_1 from m as
        above.  At eta = 0 every entry is what it was, bit for bit, and c_z = 0.  A first-order row at eta = 1 is the ancestral posterior in
        another operation order: with ``c = 1 - exp(-2 h)``, ``c_x = alpha_s (1 - c) / alpha_t``, ``m = alpha_s c`` and ``c_z = sigma_s sqrt(c)``.

        ``schedule_on`` does not apply: the table is always evaluated on the host (its scalars are differences of neighbouring log-SNR values
        in float64, which a float32 device evaluation cannot give).  Cached like ``_tables``, under a key of its own."""
        dev = torch.device(dev)
        eta = float(eta)
        key = (int(num_steps), int(batch_size), int(order), grid, float(t_start), bool(lower_order_final), str(dev), self.noise_schedule, self.image_d,
               self.noise_d_low, self.noise_d_high, eta)
        cache = self.__dict__.setdefault("_dpm_tables", {})
        hit = cache.get(key)
        if hit is not None:
            return hit
        S = int(num_steps)
        one = lambda t: _rows(self._log_snr_1d, False, [t])
        if grid == "time":
            lam = one(torch.linspace(float(t_start), 0.0, S + 1))
        elif grid == "logsnr":
            ends = one(torch.tensor([float(t_start), 0.0]))
            lam = torch.linspace(ends[0].item(), ends[1].item(), S + 1)
        else:
            raise ValueError(f"grid must be 'logsnr' or 'time', got {grid!r}")
        l64 = [float(v) for v in lam.tolist()]
        alpha = lambda l: math.sqrt(1.0 / (1.0 + math.exp(-l)))
        sigma = lambda l: math.sqrt(1.0 / (1.0 + math.exp(l)))
        h = [(l64[i + 1] - l64[i]) / 2.0 for i in range(S)]
        rows, second = [], []
        for i in range(S):
            a_t, s_t = log_snr_to_alpha_sigma(lam[i:i + 1])
            m = -alpha(l64[i + 1]) * math.expm1(-(1.0 + eta) * h[i])
            is2 = order == 2 and i > 0 and not (lower_order_final and i == S - 1)
            if is2:
                r = h[i - 1] / h[i]
                c_0, c_1 = m * (1.0 + 1.0 / (2.0 * r)), -m / (2.0 * r)
            else:
                c_0, c_1 = m, 0.0
            c_x = sigma(l64[i + 1]) / sigma(l64[i]) * math.exp(-eta * h[i])  # (eta = 0: times exp(-0.0) = 1.0 -- the values of before)
            c_z = sigma(l64[i + 1]) * math.sqrt(-math.expm1(-2.0 * eta * h[i]))
            rows.append([a_t.item(), s_t.item(), c_x, c_0, c_1, c_z, 0.0, 0.0])
            second.append(is2)
        k = torch.tensor(rows, dtype=torch.float64).float()  # (alpha_t, sigma_t are float32 values already: unchanged by the round trip)
        cond = lam[:-1, None].repeat_interleave(batch_size, dim=1).contiguous().to(dev)
        coef = k[:, None, :].repeat_interleave(batch_size, dim=1).contiguous().to(dev)
        return _cache_put(cache, key, (cond, coef, torch.tensor(second, dtype=torch.bool)))

    @torch.inference_mode()
    def sample_dpm(self, batch_size: int, num_steps: int, order: int = 2, grid: Literal["logsnr", "time"] = "logsnr", progress: bool = True, rng=None,
                   return_all: bool = False, x_t=None, t_start: float = 1.0, clip: Optional[bool] = None, lower_order_final: bool = True,
                   eta: float = 0.0, cache_interval: int = 1, cache_depth: int = 1, cache_drift: bool = False):
        """DPM-Solver++(2M) sampling (Lu et al. 2022): a deterministic second-order multistep solver of the probability-flow ODE in
        data-prediction form, on ``num_steps + 1`` log-SNR values from ``t_start`` to t = 0.  Per step one denoiser call at ``cond[i]`` and one
        ``r2dm_dpm_step``, which forms the clamped estimate of x_0 as the other samplers do, keeps it as the next step's history and combines
        it with the previous one; it is meant for 16-32 steps, where ``sample(mode="ddim")`` needs a hundred or more.

        ``x_t=None`` draws the start exactly as ``sample`` does (one ``randn(batch_size, *sampling_shape)`` on ``rng``, at ``t_start = 1``); a given
        ``x_t`` (B,C,H,W) at noise level ``t_start`` is decoded like ``sample_from`` (``batch_size`` must be its B).  NOTHING else is drawn: the
        solver is deterministic, and unlike ``sample(mode="ddim")``, which draws a tensor per step even at eta = 0 (as the reference does), it
        leaves the generators one draw further (none with a given ``x_t``).
        ``order``: 2, or 1 (every row first-order: DDIM with eta = 0 in its x_0 form).  ``grid``: "logsnr" -- uniform in log-SNR, the solver's
        natural axis -- or "time", ``sample_from``'s ``linspace(t_start, 0, num_steps + 1)`` (the same network conditions, bit for bit).
        ``lower_order_final``: the last step, into sigma ~ 0, is taken first-order.  Default True: on the time grid the last log-SNR step is
        several times the one before it, and an extrapolation over it is worse than none -- with a closed-form denoiser the second-order run
        without it is 1.5-3 x FURTHER from the exact solution than the first-order run at up to 32 steps (tests/test_dpm_cpu.py).
        ``clip``: None keeps the model's ``clip_sample`` setting, False / True switch the clamp of the x_0 estimate off / on for this call.
        ``return_all``: the (S+1,B,C,H,W) stack that starts with the start tensor.
        ``eta``: 0 (default) is the deterministic solver above, unchanged.  ``eta > 0`` is the stochastic member of the family (eta = 1:
        SDE-DPM-Solver++(2M); order 1 at eta = 1: the ancestral step): one ``randn_like`` per step on ``rng``, drawn ahead of the denoiser call on
        the side stream as in ``sample``, and the step is ``r2dm_dpm_step_known`` with that noise and no measurement.  A replay after a
        range-guard trip runs on the recorded noise.

        Runs under the deferred range guard with ``_Replay``'s recovery, whose checkpoint here is the pair (x, previous x_0 estimate): after a
        trip the loop goes back at most ``_CHECK_EVERY`` steps WITH the history those steps were taken with, on the wide-range split.
        ``schedule_on`` does not apply (see ``_dpm_table``).
        ``cache_interval``, ``cache_depth``, ``cache_drift``: the feature cache, as in ``sample`` (the log-SNR steps of a 16-32 step grid are far larger than
        those of a 256-step ancestral run, so the deep features move further between full steps: look at the drift before trusting an interval)."""
        _check_solver(order, grid, eta)
        cache = _cache_opts("sample_dpm", cache_interval, cache_depth, cache_drift)
        _check_count(num_steps=num_steps)
        _check_level(t_start)
        _check_count(batch_size=batch_size)
        if x_t is None:
            if float(t_start) != 1.0:
                raise ValueError(f"t_start = {t_start} needs x_t (the tensor at that noise level): a fresh draw starts at t_start = 1")
        elif x_t.dim() != 4 or x_t.shape[0] != batch_size:
            raise ValueError(f"x_t must be (batch_size = {batch_size},C,H,W), got {tuple(x_t.shape)}")
        self._objective_id()
        if self.device.type != "cuda" or (x_t is not None and not x_t.is_cuda):
            raise NoCPUFallback(f"sample_dpm runs as HIP kernels on an MI355X (model on {self.device}"
                                + ("" if x_t is None else f", input on {x_t.device}") + "): r2dm_amd has no CPU fallback")
        x = self.randn(batch_size, *self.sampling_shape, rng=rng, device=self.device) if x_t is None else _lib.f32c(x_t)
        return self._dpm_solve(x, num_steps, order, grid, t_start, lower_order_final, eta, clip, progress, rng, return_all, cache=cache)

    def _dpm_solve(self, x, num_steps, order, grid, t_start, lower_order_final, eta, clip, progress, rng, return_all, known=None, mask=None,
                  desc: str = "sampling", cache=None):
        """``sample_dpm`` and ``complete_dpm`` from their start tensor: ``_run_loop`` over ``_dpm_table`` with the multistep update, whose history is
        the previous estimate of x_0.  The estimates ping-pong between two buffers (``_run_loop`` copies the one a checkpoint keeps).  The step's
        noise (``eta > 0``) is drawn ahead of the denoiser call; ``known``, ``mask``: the measurement written over every estimate.  With neither
        the step is ``r2dm_dpm_step``, else ``r2dm_dpm_step_known``."""
        cond, coef, second = self._dpm_table(int(num_steps), x.shape[0], order, grid, float(t_start), lower_order_final, x.device, float(eta))
        second, objective, clip = second.tolist(), self._objective_id(), self._clip(clip)
        draw = (lambda x: self._randn_like_ahead(x, rng=rng)) if float(eta) > 0.0 else None
        bufs = (torch.empty_like(x), torch.empty_like(x))

        def update(x, prediction, noise, row, x0_prev):
            coef_i, second_i = row
            target = bufs[1] if x0_prev is bufs[0] else bufs[0]
            if draw is None and known is None:
                return _lib.dpm_step(x, prediction, x0_prev if second_i else None, coef_i, objective, clip, x0_out=target)
            return _lib.dpm_step_known(x, prediction, x0_prev if second_i else None, noise, known, mask, coef_i, objective, clip, x0_out=target)

        return self._run_loop(x, len(second), lambda i: (cond[i], (coef[i], second[i])), update, draw, progress, return_all, desc, cache=cache)

    def _transfer_table(self, steps: torch.Tensor, batch_size: int, dev):
        """``(cond (S,B), coef (S,B,4))`` on the device for DDIM transfers along ``steps`` (S+1,): the log-SNR of each step's start and
        ``(alpha_t, sigma_t, alpha_u, sigma_u)`` of its two ends, evaluated where ``schedule_on`` says (on the host row by row: see
        ``_rows``)."""
        cond = self._log_snr_of_steps(steps[:-1]).to(dev)
        rows = self._alpha_sigma_rows(steps).to(dev)
        coef = torch.cat([rows[:-1], rows[1:]], dim=-1)
        return cond[:, None].repeat_interleave(batch_size, dim=1).contiguous(), coef[:, None, :].repeat_interleave(batch_size, dim=1).contiguous()

    @torch.inference_mode()
    def invert(self, x_0, num_steps: int, t_end: float = 1.0, progress: bool = True, return_all: bool = False):
        """DDIM inversion: the deterministic encoding of ``x_0`` (B,C,H,W) into the latent at noise level ``t_end``, over
        ``linspace(0, t_end, num_steps + 1)``.  Per step one denoiser call at log-SNR(t_i) and one ``r2dm_ddim_transfer`` to t_{i+1} (the
        DDIM update with eta = 0 run towards more noise, unclipped); nothing is drawn.  ``sample_from(..., t_start=t_end, mode="ddim",
        clip=False)`` decodes the result.  -> x at ``t_end``; with ``return_all`` the (S+1,B,C,H,W) stack that starts with ``x_0``."""
        self._refuse_cpu("invert", x_0)
        _check_level(t_end, "t_end")
        if x_0.dim() != 4 or x_0.shape[0] < 1:
            raise ValueError(f"x_0 must be (B,C,H,W) with B >= 1, got {tuple(x_0.shape)}")
        objective = self._objective_id()
        x, dev = _lib.f32c(x_0), x_0.device
        steps = torch.linspace(0.0, float(t_end), num_steps + 1, device=dev if self._on_device(dev) else None)
        cond, coef = self._transfer_table(steps, x.shape[0], dev)
        return self._run_loop(x, num_steps, lambda i: (cond[i], coef[i]), lambda x, pred, _, k, __: (_ddim_transfer(x, pred, k, objective), None),
                              None, progress, return_all, desc="inverting")

    # -- forward process pieces used by RePaint (continuous_time.py:169-190) ----------------
    def _alpha_sigma_rows(self, steps: torch.Tensor) -> torch.Tensor:
        """(alpha, sigma) per row, float32, where ``schedule_on`` says (on the host row by row: see ``_rows``)."""
        return _rows(lambda t: torch.stack(log_snr_to_alpha_sigma(self._log_snr_1d(t)), dim=-1), *self._placed(steps)).contiguous()

    def _q_coef_rows(self, step_t: torch.Tensor, step_s: torch.Tensor) -> torch.Tensor:
        """(alpha_t/alpha_s, sqrt(sigma_t^2 - alpha_ts^2 sigma_s^2)) per row (continuous_time.py:181-189), evaluated as ``_alpha_sigma_rows``."""
        def rows(t, s):
            a_t, s_t = log_snr_to_alpha_sigma(self._log_snr_1d(t))
            a_s, s_s = log_snr_to_alpha_sigma(self._log_snr_1d(s))
            a_ts = a_t / a_s
            return torch.stack([a_ts, (s_t.pow(2) - a_ts.pow(2) * s_s.pow(2)).sqrt()], dim=-1)

        return _rows(rows, *self._placed(step_t, step_s)).contiguous()

    def q_step_from_x_0(self, x_0, step_t, rng=None):
        """Forward process q(z_t | x_0) (continuous_time.py:169-176); HIP kernel r2dm_q_step."""
        noise = self.randn_like(x_0, rng=rng)
        coef = self._alpha_sigma_rows(step_t).to(x_0.device)  # x_0 * alpha + sigma * noise
        return _lib.q_step(x_0, noise, coef), noise

    def q_step(self, x_s, step_t, step_s, rng=None):
        """q(z_t | z_s), 0 < s < t < 1 (continuous_time.py:178-190); HIP kernel r2dm_q_step."""
        coef = self._q_coef_rows(step_t, step_s).to(x_s.device)
        var_noise = self.randn_like(x_s, rng=rng)
        return _lib.q_step(x_s, var_noise, coef)

    @torch.inference_mode()
    def repaint(self, known, mask, num_steps: int, num_resample_steps: int = 1, jump_length: int = 1,
                progress: bool = True, rng=None, return_all: bool = False, cache_interval: int = 1, cache_depth: int = 1, cache_drift: bool = False):
        """RePaint inpainting on top of the same p_step (continuous_time.py:260-317).  A range-guard trip that only shows after the
        first step (``_early_check``) ends the loop with the denoiser switched to the wide-range split: the call is then repeated
        once, from the generator states it started with -- same draws, no exception (the reference runs any finite checkpoint)."""
        assert num_resample_steps > 0
        assert jump_length > 0
        _cache_opts("repaint", cache_interval, cache_depth, cache_drift, _NO_CACHE_IN_RESAMPLING)
        dev = self.device

        def prepare(r, k):
            return r[:, k], r[:, k + 1], self._alpha_sigma_rows(r[:, k + 1]).to(dev)

        def substep(x, row, early_check):
            # q_step_from_x_0(known) and the mask blend are one kernel; the draw order (known-region noise, then p_step's noise) is the reference's
            noise_k = self.randn_like(known, rng=rng)
            unknown_s = self.p_step(x, row[0], row[1], rng=rng, _early_check=early_check)
            return _lib.repaint_blend(known, noise_k, unknown_s, mask, row[2])

        def run():
            x_t = self.randn(known.shape[0], *self.sampling_shape, rng=rng, device=dev)
            return self._resample_walk(x_t, torch.linspace(1, 0, num_steps + 1), torch.linspace(0, 1, jump_length + 1), num_resample_steps, prepare,
                                       substep, progress, rng, return_all, "RePaint")

        return self._twice_on_fallback(rng, run)

    def _resample_walk(self, x_t, steps, frac, num_resample_steps: int, prepare, substep, progress: bool, rng, return_all: bool, desc: str):
        """The RePaint schedule (continuous_time.py:260-317) that ``repaint`` and ``complete`` share, from ``x_t`` over ``steps`` (S+1,): step i is
        J sub-steps along ``r = t + frac * (s - t)`` (``frac`` (J+1,) from 0 to 1), each ``substep(x, row, early_check) -> x`` with ``row =
        prepare(r, k)`` evaluated once per step and shared by its resamplings (``early_check``: the walk's number of denoiser calls on the first
        one, else 0); after a group of sub-steps ``q_step`` travels back and the group is repeated, ``num_resample_steps`` times in all -- not
        after the last resampling of a step, nor on the last step.  Under the deferred range guard.
        -> the last x_s, or with ``return_all`` the stack of ``x_t`` and every resampling's x_s."""
        B, num_steps, jump_length = x_t.shape[0], steps.numel() - 1, frac.numel() - 1
        steps = steps[None].repeat_interleave(B, dim=0)
        out = [x_t] if return_all else None
        x_s = x_t
        with _range_guard(self.model):
            for i in tqdm(range(num_steps), desc=desc, leave=False, disable=not progress):
                t, s = steps[:, [i]], steps[:, [i + 1]]
                r = t + frac[None] * (s - t)
                rows = [prepare(r, k) for k in range(jump_length)]
                for j in range(num_resample_steps):
                    x = x_t
                    for k in range(jump_length):
                        x = substep(x, rows[k], num_steps * num_resample_steps * jump_length if i == j == k == 0 else 0)
                    x_s = x
                    if return_all:
                        out.append(x_s)
                    if i == num_steps - 1 or j == num_resample_steps - 1:
                        x_t = x
                        break
                    for k in range(jump_length, 0, -1):
                        x = self.q_step(x, r[:, k - 1], r[:, k], rng=rng)
                    x_t = x
        return torch.stack(out) if return_all else x_s

    def _completion_args(self, what: str, known, mask, counts: dict, t_start, init, solver=None, mode=None):
        """The argument checks ``complete`` and ``complete_dpm`` share -> ``(known, mask, init)`` as the kernels take them: float32 and contiguous on
        ``known``'s device, the mask expanded over the batch.  ``solver``: ``complete_dpm``'s (order, grid, eta); ``mode``: ``complete``'s."""
        self._objective_id()
        C, H, W = self.sampling_shape
        if known.dim() != 4 or known.shape[0] < 1 or tuple(known.shape[1:]) != (C, H, W):
            raise ValueError(f"known must be (B, {C}, {H}, {W}) with B >= 1, got {tuple(known.shape)}")
        B = known.shape[0]
        if mask.dim() != 4 or mask.shape[0] not in (1, B) or mask.shape[1] not in (1, C) or tuple(mask.shape[2:]) != (H, W):
            raise ValueError(f"mask must be ({B} | 1, 1 | {C}, {H}, {W}), got {tuple(mask.shape)}")
        _check_count(**counts)
        if solver is not None:
            _check_solver(*solver)
        _check_level(t_start)
        if init is None and float(t_start) != 1.0:
            raise ValueError(f"t_start = {t_start} needs init (the x_0 that is noised to t_start): a fresh draw starts at t_start = 1")
        if init is not None and init.shape != known.shape:
            raise ValueError(f"init {tuple(init.shape)} must have known's shape {tuple(known.shape)}")
        if mode is not None and mode not in ("ddpm", "ddim"):
            raise ValueError(f"invalid mode {mode}")
        self._refuse_cpu(what, known)
        dev = known.device
        return _lib.f32c(known), _lib.f32c(mask.to(dev).expand(B, -1, H, W)), None if init is None else _lib.f32c(init.to(dev))

    def _completion_start(self, known, init, t_start: float, rng):
        """A completion's start tensor: ``randn(B, *sampling_shape)``, or ``init`` noised to ``t_start`` (one ``randn_like``)."""
        B, dev = known.shape[0], known.device
        if init is None:
            return self.randn(B, *self.sampling_shape, rng=rng, device=dev)
        return self.q_step_from_x_0(init, torch.full((B,), float(t_start), device=dev if self._on_device(dev) else None), rng=rng)[0]

    def _known_exact(self, out, known, mask, return_all: bool):
        """``exact_known``: the result, or with ``return_all`` the stack's last entry, becomes ``mask * known + (1 - mask) * x`` -- the blend kernel
        with known as its noise operand, mask * (known * 1 + known * 0) + (1 - mask) * x."""
        x_s = _lib.repaint_blend(known, known, out[-1] if return_all else out, mask, torch.tensor([[1.0, 0.0]], device=known.device).repeat(known.shape[0], 1))
        if not return_all:
            return x_s
        out[-1] = x_s
        return out

    # -- data-consistent completion (DDNM's null-space projection for a mask operator; not in the reference) ----------------
    @torch.inference_mode()
    def complete(self, known, mask, num_steps: int, num_resample_steps: int = 1, jump_length: int = 1, t_start: float = 1.0, init=None,
                 mode: Literal["ddpm", "ddim"] = "ddpm", ddim_eta: float = 0.0, exact_known: bool = True, progress: bool = True, rng=None,
                 return_all: bool = False, cache_interval: int = 1, cache_depth: int = 1, cache_drift: bool = False):
        """Completion of ``known`` (B,C,H,W) under ``mask`` (B | 1, 1 | C, H, W; 1 = measured, any weight in [0, 1] is taken as such) with
        one denoiser call per reverse sub-step: the clamped estimate of x_0 gets the measurement written over its known pixels,
        ``x0 = mask * known + (1 - mask) * x0``, and x_s is sampled from the ordinary posterior given that x_0 -- one fused kernel
        (``r2dm_posterior_step_known``) and one noise draw, no known-region noise and no separate blend (Wang, Yu, Zhang: DDNM, ICLR 2023).

        The schedule is ``repaint``'s over ``linspace(t_start, 0, num_steps + 1)``: step i is ``jump_length`` sub-steps along
        ``t + linspace(0, 1, jump_length + 1) * (s - t)``; after a group of reverse sub-steps ``q_step`` travels back and the group is
        repeated, ``num_resample_steps`` times in all (not after the last one of a step, nor on the last step).  ``num_resample_steps = 1``
        is a valid sampler of its own.  Draw order: the start (``init=None``: ``randn(B, *sampling_shape)`` at ``t_start = 1``; else
        ``q_step_from_x_0(init, t_start)``, one ``randn_like``), one ``randn_like`` per denoiser call in every mode (as ``p_step``), one per
        forward sub-step.  With an all-zero mask and ``num_resample_steps = jump_length = 1`` this is ``sample`` / ``sample_from`` on the same
        draws.  ``exact_known``: the result is ``mask * known + (1 - mask) * x`` (``r2dm_repaint_blend``), equal to ``known`` on a binary
        mask; without it the known pixels carry the last step's ``sigma(0) * z``.  ``return_all``: the stack ``repaint`` returns -- the
        start, then the x_s of every resampling, the last one projected like the result.  A range-guard trip is handled as in ``repaint``:
        the call is repeated once on the wide-range split from the generator states it started with.
        ``cache_interval`` other than 1 is refused (the resampling walk; ``complete_dpm`` is the completion that takes a feature cache)."""
        _cache_opts("complete", cache_interval, cache_depth, cache_drift, _NO_CACHE_IN_RESAMPLING)
        known, mask, init = self._completion_args("complete", known, mask, dict(num_steps=num_steps, num_resample_steps=num_resample_steps,
                                                                                jump_length=jump_length), t_start, init, mode=mode)
        dev = known.device
        where = dev if self._on_device(dev) else None  # (the grid itself is then the device's linspace, as in _table_rows)
        objective, clip = self._objective_id(), self._clip()

        def prepare(r, k):
            cond, coef, mode_id = self._coefficients(r[:, k], r[:, k + 1], mode, float(ddim_eta))
            return cond.to(dev), coef.to(dev), mode_id

        def substep(x, row, early_check):
            cond, coef, mode_id = row
            noise, drawn = self._randn_like_ahead(x, rng=rng)
            prediction = self._denoise(x, cond, early_check)
            if drawn is not None:
                torch.cuda.current_stream(dev).wait_event(drawn)
            return _lib.posterior_step_known(x, prediction, noise, known, mask, coef, mode_id, objective, clip)

        def run():
            out = self._resample_walk(self._completion_start(known, init, t_start, rng), torch.linspace(float(t_start), 0.0, int(num_steps) + 1, device=where),
                                      torch.linspace(0, 1, int(jump_length) + 1, device=where), int(num_resample_steps), prepare, substep, progress,
                                      rng, return_all, "completing")
            return self._known_exact(out, known, mask, return_all) if exact_known else out

        return self._twice_on_fallback(rng, run)

    # -- completion on DPM-Solver++(2M): the projection of ``complete`` inside the multistep solver's update (not in the reference) --------
    @torch.inference_mode()
    def complete_dpm(self, known, mask, num_steps: int, order: int = 2, grid: Literal["logsnr", "time"] = "logsnr", eta: float = 1.0,
                     t_start: float = 1.0, init=None, exact_known: bool = True, clip: Optional[bool] = None, lower_order_final: bool = True,
                     progress: bool = True, rng=None, return_all: bool = False, cache_interval: int = 1, cache_depth: int = 1, cache_drift: bool = False):
        """Completion of ``known`` (B,C,H,W) under ``mask`` (B | 1, 1 | C, H, W; 1 = measured, any weight in [0, 1] is taken as such) on
        ``sample_dpm``'s solver: per step one denoiser call and one ``r2dm_dpm_step_known``, which forms the clamped estimate of x_0, writes
        the measurement over it (``x0 = mask * known + (1 - mask) * x0``, ``complete``'s projection), keeps THAT as the next step's history
        and takes the multistep update from it, plus ``c_z`` times the step's noise.  ``num_steps``, ``order``, ``grid``, ``clip`` and
        ``lower_order_final`` are ``sample_dpm``'s; the table is ``_dpm_table(..., eta)``.

        ``eta``: the share of each step's noise that is drawn anew.  Default 1 (SDE-DPM-Solver++(2M)): it continues ``complete``'s default,
        the ancestral posterior, which is this sampler at order 1 on the time grid -- fresh noise is what lets the unknown region
        re-harmonise with the pixels that were written in.  ``eta = 0`` is the deterministic solver with hard replacement.
        Draw order: the start (``init=None``: ``randn(B, *sampling_shape)`` at ``t_start = 1``; else ``q_step_from_x_0(init, t_start)``, one
        ``randn_like``), then one ``randn_like`` per step when ``eta > 0`` (ahead of the denoiser call, on the side stream), none when
        ``eta == 0``.  With an all-zero mask this is ``sample_dpm`` with the same ``eta`` on the same draws.
        There is NO resampling (``num_resample_steps`` / ``jump_length`` of ``complete`` and ``repaint``): a travel back through ``q_step``
        lands on a state that the kept estimate of x_0 was not formed from, so it invalidates the multistep history.
        ``exact_known``: the result is ``mask * known + (1 - mask) * x`` (``r2dm_repaint_blend``), equal to ``known`` on a binary mask.
        ``return_all``: the (S+1,B,C,H,W) stack from the start, the last entry projected like the result.
        A range-guard trip is handled by ``_Replay`` as in ``sample_dpm``: back at most ``_CHECK_EVERY`` steps with the checkpointed pair
        (x, previous estimate), on the recorded noise, on the wide-range split.
        ``cache_interval``, ``cache_depth``, ``cache_drift``: the feature cache, as in ``sample_dpm``."""
        cache = _cache_opts("complete_dpm", cache_interval, cache_depth, cache_drift)
        known, mask, init = self._completion_args("complete_dpm", known, mask, dict(num_steps=num_steps), t_start, init, solver=(order, grid, eta))
        out = self._dpm_solve(self._completion_start(known, init, t_start, rng), num_steps, order, grid, t_start, lower_order_final, eta, clip, progress,
                              rng, return_all, known, mask, desc="completing", cache=cache)
        return self._known_exact(out, known, mask, return_all) if exact_known else out


# --------------------------------------------------------------------------------------
class DiscreteTimeGaussianDiffusion(GaussianDiffusion):
    """DDPM / DDIM over an integer-step beta schedule (discrete_time.py:51-201)."""

    def setup_parameters(self) -> None:
        assert self.num_training_steps is not None
        beta, ab, abp, snr = discrete_tables(self.num_training_steps, self.noise_schedule)
        v4 = lambda t: t[:, None, None, None]
        self.register_buffer("beta", v4(beta))
        self.register_buffer("alpha_bar", v4(ab))
        self.register_buffer("alpha_bar_prev", v4(abp))
        self.register_buffer("snr", v4(snr))

    def get_network_condition(self, steps):
        return steps

    # -- the denoising loss's pieces (discrete_time.py:80-124) -----------------------------
    def sample_timesteps(self, batch_size: int, device) -> torch.Tensor:
        return torch.randint(low=0, high=self.num_training_steps, size=(batch_size,), device=device, dtype=torch.long)

    def _log_snr_of_steps(self, steps) -> torch.Tensor:
        """(B,) ``log(snr[steps])`` where ``schedule_on`` says: on the host row by row (a row does not depend on the batch), or on the device."""
        whole = self._on_device(steps.device)
        snr = self.snr if whole else self.snr.detach().cpu()
        return _rows(torch.log, whole, [snr[steps.detach().to(snr.device, torch.long).reshape(-1), 0, 0, 0]])

    def _loss_coef(self, steps) -> torch.Tensor:
        """(sqrt(alpha_bar), sqrt(1 - alpha_bar)) rows on the host (discrete_time.py:122-123).  The roots are taken in float64 and rounded
        to float32 -- the correctly rounded float32 root, which a GPU's float32 sqrt also gives: torch's float32 sqrt on a CPU is not
        correctly rounded on every host (measured: 9 of the 1000 steps' roots one ulp off on one host, 213 on another)."""
        ab = self.alpha_bar.detach().cpu()[steps.detach().to("cpu", torch.long).reshape(-1), 0, 0, 0]
        return torch.stack([ab.double().sqrt().float(), (1 - ab).double().sqrt().float()], dim=-1).contiguous()

    def get_target(self, x_0, steps, noise):
        """discrete_time.py:93-102, in torch (the fused loss kernel does not call this; the tests compare it with that kernel)."""
        if self.objective == "eps":
            return noise
        if self.objective == "x_0":
            return x_0
        if self.objective == "v":
            alpha_bar = self.alpha_bar.to(x_0.device)[steps.to(x_0.device)]
            return alpha_bar.sqrt() * noise - (1 - alpha_bar).sqrt() * x_0
        raise ValueError(f"invalid objective {self.objective}")

    def get_loss_weight(self, timesteps):
        """(B,1,1,1) min-SNR loss weights (discrete_time.py:104-117): a table lookup, a clamp and one division -- the same bits on
        the host and on the device."""
        return self._loss_weight_of_snr(self.snr[timesteps.to(self.snr.device)])

    def q_step_from_x_0(self, x_0, steps, rng=None):
        """Forward process q(x_t | x_0) (discrete_time.py:119-124); HIP kernel r2dm_q_step, which replays the reference's operation
        order (two products, one sum): the same bits as the reference's expression."""
        noise = self.randn_like(x_0, rng=rng)
        return _lib.q_step(x_0, noise, self._loss_coef(steps).to(x_0.device)), noise

    def _coefficients(self, steps: torch.Tensor, mode: str, eta: float):
        """Row scalars of discrete_time.py:135-177 on the host (float32, same op order)."""
        idx = steps.detach().to("cpu", torch.long)
        beta = self.beta.detach().cpu()[idx, 0, 0, 0]
        ab = self.alpha_bar.detach().cpu()[idx, 0, 0, 0]
        abp = self.alpha_bar_prev.detach().cpu()[idx, 0, 0, 0]
        alpha = 1 - beta
        live = (idx != 0).float()  # var_noise[steps == 0] *= 0 (discrete_time.py:162,176)
        if self.objective == "eps":
            k0, k1 = ab.rsqrt(), (ab.reciprocal() - 1).sqrt()
        elif self.objective == "v":
            k0, k1 = ab.sqrt(), (1 - ab).sqrt()
        else:
            k0 = k1 = torch.zeros_like(ab)
        if mode == "ddpm":
            x0c = abp.sqrt() * beta / (1 - ab)
            xtc = (1 - abp) * alpha.sqrt() / (1 - ab)
            var = (beta * (1 - abp) / (1 - ab)).clamp(min=1e-20)
            sd = (0.5 * var.log()).exp() * live
            coef = torch.stack([k0, k1, x0c, xtc, sd, torch.zeros_like(ab), torch.zeros_like(ab),
                                torch.zeros_like(ab)], dim=-1)
            return coef.contiguous(), _M_DT_DDPM
        if mode == "ddim":
            var = (1 - abp) / (1 - ab) * (1 - ab / abp)
            std = eta * torch.sqrt(var)
            coef = torch.stack([k0, k1, ab.sqrt(), (1 - ab).sqrt(), (1 - abp - std**2).sqrt(), abp.sqrt(),
                                std * live, torch.zeros_like(ab)], dim=-1)
            return coef.contiguous(), (_M_DT_DDIM_NOISE if eta > 0 else _M_DT_DDIM)
        raise ValueError(f"invalid mode {mode}")

    @torch.inference_mode()
    def p_step(self, x_t, steps, rng=None, mode: Literal["ddpm", "ddim"] = "ddim", eta: float = 0.0):
        self._objective_id()
        coef, mode_id = self._coefficients(steps, mode, eta)
        prediction = self.model(x_t, steps.to(x_t.device))
        # draw order as the reference: DDPM always draws; DDIM only when eta > 0 (:160,:174)
        noise = self.randn_like(x_t, rng=rng) if mode_id != _M_DT_DDIM else None
        return self._posterior(x_t, prediction, noise, coef.to(x_t.device), mode_id)

    @torch.inference_mode()
    def sample(self, batch_size: int, num_steps: int, progress: bool = True, rng=None,
               return_all: bool = False, mode: Literal["ddpm", "ddim"] = "ddpm", cache_interval: int = 1, cache_depth: int = 1, cache_drift: bool = False):
        """t = num_steps-1 ... 0 without respacing (discrete_time.py:182-201).  ``cache_interval`` other than 1 is refused: the feature cache is
        wired into the continuous-time samplers only."""
        _cache_opts("DiscreteTimeGaussianDiffusion.sample", cache_interval, cache_depth, cache_drift,
                    "the feature cache is implemented for the continuous-time samplers (sample, sample_from, sample_dpm, complete_dpm) only")
        dev = self.device
        self._objective_id()
        x = self.randn(batch_size, *self.sampling_shape, rng=rng, device=dev)
        order = torch.arange(num_steps - 1, -1, -1)
        coef, mode_id = self._coefficients(order, mode, 0.0)
        coef = coef[:, None, :].expand(num_steps, batch_size, _NCOEF).contiguous().to(dev)
        cond = order[:, None].expand(num_steps, batch_size).contiguous().to(dev)
        draw = (lambda x: self._randn_like_ahead(x, rng=rng)) if mode_id != _M_DT_DDIM else None
        return self._run_loop(x, num_steps, lambda i: (cond[i], coef[i]), lambda x, pred, noise, k, _: (self._posterior(x, pred, noise, k, mode_id), None),
                              draw, progress, return_all)

    def invert(self, *args, **kwargs):
        raise NotImplementedError("invert is implemented for continuous time only (ContinuousTimeGaussianDiffusion)")

    def sample_from(self, *args, **kwargs):
        raise NotImplementedError("sample_from is implemented for continuous time only (ContinuousTimeGaussianDiffusion)")

    def complete(self, *args, **kwargs):
        raise NotImplementedError("complete is implemented for continuous time only (ContinuousTimeGaussianDiffusion)")

    def sample_dpm(self, *args, **kwargs):
        raise NotImplementedError("sample_dpm is implemented for continuous time only (ContinuousTimeGaussianDiffusion)")

    def complete_dpm(self, *args, **kwargs):
        raise NotImplementedError("complete_dpm is implemented for continuous time only (ContinuousTimeGaussianDiffusion)")
