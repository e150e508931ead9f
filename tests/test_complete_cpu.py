"""Data-consistent completion without a GPU: the oracle of ``ContinuousTimeGaussianDiffusion.complete`` (tests/complete_oracle.py) against the
oracle's own sampler and its defining properties, the draw count, and what ``complete``, ``evaluate_completion`` and the two scripts refuse or
accept before anything reaches a kernel."""
from pathlib import Path

import pytest
import torch

from conftest import GOLDEN_RES, rnd, synthetic_ckpt

import complete_oracle as CO
import latent_oracle as LO

from oracle import r2dm_oracle as O

B = 3
SHAPE = (B, 2, *GOLDEN_RES)


def tape_for(S, r=1, j=1, seed=200):
    return [rnd(seed + n, *SHAPE) for n in range(CO.num_draws(S, r, j))]


def binary_mask(seed=5):
    g = torch.Generator().manual_seed(seed)
    mask = (torch.rand(B, 1, *GOLDEN_RES, generator=g) < 0.5).double()
    mask[1] = 0
    mask[1, :, ::4] = 1  # every fourth beam
    return mask


@pytest.mark.parametrize("mode,eta", [("ddpm", 0.0), ("ddim", 0.0), ("ddim", 0.5)])
def test_with_nothing_known_the_loop_is_the_oracles_sampler(mode, eta):
    """mask = 0: the projection leaves the estimate as it is (0 * y + 1 * x0), so the loop is ``O.sample_continuous`` on the same tape, bit for bit
    (S = 4: the grid and ``t + 1 * (s - t)`` are exact)"""
    S = 4
    tape = [t.double() for t in tape_for(S)]
    known = torch.tanh(rnd(70, *SHAPE)).double()
    zero = torch.zeros(B, 1, *GOLDEN_RES, dtype=torch.float64)
    got = CO.complete(LO.analytic_eps, known, zero, S, tape, mode=mode, ddim_eta=eta, return_all=True)
    # (``O.sample_continuous`` builds its grid in float32 whatever ``dtype``: 1, 0.75, 0.5, 0.25, 0 are the same numbers in float64, and the
    # schedule is evaluated on them in float64 here as it is there)
    log_snr64 = lambda t: O.log_snr_cosine(t.double())
    want = O.sample_continuous(LO.analytic_eps, SHAPE, S, noises=tape, return_all=True, mode=mode, ddim_eta=eta, dtype=torch.float64, log_snr=log_snr64)
    assert got.dtype == want.dtype == torch.float64 and got.shape == (S + 1, *SHAPE)
    assert torch.equal(got, want)
    # ... and in float32, where the grid has the run's dtype there too
    tape32 = [t.float() for t in tape]
    assert torch.equal(CO.complete(LO.analytic_eps, known.float(), zero.float(), S, tape32, mode=mode, ddim_eta=eta, return_all=True),
                       O.sample_continuous(LO.analytic_eps, SHAPE, S, noises=tape32, return_all=True, mode=mode, ddim_eta=eta))


def test_known_pixels_are_exact_and_the_rest_ignores_what_the_mask_hides():
    S, r, j = 3, 2, 2
    tape = [t.double() for t in tape_for(S, r, j)]
    known = torch.tanh(rnd(70, *SHAPE)).double()
    mask = binary_mask()
    on = mask.expand_as(known) == 1
    assert 0 < on.sum() < on.numel()
    got = CO.complete(LO.analytic_eps, known, mask, S, tape, r, j)
    assert torch.equal(got[on], known[on])
    other = torch.where(on, known, torch.tanh(rnd(71, *SHAPE)).double())  # other values where the mask is 0
    assert not torch.equal(other, known)
    assert torch.equal(CO.complete(LO.analytic_eps, other, mask, S, tape, r, j), got)
    # without the final projection the known pixels carry the last step's sigma(0) z: close to alpha(0) known, not equal to known
    raw = CO.complete(LO.analytic_eps, known, mask, S, tape, r, j, exact_known=False)
    a0, s0 = O.alpha_sigma(O.log_snr_cosine(torch.zeros(1, dtype=torch.float64)))
    dev = (raw - a0 * known)[on].abs().max().item()
    assert 0 < dev <= 6 * s0.item() * max(t.abs().max().item() for t in tape)
    assert torch.equal(raw[~on], got[~on])
    # the weight form: m = 1/4 is neither, and the stack has one entry per resampling
    stack = CO.complete(LO.analytic_eps, known, torch.full_like(mask, 0.25), S, tape, r, j, return_all=True)
    assert stack.shape == (1 + S * r - (r - 1), *SHAPE) and torch.isfinite(stack).all()


@pytest.mark.parametrize("S,r,j,init", [(4, 1, 1, False), (3, 2, 2, False), (3, 2, 1, True)])
def test_the_tape_is_the_draw_count(S, r, j, init):
    """one draw for the start (a fresh one or ``q_step_from_x_0(init)``), one per denoiser call, one per forward sub-step: a tape one short or
    one long raises"""
    calls = []

    def denoise(x, c):
        calls.append(c)
        return LO.analytic_eps(x, c)

    n = CO.num_draws(S, r, j)
    assert n == {(4, 1, 1): 5, (3, 2, 2): 15, (3, 2, 1): 8}[(S, r, j)]
    tape = [rnd(300 + k, *SHAPE) for k in range(n + 1)]
    known = torch.tanh(rnd(70, *SHAPE))
    mask = binary_mask().float()
    kw = dict(init=0.5 * known, t_start=0.5) if init else {}
    CO.complete(denoise, known, mask, S, tape[:n], r, j, **kw)
    groups = (S - 1) * r + 1
    assert len(calls) == j * groups and n == 1 + len(calls) + j * (S - 1) * (r - 1)
    for bad in (tape[:n - 1], tape):
        with pytest.raises(ValueError, match="draws"):
            CO.complete(denoise, known, mask, S, bad, r, j, **kw)
    with pytest.raises(ValueError, match="init"):
        CO.complete(denoise, known, mask, S, tape[:n], r, j, t_start=0.5)


def cpu_model():
    import r2dm_amd

    return r2dm_amd.setup_model(synthetic_ckpt(resolution=GOLDEN_RES), device="cpu", show_info=False)[0]


def test_complete_on_a_cpu_model_raises_no_cpu_fallback():
    import r2dm_amd
    from r2dm_amd.diffusion import NoCPUFallback

    ddpm = cpu_model()
    known, mask = torch.zeros(1, 2, *GOLDEN_RES), torch.ones(1, 1, *GOLDEN_RES)
    state = torch.get_rng_state()
    for kw in ({}, dict(init=known, t_start=0.5), dict(mode="ddim", num_resample_steps=2, jump_length=2, mask=torch.ones(1, 2, *GOLDEN_RES))):
        with pytest.raises(NoCPUFallback, match="no CPU fallback"):
            ddpm.complete(**{"known": known, "mask": mask, "num_steps": 2, "progress": False, **kw})
    assert torch.equal(torch.get_rng_state(), state)  # (refused before anything is drawn)
    discrete = r2dm_amd.DiscreteTimeGaussianDiffusion(ddpm.model, num_training_steps=10)
    with pytest.raises(NotImplementedError, match="continuous time only"):
        discrete.complete(known, mask, 2)


def test_complete_refuses_malformed_arguments():
    ddpm = cpu_model()
    H, W = GOLDEN_RES
    known, mask = torch.zeros(2, 2, H, W), torch.ones(2, 1, H, W)
    bad = [
        dict(known=torch.zeros(2, 2, H, W + 4)), dict(known=torch.zeros(2, 3, H, W)), dict(known=torch.zeros(2, H, W)),
        dict(mask=torch.ones(3, 1, H, W)), dict(mask=torch.ones(2, 3, H, W)), dict(mask=torch.ones(2, 1, H, W // 2)), dict(mask=torch.ones(H, W)),
        dict(num_steps=0), dict(num_resample_steps=0), dict(jump_length=0), dict(jump_length=-1),
        dict(t_start=0.0, init=known), dict(t_start=1.5, init=known), dict(t_start=-0.5, init=known),
        dict(init=torch.zeros(2, 2, H, W + 4), t_start=0.5), dict(init=torch.zeros(1, 2, H, W), t_start=0.5),
        dict(t_start=0.5),  # (no init)
        dict(mode="ode"),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            ddpm.complete(**{"known": known, "mask": mask, "num_steps": 2, "progress": False, **kw})


def test_the_method_and_the_parsers_take_the_new_names():
    import completion_demo
    import completion_eval
    from r2dm_amd import completion

    assert "ddnm" in completion.METHODS and set(completion.METHODS) >= {"repaint", "nearest", "linear", "target"}
    # the defaults are what they were; the new options come on top
    ns = vars(completion_eval.build_parser().parse_args(["--ckpt", "c.pth"]))
    new = {"ddnm_resample_steps": 1, "ddnm_init": "none", "ddnm_t_start": 1.0}
    old = {"ckpt": Path("c.pth"), "real_scans": None, "real_dir": None, "limit": None, "corruption": None, "methods": ["repaint"], "num_steps": 32,
           "num_resample_steps": 10, "jump_length": 1, "batch_size": 8, "seed": 0, "rangenet_weights": None, "semseg_postprocess": "none",
           "chamfer": False, "fscore_threshold": 0.2, "save_dir": None, "out": "completion.json"}
    assert ns == {**old, **new}
    ns = vars(completion_eval.build_parser().parse_args(["--ckpt", "c.pth", "--methods", "repaint", "ddnm", "linear", "--ddnm_resample_steps", "3",
                                                         "--ddnm_init", "linear", "--ddnm_t_start", "0.5"]))
    assert ns["methods"] == ["repaint", "ddnm", "linear"] and (ns["ddnm_resample_steps"], ns["ddnm_init"], ns["ddnm_t_start"]) == (3, "linear", 0.5)
    with pytest.raises(SystemExit):
        completion_eval.build_parser().parse_args(["--ckpt", "c.pth", "--ddnm_init", "cubic"])
    ns = vars(completion_demo.parser().parse_args(["--ckpt", "c.pth", "--scan", "s.bin"]))
    assert ns == {"ckpt": Path("c.pth"), "num_steps": 32, "num_resample_steps": 16, "jump_length": 1, "seed": 0, "scan": Path("s.bin"), "out": None,
                  "rangenet_weights": None, "semseg_postprocess": "none", "out_scan": None, "method": "repaint"}
    assert completion_demo.parser().parse_args(["--ckpt", "c.pth", "--scan", "s.bin", "--method", "ddnm"]).method == "ddnm"
    with pytest.raises(SystemExit):
        completion_demo.parser().parse_args(["--ckpt", "c.pth", "--scan", "s.bin", "--method", "repaint2"])


def test_evaluate_completion_refuses_an_init_without_a_start_and_the_reverse():
    """(checked before the planes are looked at: ``ddnm_init`` and ``ddnm_t_start`` < 1 only go together)"""
    from r2dm_amd import completion

    planes = torch.zeros(1, 6, *GOLDEN_RES)
    for kw in (dict(ddnm_init="linear"), dict(ddnm_t_start=0.5), dict(ddnm_init="cubic", ddnm_t_start=0.5), dict(ddnm_init="linear", ddnm_t_start=0.0),
               dict(ddnm_resample_steps=0)):
        with pytest.raises(ValueError, match="ddnm"):
            completion.evaluate_completion(None, None, planes, ["beams:4"], methods=("ddnm",), **kw)
