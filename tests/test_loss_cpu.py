"""The denoising loss's host side, without a GPU: timestep draws, the torch target and loss weight against the reference's values
(tests/golden/loss.npz, written by tests/golden/make_golden_loss.py from the reference's own run), the refusal on a CPU model, the C
ABI's argument checks and the level grids of the loss curve."""
import copy

import numpy as np
import pytest
import torch

from conftest import GOLDEN_RES, synthetic_ckpt

CASES = {"ct": (dict(), ("eps", "v", "x_0")),
         "dt": (dict(timestep_type="discrete", num_training_steps=1000, noise_schedule="linear"), ("eps", "v"))}


def build(tt, obj, device="cpu", loss_type="l2", **kw):
    import r2dm_amd

    ck = synthetic_ckpt(resolution=GOLDEN_RES, prediction_type=obj, **CASES[tt][0])
    if loss_type != "l2":
        ck = copy.deepcopy(ck)
        ck["cfg"]["diffusion"]["loss_type"] = loss_type
    return r2dm_amd.setup_model(ck, device=device, show_info=False, **kw)[0]


def test_sample_timesteps_dtype_range_shape():
    c, d = build("ct", "eps"), build("dt", "eps")
    torch.manual_seed(5)
    t = c.sample_timesteps(4096, "cpu")
    assert t.shape == (4096,) and t.dtype == torch.float32 and t.device.type == "cpu"
    assert 0.0 <= t.min().item() and t.max().item() < 1.0 and t.min().item() < 0.01 and t.max().item() > 0.99
    torch.manual_seed(5)
    assert torch.equal(t, torch.rand(4096, dtype=torch.float32))  # the reference's draw (continuous_time.py:133-135)
    torch.manual_seed(6)
    s = d.sample_timesteps(4096, "cpu")
    assert s.shape == (4096,) and s.dtype == torch.long
    assert s.min().item() >= 0 and s.max().item() <= 999 and s.min().item() < 10 and s.max().item() > 989
    torch.manual_seed(6)
    assert torch.equal(s, torch.randint(0, 1000, (4096,), dtype=torch.long))  # discrete_time.py:80-88


@pytest.mark.parametrize("tt", ["ct", "dt"])
def test_target_and_loss_weight_match_the_reference_bit_for_bit(golden, tt):
    """schedule_on="host" (the default): the same float32 values as the reference's CPU run."""
    g = golden("loss")
    x_0, noise, steps = g["x_0"], g["noise"], g[f"{tt}_steps"]
    snr_on_both_sides = False
    for obj in CASES[tt][1]:
        d = build(tt, obj)
        assert d.schedule_on == "host"
        target = d.get_target(x_0, steps, noise)
        want = {"eps": noise, "x_0": x_0, "v": g[f"{tt}_v_target"]}[obj]
        assert torch.equal(target, want), obj
        for on in (True, False):
            d.min_snr_loss_weight = on
            w = d.get_loss_weight(steps)
            assert w.shape == (4, 1, 1, 1) and w.dtype == torch.float32  # the reference's shape
            assert torch.equal(w.reshape(4), g[f"{tt}_{obj}_w{int(on)}"]), (obj, on)
        if obj == "eps":  # clipped / snr: 1 where the clamp is off, < 1 where it is on
            w1 = g[f"{tt}_eps_w1"]
            snr_on_both_sides = bool((w1 == 1).any() and (w1 < 1).any())
        assert torch.equal(d._loss_coef(steps), g[f"{tt}_alpha_sigma"])
        cond = d.get_network_condition(steps)  # per-sample steps
        assert cond.shape == (4,)
    assert snr_on_both_sides, "the fixture must have the min-SNR clamp on for one step and off for another"
    with pytest.raises(ValueError, match="invalid objective"):
        d.objective = "score"
        d.get_loss_weight(steps)


def test_loss_on_a_cpu_model_raises_one_error_of_both_kinds():
    from r2dm_amd import _lib
    from r2dm_amd.diffusion import NoCPUFallback

    assert issubclass(NoCPUFallback, _lib.R2DMError) and issubclass(NoCPUFallback, NotImplementedError)
    for tt in CASES:
        d = build(tt, "eps")
        x = torch.zeros(1, 2, *GOLDEN_RES)
        state = torch.get_rng_state()
        for call in (lambda: d(x), lambda: d.forward(x, None), lambda: d.p_loss(x, d.sample_timesteps(1, "cpu")),
                     lambda: d.loss_terms(x, d.sample_timesteps(1, "cpu"))):
            with pytest.raises(NoCPUFallback, match="no CPU fallback") as e:
                call()
            assert isinstance(e.value, NotImplementedError) and isinstance(e.value, _lib.R2DMError)
        torch.set_rng_state(state)


def _abi():
    from r2dm_amd import _lib

    L = _lib.lib()

    def call(pred=4096, x_0=8192, noise=12288, mask=None, mask_c=0, coef=None, objective=0, criterion=0, B=2, C=2, plane=64, scratch=16384,
             num=20480, den=24576):
        rc = L.r2dm_diffusion_loss(pred, x_0, noise, mask, mask_c, coef, objective, criterion, B, C, plane, scratch, num, den, None)
        return rc, L.r2dm_last_error().decode()

    return L, call


def test_c_abi_refuses_bad_arguments_with_a_status():
    """Every refusal is a status and a message, decided before anything touches a GPU (the pointers here are made-up addresses)."""
    _, call = _abi()
    for null in ("pred", "x_0", "noise", "scratch", "num", "den"):
        rc, msg = call(**{null: None})
        assert rc == 1 and "null argument" in msg, null
    rc, msg = call(objective=1, coef=None)
    assert rc == 1 and "null argument" in msg and "coef" in msg
    for mask_c in (0, 3, -1):
        rc, msg = call(mask=28672, mask_c=mask_c)
        assert rc == 1 and "mask_channels must be 1 or 2" in msg, mask_c
    for objective in (-1, 3):
        rc, msg = call(objective=objective)
        assert rc == 1 and "objective must be" in msg
    for criterion in (-1, 3):
        rc, msg = call(criterion=criterion)
        assert rc == 1 and "criterion must be" in msg
    for name in ("pred", "x_0", "noise"):  # a plane that is a multiple of 4 is read as 16-byte quads
        rc, msg = call(**{name: 4096 + 4})
        assert rc == 1 and "16-byte aligned" in msg, name
    rc, msg = call(mask=28672 + 8, mask_c=1)
    assert rc == 1 and "16-byte aligned" in msg
    rc, msg = call(pred=4096 + 2, plane=63)  # any other plane element by element: 4-byte alignment
    assert rc == 1 and "4-byte aligned" in msg
    for name in ("scratch", "num", "den"):
        rc, msg = call(**{name: 16384 + 4})
        assert rc == 1 and "8-byte aligned" in msg, name
    rc, msg = call(objective=1, coef=4096 + 2)
    assert rc == 1 and "coef must be 4-byte aligned" in msg
    for geometry in (dict(B=0), dict(B=-1), dict(C=0), dict(plane=0), dict(B=65536), dict(C=65536), dict(plane=1 << 41)):
        rc, msg = call(**geometry)
        assert rc == 1 and "batch and channels must be in" in msg, geometry


def test_scratch_bytes_is_monotone_and_zero_for_an_empty_batch():
    L, _ = _abi()
    f = L.r2dm_diffusion_loss_scratch_bytes
    for empty in ((0, 2, 2048), (-1, 2, 2048), (2, 0, 2048), (2, 2, 0), (2, 2, -5)):
        assert f(*empty) == 0, empty
    assert f(1, 1, 1) >= 16  # at least one (loss sum, mask sum) pair of doubles
    planes = [1, 3, 4, 1023, 1024, 1025, 2048, 16 * 1024, 16 * 1024 + 1, 65536, 1 << 24]
    for B in (1, 2, 7):
        for C in (1, 2, 3):
            sizes = [f(B, C, p) for p in planes]
            assert all(s > 0 and s % 8 == 0 for s in sizes)
            assert sizes == sorted(sizes), (B, C, sizes)
            assert f(B + 1, C, 2048) > f(B, C, 2048) and f(B, C + 1, 2048) > f(B, C, 2048)
    assert f(8, 2, 65536) == f(8, 2, 1 << 24)  # the grid is capped: large planes take several grid-stride passes


def test_loss_curve_level_grids():
    from r2dm_amd.loss import level_grid

    c, d = build("ct", "eps"), build("dt", "eps")
    t = level_grid(c, 16)
    assert t.dtype == torch.float32 and t.shape == (16,)
    assert torch.equal(t, torch.tensor([(k + 0.5) / 16 for k in range(16)], dtype=torch.float32))
    assert np.allclose(level_grid(c, 3).numpy(), [1 / 6, 0.5, 5 / 6], rtol=1e-7)
    assert torch.equal(level_grid(c, 1), torch.tensor([0.5]))
    s = level_grid(d, 4)
    assert s.dtype == torch.long and s.tolist() == [0, 333, 666, 999]
    s = level_grid(d, 16)
    assert s[0].item() == 0 and s[-1].item() == 999 and len(set(s.tolist())) == 16
    gaps = (s[1:] - s[:-1]).tolist()
    assert max(gaps) - min(gaps) <= 1  # evenly spaced, to the integer
    assert level_grid(d, 1000).tolist() == list(range(1000)) and level_grid(d, 1).tolist() == [0]
    for bad in (0, -2):
        with pytest.raises(ValueError):
            level_grid(c, bad)
    with pytest.raises(ValueError):
        level_grid(d, 1001)
