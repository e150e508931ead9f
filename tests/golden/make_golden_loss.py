#!/usr/bin/env python3
"""Generate tests/golden/loss.npz by running the REAL reference's denoising loss (models/diffusion/base.py:122-149) on the CPU.

Runs only where the reference is checked out (the pattern of make_golden.py: noise tape instead of ``randn``, synthetic weights by
(config, seed), 16 x 128); the emitted file is data -- inputs and the reference's outputs.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_loss.py

Per time type TT ("ct": continuous / cosine, objectives eps, v, x_0, steps 0.02, 0.3, 0.7, 0.98; "dt": discrete, T = 1000, linear, objectives
eps, v, steps 0, 10, 500, 999), B = 4:
  x_0, noise, mask_m1 (B,1,H,W), mask_mc (B,C,H,W)      shared inputs; the masks are random 0/1 with sample 2 entirely zero
  TT_steps, TT_x_t                                        the reference's q_step_from_x_0 on the taped noise (no objective enters it)
  TT_alpha_sigma (B,2)                                    the scalars of that noising, as the reference evaluated them
  TT_OBJ_pred                                             the reference U-Net's prediction inside p_loss
  TT_v_target                                             get_target for v (for eps it IS the noise, for x_0 it IS x_0: asserted here)
  TT_OBJ_w1, TT_OBJ_w0                                    get_loss_weight with min_snr_loss_weight True / False, (B,)
  TT_OBJ_CRIT_MASK_loss (B,), TT_OBJ_CRIT_MASK_p_loss     the per-sample unweighted loss (base.py:137) and p_loss's return value,
                                                          CRIT in l2 / l1 / huber, MASK in none / m1 / mc
  ..._loss64, ..._p_loss64                                the same two recomputed in float64 from the stored prediction, target and mask
  ref_gap                                                 the largest relative difference between a float32 value and its float64 twin
The per-sample loss is read from p_loss's own frame when it asks for the loss weight, so it is the reference's value, not a replay.
"""
import copy
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")
warnings.filterwarnings("ignore")

from r2dm_amd import synthetic  # noqa: E402

import utils.inference as ref_inference  # noqa: E402  (reference)

RES = (16, 128)
SEED = 0
B, C = 4, 2
ZERO_SAMPLE = 2
CRITERIA = ("l2", "l1", "huber")
CASES = {
    "ct": dict(kw=dict(), objectives=("eps", "v", "x_0"), steps=torch.tensor([0.02, 0.3, 0.7, 0.98])),
    "dt": dict(kw=dict(timestep_type="discrete", num_training_steps=1000, noise_schedule="linear"), objectives=("eps", "v"),
               steps=torch.tensor([0, 10, 500, 999])),
}


def rnd(seed, *shape):
    return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal(shape).astype(np.float32))


def bits(seed, *shape):
    m = torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).integers(0, 2, shape).astype(np.float32))
    m[ZERO_SAMPLE] = 0.0
    return m


def build(loss_type, **kw):
    ckpt = copy.deepcopy(synthetic.synthetic_checkpoint(seed=SEED, resolution=RES, **kw))
    ckpt["cfg"]["diffusion"]["loss_type"] = loss_type
    return ref_inference.setup_model(ckpt, device="cpu", show_info=False)[0]


class Tape:
    """Replaces ddpm.randn: every draw is the given tensor."""

    def __init__(self, ddpm, z):
        self.z = z
        ddpm.randn = self

    def __call__(self, *shape, rng=None, **kw):
        assert tuple(shape) == tuple(self.z.shape)
        return self.z.clone()


class Probe:
    """Records what p_loss holds when it asks for the loss weight: the prediction it got from the model (forward hook) and its own
    local ``loss``, the per-sample unweighted loss of base.py:137."""

    def __init__(self, ddpm):
        self.ddpm, self.weight_fn = ddpm, ddpm.get_loss_weight
        ddpm.get_loss_weight = self.get_loss_weight
        ddpm.model.register_forward_hook(lambda mod, args, out: setattr(self, "pred", out.detach().clone()))

    def get_loss_weight(self, steps):
        self.loss = sys._getframe(1).f_locals["loss"].detach().clone()
        self.weight = self.weight_fn(steps)
        return self.weight


def loss64(pred, target, mask, crit):
    d = pred.double() - target.double()
    if crit == "l2":
        l = d * d
    elif crit == "l1":
        l = d.abs()
    else:
        l = torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5)
    m = torch.ones_like(l) if mask is None else mask.double().expand_as(l)
    own = torch.ones_like(l) if mask is None else mask.double()
    return (l * m).flatten(1).sum(1) / (own.flatten(1).sum(1) + 1e-8)


def rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    nz = b != 0
    assert (a[~nz] == 0).all()
    return float((np.abs(a[nz] - b[nz]) / np.abs(b[nz])).max()) if nz.any() else 0.0


@torch.no_grad()
def main():
    x_0 = rnd(1200, B, C, *RES).clamp(-1, 1)
    noise = rnd(1201, B, C, *RES)
    masks = {"none": None, "m1": bits(1202, B, 1, *RES), "mc": bits(1203, B, C, *RES)}
    out = {"x_0": x_0, "noise": noise, "mask_m1": masks["m1"], "mask_mc": masks["mc"]}
    gap = 0.0
    for tt, case in CASES.items():
        steps = case["steps"]
        out[f"{tt}_steps"] = steps
        for obj in case["objectives"]:
            for crit in CRITERIA:
                d = build(crit, prediction_type=obj, **case["kw"])
                Tape(d, noise)
                probe = Probe(d)
                x_t, z = d.q_step_from_x_0(x_0, steps)
                assert torch.equal(z, noise)
                target = d.get_target(x_0, steps, noise)
                if obj != "v":
                    assert torch.equal(target, noise if obj == "eps" else x_0)
                else:
                    out[f"{tt}_v_target"] = target
                if f"{tt}_x_t" in out:
                    assert np.array_equal(out[f"{tt}_x_t"].numpy(), x_t.numpy())  # (no objective or criterion enters the noising)
                out[f"{tt}_x_t"] = x_t
                if tt == "ct":
                    a, s = d.log_snr(steps).sigmoid().sqrt(), (-d.log_snr(steps)).sigmoid().sqrt()
                else:
                    a, s = d.alpha_bar[steps].sqrt(), (1 - d.alpha_bar[steps]).sqrt()
                out[f"{tt}_alpha_sigma"] = torch.stack([a.reshape(B), s.reshape(B)], dim=-1)
                for on in (True, False):
                    d.min_snr_loss_weight = on
                    out[f"{tt}_{obj}_w{int(on)}"] = probe.weight_fn(steps).reshape(B)
                d.min_snr_loss_weight = True
                w1 = out[f"{tt}_{obj}_w1"]
                snr = d.log_snr(steps).exp().reshape(B) if tt == "ct" else d.snr[steps].reshape(B)
                assert (snr > d.min_snr_gamma).any() and (snr < d.min_snr_gamma).any(), "the min-SNR clamp must be on for one step and off for one"
                for mk, mask in masks.items():
                    p = d.p_loss(x_0, steps, mask)
                    key = f"{tt}_{obj}_{crit}_{mk}"
                    if f"{tt}_{obj}_pred" in out:
                        assert torch.equal(out[f"{tt}_{obj}_pred"], probe.pred)
                    out[f"{tt}_{obj}_pred"] = probe.pred
                    loss = probe.loss.reshape(B)
                    assert torch.equal(probe.weight.reshape(B), w1)
                    l64 = loss64(probe.pred, target, mask, crit)
                    p64 = (l64[None, :] * w1.double()[:, None]).mean()  # base.py:138: (B,1) * (B,1,1,1) -> every loss with every weight
                    out[key + "_loss"], out[key + "_p_loss"], out[key + "_loss64"], out[key + "_p_loss64"] = loss, p, l64, p64
                    gap = max(gap, rel(loss, l64), rel(p, p64))
                    if mask is not None:
                        assert loss[ZERO_SAMPLE].item() == 0.0 and l64[ZERO_SAMPLE].item() == 0.0, "the all-zero-mask sample must give exactly 0"
                    paired = (loss * w1).mean().item()
                    print(f"{key:24s} p_loss {p.item():.7e}  fp64 {p64.item():.7e}  mean(loss_b w_b) {paired:.7e}  per-sample {loss.numpy()}")
                if crit == "huber":
                    ad = (probe.pred - target).abs()
                    lo, hi = (ad < 1).float().mean().item(), (ad >= 1).float().mean().item()
                    print(f"{tt}_{obj}: |d| < 1 for {lo:.3f}, >= 1 for {hi:.3f} of the elements")
                    assert lo >= 0.05 and hi >= 0.05, "huber must be exercised on both sides of |d| = 1"
    out["ref_gap"] = np.float64(gap)
    print(f"ref_gap {gap:.3e}")
    arrays = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, "loss.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(f"loss.npz: {size / 1024:.1f} KiB, {len(arrays)} arrays")
    assert size < 1_000_000


if __name__ == "__main__":
    main()
