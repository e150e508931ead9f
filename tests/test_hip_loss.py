"""-m gpu: the denoising loss -- the fused kernel r2dm_diffusion_loss alone, and ``ddpm(x_0, loss_mask)`` / ``loss_terms`` / ``loss_curve`` /
denoising_loss.py end to end -- against the reference's own run (tests/golden/loss.npz, tests/golden/make_golden_loss.py).

Tolerances (stated, derived from the number formats and the fixture, not from the code under test):
  * kernel vs float64: relative 2e-6 per sample.  The float64 comparator starts from the same float32 prediction and target (the kernel's
    ``v`` target replays the reference's two products and one difference, so its bits are the stored target's).  From there an element is
    d = prediction - target (one rounding), then d*d / |d| / 0.5 d d / |d| - 0.5 (at most two more) and the product with a 0/1 mask
    (exact): at most about five float32 roundings, each 2^-24 relative, of a NON-NEGATIVE term.  Sums of non-negative terms keep the
    relative bound, the accumulation is float64 (2^-53 per add), so a sample's sum is within a few 2^-23 of the float64 value: 2e-6 is
    that with a margin of about four.
  * kernel vs the reference's float32 value: ``ref_gap + 2e-6``, ref_gap being the fixture's recorded largest relative distance between
    a reference float32 loss and its float64 twin (1.7e-7).
  * end to end: the only further difference is the U-Net's parity class max|delta prediction| < DELTA = 2e-5 (tests/test_hip_unet.py);
    the bar per element follows from r = |prediction_ref - target| of the STORED tensors (``element_bound``).
"""
import copy
import json
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, GOLDEN_RES, rnd, synthetic_ckpt

pytestmark = pytest.mark.gpu
DEV = "cuda"
DELTA = 2e-5  # the U-Net's parity class (tests/test_hip_unet.py, tolerance policy at its top)
KERNEL_BAR = 2e-6
CRITERIA = ("l2", "l1", "huber")
MASKS = ("none", "m1", "mc")
CASES = {"ct": (dict(), ("eps", "v", "x_0")),
         "dt": (dict(timestep_type="discrete", num_training_steps=1000, noise_schedule="linear"), ("eps", "v"))}
ZERO_SAMPLE = 2  # the sample whose masks are entirely zero (make_golden_loss.py)


def build(tt, obj, loss_type="l2", **kw):
    import r2dm_amd

    ck = synthetic_ckpt(resolution=GOLDEN_RES, prediction_type=obj, **CASES[tt][0])
    if loss_type != "l2":
        ck = copy.deepcopy(ck)
        ck["cfg"]["diffusion"]["loss_type"] = loss_type
    return r2dm_amd.setup_model(ck, device=DEV, show_info=False, **kw)[0]


@pytest.fixture(scope="module")
def g(golden):
    return golden("loss")


@pytest.fixture(scope="module")
def models():
    """One model per (time type, objective), built through the checkpoint's ``cfg.diffusion.loss_type`` = "huber"; the tests then switch
    ``loss_type``, which the loss reads at call time."""
    cache = {}

    def get(tt, obj):
        if (tt, obj) not in cache:
            cache[tt, obj] = build(tt, obj, loss_type="huber")
            assert cache[tt, obj].loss_type == "huber"
        return cache[tt, obj]

    return get


def mask_of(g, mk):
    return None if mk == "none" else g[f"mask_{mk}"]


def target_of(g, tt, obj):
    return {"eps": g["noise"], "x_0": g["x_0"], "v": g[f"{tt}_v_target"]}[obj]


def criterion64(d, crit):
    if crit == "l2":
        return d * d
    if crit == "l1":
        return d.abs()
    return torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5)


def sums64(pred, target, mask, crit):
    """float64 (num (B,C), den (B,)) from float32 prediction / target: what the kernel is specified to return."""
    l = criterion64(pred.double() - target.double(), crit)
    if mask is None:
        return l.flatten(2).sum(2), torch.full((l.shape[0],), float(l[0].numel()), dtype=torch.float64)
    return (l * mask.double()).flatten(2).sum(2), mask.double().flatten(1).sum(1)


def rel_err(got, want):
    got, want = got.double().cpu().reshape(-1), want.double().cpu().reshape(-1)
    zero = want == 0
    assert (got[zero] == 0).all(), "a zero of the comparator must be an exact zero"
    return ((got[~zero] - want[~zero]).abs() / want[~zero].abs()).max().item() if (~zero).any() else 0.0


def kernel(pred, x_0, noise, mask, coef, obj, crit):
    from r2dm_amd import _lib

    dev = lambda t: None if t is None else t.to(DEV)
    return _lib.diffusion_loss(dev(pred), dev(x_0), dev(noise), dev(mask), dev(coef), obj, crit)


# ---- 1. the kernel alone, on the reference's tensors ------------------------------------------------------------------------------
@pytest.mark.parametrize("tt", ["ct", "dt"])
def test_kernel_on_the_reference_tensors(g, tt):
    gap = g["ref_gap"].item()
    assert 0 < gap < 1e-6
    worst64 = worst32 = 0.0
    for obj in CASES[tt][1]:
        pred = g[f"{tt}_{obj}_pred"]
        for crit in CRITERIA:
            for mk in MASKS:
                mask = mask_of(g, mk)
                num, den = kernel(pred, g["x_0"], g["noise"], mask, g[f"{tt}_alpha_sigma"], obj, crit)
                assert num.dtype == den.dtype == torch.float64 and num.shape == (4, 2) and den.shape == (4,)
                want_den = torch.full((4,), 2.0 * 16 * 128, dtype=torch.float64) if mask is None else mask.double().flatten(1).sum(1)
                assert torch.equal(den.cpu(), want_den), (obj, crit, mk)  # exact
                if mask is not None:
                    assert den[ZERO_SAMPLE].item() == 0 and (num[ZERO_SAMPLE] == 0).all()  # exactly 0
                per_sample = num.sum(1).cpu() / (den.cpu() + 1e-8)
                key = f"{tt}_{obj}_{crit}_{mk}"
                e64, e32 = rel_err(per_sample, g[key + "_loss64"]), rel_err(per_sample, g[key + "_loss"])
                worst64, worst32 = max(worst64, e64), max(worst32, e32)
                assert e64 <= KERNEL_BAR, (key, e64)
                assert e32 <= gap + KERNEL_BAR, (key, e32)
                # per channel too, against the float64 sums of the stored prediction and target
                num64, _ = sums64(pred, target_of(g, tt, obj), mask, crit)
                assert rel_err(num, num64) <= KERNEL_BAR, key
    print(f"{tt}: kernel vs float64 {worst64:.2e}, vs the reference's float32 {worst32:.2e} (ref_gap {gap:.2e})")


# ---- 2. small shapes where the kernel can go wrong --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 2, 3, 5), (1, 1, 1, 1), (2, 3, 7, 33), (2, 2, 64, 1024)],
                         ids=lambda s: "x".join(map(str, s)))
def test_kernel_small_and_odd_shapes(shape):
    """3x5: planes below a quad, tails only; 1x1; 7x33: an odd plane (element by element, planes not 16-byte aligned) with C = 3 and both
    mask widths; 64x1024: 16 blocks per plane, four grid-stride passes each (the grid is capped at 16 x 1024 elements per pass)."""
    B, C = shape[:2]
    pred, x_0, noise = 1.5 * rnd(1300, *shape), rnd(1301, *shape).clamp(-1, 1), rnd(1302, *shape)
    ang = rnd(1303, B).abs()
    coef = torch.stack([ang.cos(), ang.sin()], dim=-1)
    bits = lambda seed, *s: (rnd(seed, *s) > 0).float()
    masks = {"none": None, "m1": bits(1304, B, 1, *shape[2:]), "mc": bits(1305, *shape)}
    for obj in ("eps", "v", "x_0"):
        target = {"eps": noise, "x_0": x_0, "v": coef[:, 0, None, None, None] * noise - coef[:, 1, None, None, None] * x_0}[obj]  # float32, the reference's ops
        for crit in CRITERIA:
            for mk, mask in masks.items():
                num, den = kernel(pred, x_0, noise, mask, coef, obj, crit)
                num64, den64 = sums64(pred, target, mask, crit)
                assert torch.equal(den.cpu(), den64), (obj, crit, mk)
                assert rel_err(num, num64) <= KERNEL_BAR, (obj, crit, mk, rel_err(num, num64))


# ---- 3. determinism and batch independence ----------------------------------------------------------------------------------------
def test_kernel_is_deterministic_and_batch_independent(g):
    for shape, seed in (((4, 2, 16, 128), 1310), ((4, 3, 7, 33), 1311), ((3, 2, 64, 1024), 1312)):
        B = shape[0]
        pred, x_0, noise = (1.5 * rnd(seed, *shape)).to(DEV), rnd(seed + 10, *shape).clamp(-1, 1).to(DEV), rnd(seed + 20, *shape).to(DEV)
        coef = torch.stack([rnd(seed + 30, B).abs().cos(), rnd(seed + 30, B).abs().sin()], dim=-1).to(DEV)
        for mask in (None, (rnd(seed + 40, B, 1, *shape[2:]) > 0).float().to(DEV), (rnd(seed + 50, *shape) > 0).float().to(DEV)):
            num, den = kernel(pred, x_0, noise, mask, coef, "v", "huber")
            again = kernel(pred, x_0, noise, mask, coef, "v", "huber")
            assert torch.equal(num, again[0]) and torch.equal(den, again[1])
            for b in range(B):
                n1, d1 = kernel(pred[b:b + 1], x_0[b:b + 1], noise[b:b + 1], None if mask is None else mask[b:b + 1], coef[b:b + 1], "v", "huber")
                assert torch.equal(n1[0], num[b]) and torch.equal(d1[0], den[b]), (shape, b)


@pytest.mark.parametrize("tt", ["ct", "dt"])
def test_loss_terms_rows_do_not_depend_on_the_batch(g, models, tt):
    d = models(tt, "v")
    d.loss_type = "huber"
    x_0, noise, steps, mask = g["x_0"].to(DEV), g["noise"].to(DEV), g[f"{tt}_steps"].to(DEV), g["mask_mc"].to(DEV)
    full = d.loss_terms(x_0, steps, mask, noise=noise)
    again = d.loss_terms(x_0, steps, mask, noise=noise)
    for key in ("per_channel", "per_sample", "weight", "weighted", "log_snr"):
        assert torch.equal(full[key], again[key]), key
    assert torch.equal(full["loss"], again["loss"])
    for b in range(4):
        one = d.loss_terms(x_0[b:b + 1], steps[b:b + 1], mask[b:b + 1], noise=noise[b:b + 1])
        for key in ("per_channel", "per_sample", "weight", "weighted", "log_snr"):
            assert torch.equal(one[key][0], full[key][b]), (key, b)


# ---- 4. the discrete forward process ----------------------------------------------------------------------------------------------
def test_discrete_q_step_from_x_0_is_the_references_bits(g, models):
    """r2dm_q_step replays the reference's operation order (two float32 products, one sum, no contraction) on correctly rounded float32
    square roots of alpha_bar and 1 - alpha_bar: BIT-IDENTICAL to the reference's x_t, which is the stronger of the two statements
    (within 1 ulp, a fortiori).  (The roots are taken in float64 on the host: torch's float32 sqrt on a CPU was found one ulp off the
    correctly rounded root at two of these four steps on one host.)"""
    d = models("dt", "eps")
    noise = g["noise"].to(DEV)
    d.randn = lambda *shape, rng=None, **kw: noise
    try:
        x_t, z = d.q_step_from_x_0(g["x_0"].to(DEV), g["dt_steps"].to(DEV))
    finally:
        del d.randn
    assert z is noise and torch.equal(x_t.cpu(), g["dt_x_t"])
    # a drawn call: the noise comes from the generator given
    gen = torch.Generator(device=DEV).manual_seed(11)
    x_t, z = d.q_step_from_x_0(g["x_0"].to(DEV), g["dt_steps"].to(DEV), rng=gen)
    want = torch.randn(*z.shape, generator=torch.Generator(device=DEV).manual_seed(11), device=DEV)
    assert torch.equal(z, want)


# ---- 5. end to end against the reference ------------------------------------------------------------------------------------------
def element_bound(r, crit):
    """How far one element's loss can move when the prediction moves by at most DELTA, r = |prediction_ref - target|."""
    if crit == "l2":
        return 2 * r * DELTA + DELTA ** 2       # |(r + e)^2 - r^2|
    if crit == "l1":
        return torch.full_like(r, DELTA)          # | |d + e| - |d| | <= |e|
    return torch.clamp(r, min=1.0) * DELTA + DELTA ** 2 / 2  # huber: slope min(|d|, 1) <= max(r, 1) anywhere within DELTA of d


@pytest.mark.parametrize("tt", ["ct", "dt"])
def test_loss_terms_against_the_reference(g, models, tt):
    gap = g["ref_gap"].item()
    x_0, noise, steps = g["x_0"].to(DEV), g["noise"].to(DEV), g[f"{tt}_steps"].to(DEV)
    worst = {"per_sample": 0.0, "per_sample_over_bar": 0.0, "loss": 0.0, "loss_over_bar": 0.0}
    for obj in CASES[tt][1]:
        d = models(tt, obj)
        r = (g[f"{tt}_{obj}_pred"].double() - target_of(g, tt, obj).double()).abs()
        w = g[f"{tt}_{obj}_w1"].double()
        for crit in CRITERIA:
            d.loss_type = crit
            for mk in MASKS:
                mask = mask_of(g, mk)
                terms = d.loss_terms(x_0, steps, None if mask is None else mask.to(DEV), noise=noise)
                key = f"{tt}_{obj}_{crit}_{mk}"
                want, want_p = g[key + "_loss"].double(), g[key + "_p_loss"].double()
                m = torch.ones_like(r) if mask is None else mask.double().expand_as(r)
                own = float(r[0].numel()) if mask is None else mask.double().flatten(1).sum(1)
                bar = (element_bound(r, crit) * m).flatten(1).sum(1) / (own + 1e-8) + (gap + KERNEL_BAR) * want.abs()
                diff = (terms["per_sample"].double().cpu() - want).abs()
                # the reference's p_loss pairs every loss with every weight (base.py:138: (B,1) * (B,1,1,1)), so its bar is the same mean of the bars
                bar_p = (w[:, None] * bar[None, :]).mean() + (gap + KERNEL_BAR) * want_p.abs()
                diff_p = (terms["loss"].double().cpu() - want_p).abs()
                print(f"{key:22s} per-sample |diff| {diff.max().item():.2e} (bar {bar.max().item():.2e})  loss |diff| {diff_p.item():.2e} (bar {bar_p.item():.2e})")
                worst["per_sample"], worst["loss"] = max(worst["per_sample"], diff.max().item()), max(worst["loss"], diff_p.item())
                live = bar > 0
                worst["per_sample_over_bar"] = max(worst["per_sample_over_bar"], (diff[live] / bar[live]).max().item())
                worst["loss_over_bar"] = max(worst["loss_over_bar"], (diff_p / bar_p).item())
                assert (diff <= bar).all(), (key, diff.tolist(), bar.tolist())
                assert diff_p <= bar_p, (key, diff_p.item(), bar_p.item())
                assert terms["loss"].dim() == 0 and terms["loss"].dtype == torch.float32 and terms["loss"].is_cuda
                if tt == "dt":  # a table lookup, a clamp and one division: the same bits anywhere
                    assert torch.equal(terms["weight"].cpu(), g[f"{tt}_{obj}_w1"])
                else:  # through the host's libm (tan, log, exp of a log-SNR within +-16, whose ulp is 9.5e-7): ten ulps of the log-SNR
                    assert torch.allclose(terms["weight"].cpu(), g[f"{tt}_{obj}_w1"], rtol=1e-5, atol=0)
                if mask is not None:
                    assert terms["per_sample"][ZERO_SAMPLE].item() == 0.0 and (terms["per_channel"][ZERO_SAMPLE] == 0).all()
                assert torch.allclose(terms["per_channel"].sum(1), terms["per_sample"], rtol=1e-6, atol=0)
                assert torch.equal(terms["weighted"], terms["per_sample"] * terms["weight"])
        host_steps = g[f"{tt}_steps"]
        if tt == "ct":  # the schedule on the host, row by row
            want_snr = torch.cat([d.log_snr(host_steps[i:i + 1]).reshape(1) for i in range(4)])
        else:
            want_snr = torch.cat([d.snr.cpu()[host_steps[i:i + 1], 0, 0, 0].log() for i in range(4)])
        assert torch.equal(terms["log_snr"].cpu(), want_snr) and torch.isfinite(terms["log_snr"]).all()
    print(f"{tt}: largest differences from the reference {json.dumps({k: float(f'{v:.3e}') for k, v in worst.items()})}")


# ---- 6. draw order, generators, no gradient ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("tt", ["ct", "dt"])
def test_forward_draws_the_steps_first_then_the_noise(g, models, tt):
    import r2dm_amd

    d = models(tt, "eps")
    d.loss_type = "l2"
    x_0, mask = g["x_0"].to(DEV), g["mask_m1"].to(DEV)
    torch.manual_seed(77)
    loss = d(x_0, mask)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and not loss.requires_grad and torch.isfinite(loss)
    torch.manual_seed(77)
    steps = d.sample_timesteps(4, x_0.device)
    noise = torch.randn_like(x_0)
    by_hand = d.loss_terms(x_0, steps, mask, noise=noise)["loss"]
    assert torch.equal(loss, by_hand)
    torch.manual_seed(77)
    steps_again = d.sample_timesteps(4, x_0.device)
    assert torch.equal(steps_again, steps) and torch.equal(d.p_loss(x_0, steps_again, mask), loss)  # p_loss draws the noise itself
    torch.manual_seed(78)
    assert not torch.equal(d(x_0, mask), loss)
    # one generator per sample: a sample's loss does not depend on how the batch is cut
    steps = g[f"{tt}_steps"].to(DEV)
    seeds = [3, 4, 5, 6]
    whole = d.loss_terms(x_0, steps, mask, rng=r2dm_amd.setup_rng(seeds, DEV))["per_sample"]
    parts = torch.cat([d.loss_terms(x_0[a:b], steps[a:b], mask[a:b], rng=r2dm_amd.setup_rng(seeds[a:b], DEV))["per_sample"]
                       for a, b in ((0, 1), (1, 3), (3, 4))])
    assert torch.equal(whole, parts)
    assert not d.p_loss(x_0, steps, mask, rng=r2dm_amd.setup_rng(seeds, DEV)).requires_grad


# ---- 7. the curve and the script --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tt", ["ct", "dt"])
def test_loss_curve_is_its_single_rows_regrouped(g, models, tt):
    import r2dm_amd
    from r2dm_amd.loss import level_grid, loss_curve

    d = models(tt, "v")
    d.loss_type = "l2"
    x_0, mask = g["x_0"][:3].to(DEV), g["mask_mc"][[0, 1, 3]].to(DEV)
    seeds = [21, 22, 23]
    curve = loss_curve(d, x_0, loss_mask=mask, levels=4, rng=r2dm_amd.setup_rng(seeds, DEV), batch_size=5)  # calls that span levels
    grid = level_grid(d, 4)
    gens = r2dm_amd.setup_rng(seeds, DEV)
    assert curve["num_images"] == 3 and len(curve["levels"]) == 4
    weighted = []
    for k, level in enumerate(curve["levels"]):
        rows = [d.loss_terms(x_0[i:i + 1], grid[k:k + 1].to(DEV), mask[i:i + 1], rng=[gens[i]]) for i in range(3)]
        mean = lambda key: torch.cat([r[key] for r in rows]).double().cpu().mean(0)
        assert level["t"] == grid[k].item()
        # (float64 means of three float32 rows: equal up to the order of two float64 additions)
        assert level["loss"] == pytest.approx(mean("per_sample").item(), rel=1e-14)
        assert level["weighted_loss"] == pytest.approx(mean("weighted").item(), rel=1e-14)
        assert level["log_snr"] == pytest.approx(mean("log_snr").item(), rel=1e-14)
        assert level["per_channel"] == pytest.approx(mean("per_channel").tolist(), rel=1e-14)
        weighted.append(mean("weighted").item())
    assert curve["mean_weighted_loss"] == pytest.approx(float(np.mean(weighted)), rel=1e-14)
    other = loss_curve(d, x_0, loss_mask=mask, levels=4, rng=r2dm_amd.setup_rng(seeds, DEV), batch_size=2)
    assert other == curve  # whatever the chunking


@pytest.mark.parametrize("mask_loss", [False, True], ids=["no_mask", "mask_loss"])
def test_denoising_loss_script(tmp_path, mask_loss):
    import torch.nn.functional as F

    import r2dm_amd
    from r2dm_amd import projection
    from r2dm_amd.loss import loss_curve

    sys.path.insert(0, GOLDEN)
    import make_golden_projection as GP  # (the projection fixture's integer-only cloud generator)

    import denoising_loss

    ckpt = tmp_path / "synthetic.pth"
    torch.save(synthetic_ckpt(resolution=GOLDEN_RES), ckpt)
    pts = GP.make_cloud("free_64x1024")
    scans = tmp_path / "scans" / "seq_0" / "velodyne_points" / "data"
    scans.mkdir(parents=True)
    for k in range(2):
        np.ascontiguousarray(pts[20000 * k:20000 * k + 15000 + 500 * k]).tofile(scans / f"{k:010d}.bin")
    out = tmp_path / "loss.json"
    argv = ["--ckpt", str(ckpt), "--real_scans", str(tmp_path / "scans"), "--levels", "2", "--batch_size", "3", "--seed", "9", "--out", str(out)]
    doc = denoising_loss.main(argv + (["--mask_loss"] if mask_loss else []))
    assert json.loads(out.read_text()) == json.loads(json.dumps(doc))

    ddpm, lidar, cfg = r2dm_amd.setup_model(ckpt, device=DEV, show_info=False, max_batch=3)
    unfolding, width = projection.parse_projection(cfg.data.projection)
    points, offsets = projection.load_scans(sorted((tmp_path / "scans").rglob("*.bin")))
    xyzrdm = projection.project_scans(points, offsets, H=64, W=width, scan_unfolding=unfolding, min_depth=lidar.min_depth, max_depth=lidar.max_depth,
                                      apply_mask=True, device=DEV)
    x_0 = projection.known_from_scan(xyzrdm, lidar, cfg.data.resolution)
    measured = F.interpolate(xyzrdm[:, [5]], size=GOLDEN_RES, mode="nearest-exact")
    assert 0 < measured.mean().item() < 1 and ((x_0 == -1).all(1, keepdim=True) | (measured == 1)).all()  # -1 wherever nothing was measured
    want = loss_curve(ddpm, x_0, loss_mask=measured if mask_loss else None, levels=2, rng=r2dm_amd.setup_rng([9, 10], DEV), batch_size=3)
    assert doc["num_scans"] == 2 and doc["seed"] == 9 and doc["levels"] == 2 and doc["mask_loss"] is mask_loss and doc["weights"] == "ema"
    assert doc["mean_weighted_loss"] == want["mean_weighted_loss"] and np.isfinite(doc["mean_weighted_loss"])
    assert [lv["t"] for lv in doc["curve"]] == [0.25, 0.75]
    for got, lv in zip(doc["curve"], want["levels"]):
        assert got["loss"] == lv["loss"] and got["weighted_loss"] == lv["weighted_loss"] and got["log_snr"] == lv["log_snr"]
        assert got["per_channel"] == {"depth": lv["per_channel"][0], "reflectance": lv["per_channel"][1]}
    assert doc["config"]["diffusion"]["prediction_type"] == "eps" and list(doc["config"]["data"]["resolution"]) == list(GOLDEN_RES)
