"""-m gpu: the latent-space operators (r2dm_amd/csrc/latent.hip) and the sampler methods on top of them -- ``r2dm_ddim_transfer`` and
``r2dm_slerp`` against their contracts (tests/latent_oracle.py), ``sample_from`` against ``sample``, ``invert`` / ``sample_from`` against the
oracle in float64, ``latent.interpolate`` and the ``interpolate.py`` script."""
import ctypes
import functools
import json
import math
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN_RES, ROOT, rnd, synthetic_ckpt

import latent_oracle as LO

import r2dm_amd
from oracle import r2dm_oracle as O
from r2dm_amd import _lib, latent
from r2dm_amd._lib import R2DMError

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, S = 3, 4
SHAPE = (B, 2, *GOLDEN_RES)
OBJECTIVES = ["eps", "v", "x_0"]


@functools.lru_cache(maxsize=None)
def model(objective="eps", max_batch=8):
    return r2dm_amd.setup_model(synthetic_ckpt(resolution=GOLDEN_RES, prediction_type=objective), device=DEV, show_info=False, max_batch=max_batch)


def stats(got, want):
    e = (got.double() - want.double()).abs().flatten()
    return e.pow(2).mean().sqrt().item(), torch.quantile(e, 0.99).item(), e.max().item()


# ---- 1. r2dm_ddim_transfer ------------------------------------------------------------------------
# rows at t = 0 (alpha ~ 1, sigma ~ 5.5e-4), at t = 1 and in between; forward (towards noise) and backward
T_ROWS = [0.0, 1.0, 0.4]
U_ROWS = {"forward": [0.3, 1.0, 0.9], "backward": [0.0, 0.6, 0.1]}
# 4096: one pass of sixteen blocks.  1024 blocks x 256 threads x 4 elements is one pass of the capped grid: 4 KiB more is a second pass
PER_SAMPLE = [4096, 1024 * 256 * 4 + 4096]


@pytest.mark.parametrize("per_sample", PER_SAMPLE)
@pytest.mark.parametrize("direction", ["forward", "backward"])
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_ddim_transfer_bit_exact_vs_torch_ops(objective, direction, per_sample):
    ddpm = model()[0]
    rows_t, rows_u = (ddpm._alpha_sigma_rows(torch.tensor(v)) for v in (T_ROWS, U_ROWS[direction]))
    assert rows_t[0, 1] < 6e-4 and rows_t[0, 0] > 0.999 and rows_t[1, 0] < 6e-4
    coef = torch.cat([rows_t, rows_u], dim=-1).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(per_sample % 1000 + OBJECTIVES.index(objective))
    x, pr = (torch.randn(B, per_sample, generator=g, device=DEV) for _ in range(2))
    got = latent.ddim_transfer(x, pr, coef, objective)
    a_t, s_t, a_u, s_u = (coef[:, k][:, None] for k in range(4))
    want = LO.ddim_transfer(x, pr, a_t, s_t, a_u, s_u, objective)  # (the contract's expression in torch ops on the device: one rounding per op)
    assert got.dtype == torch.float32 and torch.isfinite(got).all()
    assert torch.equal(got, want), (got - want).abs().max().item()


def test_ddim_transfer_refusals():
    coef = torch.ones(2, 4, device=DEV)
    buf = torch.zeros(2 * 4096 + 4, device=DEV)
    ok, off = buf[:2 * 4096].view(2, 4096), buf[1:1 + 2 * 4096].view(2, 4096)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    latent.ddim_transfer(ok, ok, coef, "eps")
    for x, pr in ((off, ok), (ok, off)):
        with pytest.raises(R2DMError, match="16-byte aligned"):
            latent.ddim_transfer(x, pr, coef, "eps")
    odd = torch.zeros(2, 4098, device=DEV)
    with pytest.raises(R2DMError, match="multiple of 4"):
        latent.ddim_transfer(odd, odd, coef, "v")
    with pytest.raises(ValueError):
        latent.ddim_transfer(ok, ok, coef, "noise")
    with pytest.raises(ValueError):
        latent.ddim_transfer(ok, ok, coef[:, :2], "eps")
    assert _lib.lib().r2dm_ddim_transfer(ok.data_ptr(), ok.data_ptr(), coef.data_ptr(), ok.data_ptr(), 2, 4096, 3, None) != 0


# ---- 2. r2dm_slerp ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def slerp_case(K):
    """(a, b on the GPU, weights, the oracle's sums): computed once, left unchanged"""
    a, b = LO.slerp_inputs(SHAPE)
    weights = [0.35] if K == 1 else [0.0, 0.25, 0.5, 1.0, 1.25]
    return a.to(DEV), b.to(DEV), weights, LO.slerp_sums(a.numpy(), b.numpy())


@pytest.mark.parametrize("K", [1, 5])
def test_slerp_coefficients_within_the_summation_bound_and_output_bit_exact(K):
    """The bound on |c - c_oracle|, u = 2^-53, N = per_sample.  The kernel adds N exactly represented products p_i in float64 in some fixed
    order: its sum differs from the exact one (the oracle's fsum) by at most N u sum|p_i| (the standard recursive-summation bound, which
    covers every order).  With A = <a,a>, B = <b,b>, D = <a,b>, T = sum|a_i b_i|:
      cos = D / sqrt(A B):  d_cos <= N u T / sqrt(A B) + |cos| (N u / 2 + N u / 2) + 4 u   (one product, one root, one quotient, the clamp)
      omega = acos(cos):    d_om  <= d_cos / sin(omega) + 4 u pi                          (two libms, each within 2 ulp of a value <= pi)
      c = sin(f omega) / sin(omega), f = 1 - w or w:  |dc/d omega| = |f cos(f omega) sin(omega) - sin(f omega) cos(omega)| / sin^2(omega)
                                                      <= (|f| + |c|) / sin(omega)
      evaluation of c itself (the product f omega, two sines of two libms within 2 ulp each, one quotient):
                            <= 8 u (1 + |f| omega + |c|) / sin(omega)
    so |c - c_oracle| <= (|f| + |c|) d_om / sin(omega) + 8 u (1 + |f| omega + |c|) / sin(omega).  With |cos| <= 0.9 (checked on the CPU for
    these inputs, and again here) sin(omega) >= 0.43 and the bound is a few 1e-12 at N = 4096."""
    a, b, weights, sums = slerp_case(K)
    out, coef64 = latent.slerp(a, b, weights, return_coefficients=True)
    assert out.shape == (K, *SHAPE) and out.dtype == torch.float32 and coef64.shape == (K, B, 2) and coef64.dtype == torch.float64
    want, cos = LO.slerp_coefficients(sums, weights)
    assert np.all(np.abs(cos) <= 0.9)
    u, N = 2.0 ** -53, a[0].numel()
    D, A, Bb, T = sums.T
    d_cos = N * u * T / np.sqrt(A * Bb) + np.abs(cos) * N * u + 4 * u
    omega = np.arccos(cos)
    so = np.sin(omega)
    d_om = d_cos / so + 4 * u * math.pi
    got = coef64.cpu().numpy()
    worst = 0.0
    for k, w in enumerate(weights):
        for f, col in ((1.0 - w, 0), (w, 1)):
            c = want[k, :, col]
            bound = (abs(f) + np.abs(c)) * d_om / so + 8 * u * (1 + abs(f) * omega + np.abs(c)) / so
            err = np.abs(got[k, :, col] - c)
            worst = max(worst, (err / bound).max())
            assert np.all(err <= bound), (k, col, err, bound)
    print(f"slerp K={K}: worst |c - c_oracle| / bound = {worst:.3g}; bound ~ {bound.max():.2e}")
    # the output: the returned coefficients rounded to float32, two products and one sum per element
    c32 = coef64.float()[..., None, None, None]
    assert torch.equal(out, c32[:, :, 0] * a[None] + c32[:, :, 1] * b[None])
    # ... and the oracle's output, whose coefficients may round to a neighbouring float32: a few ulp of the operands
    ref = torch.from_numpy(LO.slerp(a.cpu().numpy(), b.cpu().numpy(), weights)[0])
    assert (out.cpu() - ref).abs().max().item() <= 2.0 ** -22 * max(a.abs().max().item(), b.abs().max().item()) * np.abs(want).max()


def test_slerp_is_batch_independent_and_reproducible():
    a, b, weights, _ = slerp_case(5)
    out, coef = latent.slerp(a, b, weights, return_coefficients=True)
    out2, coef2 = latent.slerp(a, b, weights, return_coefficients=True)
    assert torch.equal(out, out2) and torch.equal(coef, coef2)
    alone, coef1 = latent.slerp(a[1:2], b[1:2], weights, return_coefficients=True)
    assert torch.equal(alone[:, 0], out[:, 1]) and torch.equal(coef1[:, 0], coef[:, 1])
    # more weights than one launch takes (64): chunks, the same frames
    many = torch.linspace(-0.5, 1.5, 70).tolist()
    out70, coef70 = latent.slerp(a, b, many, return_coefficients=True)
    tail, coef_tail = latent.slerp(a, b, many[64:], return_coefficients=True)
    assert torch.equal(out70[64:], tail) and torch.equal(coef70[64:], coef_tail)
    # a sample of more than 16 x 1024 elements: every block of launch 1 makes a second grid-stride pass
    big_a, big_b = rnd(60, 2, 5 * 16 * 1024 + 8).to(DEV), rnd(61, 2, 5 * 16 * 1024 + 8).to(DEV)
    got = latent.slerp(big_a, big_b, [0.5], return_coefficients=True)[1].cpu().numpy()
    want, _ = LO.slerp_coefficients(LO.slerp_sums(big_a.cpu().numpy(), big_b.cpu().numpy()), [0.5])
    assert np.abs(got - want).max() < 1e-10, np.abs(got - want).max()  # (rough: the exact bound is tested above)


def test_slerp_lerp_fallback_and_refusals():
    a, b, _, _ = slerp_case(5)
    w = [0.25, 1.5]
    lerp = torch.tensor([[0.75, 0.25], [-0.5, 1.5]], dtype=torch.float64, device=DEV)[:, None].expand(2, B, 2)
    zero = torch.zeros_like(a)
    for x, y in ((a, a), (zero, b), (a, zero), (a, -a)):
        out, coef = latent.slerp(x, y, w, return_coefficients=True)
        assert torch.equal(coef, lerp)
        c32 = coef.float()[..., None, None, None]
        assert torch.equal(out, c32[:, :, 0] * x[None] + c32[:, :, 1] * y[None])
    # one sample of the batch falls back, the others do not
    mixed = torch.cat([a[:1], b[1:]])
    coef = latent.slerp(a, mixed, w, return_coefficients=True)[1]
    assert torch.equal(coef[:, 0], lerp[:, 0]) and not torch.equal(coef[:, 1], lerp[:, 1])
    for bad in ([math.nan], [0.5, math.inf], []):
        with pytest.raises(ValueError):
            latent.slerp(a, b, bad)
    with pytest.raises(ValueError):
        latent.slerp(a, b[:2], [0.5])
    with pytest.raises(R2DMError, match="multiple of 4"):
        latent.slerp(torch.zeros(2, 4098, device=DEV), torch.zeros(2, 4098, device=DEV), [0.5])
    # the C entry itself: K < 1, K > 64, a non-finite weight, a misaligned pointer
    L = _lib.lib()
    n = 4096
    buf = torch.zeros(2 * n + 4, device=DEV)
    ok, off = buf[:2 * n], buf[1:1 + 2 * n]
    out, coef = torch.empty(2 * n, device=DEV), torch.empty(4, dtype=torch.float64, device=DEV)
    scratch = torch.empty(L.r2dm_slerp_scratch_bytes(2, n) // 8, dtype=torch.float64, device=DEV)
    assert scratch.numel() == 2 * 4 * 3 and L.r2dm_slerp_scratch_bytes(2, 4098) == 0 and L.r2dm_slerp_scratch_bytes(0, n) == 0
    call = lambda x, y, ws, K: L.r2dm_slerp(x.data_ptr(), y.data_ptr(), (ctypes.c_float * len(ws))(*ws), K, out.data_ptr(), coef.data_ptr(), 2, n,
                                            scratch.data_ptr(), _lib.stream_ptr(torch.device(DEV, 0)))
    assert call(ok, ok, [0.5], 1) == 0
    assert call(ok, ok, [0.5], 0) != 0 and call(ok, ok, [0.5] * 65, 65) != 0
    assert call(ok, ok, [math.nan], 1) != 0 and b"not finite" in L.r2dm_last_error()
    assert call(off, ok, [0.5], 1) != 0 and call(ok, off, [0.5], 1) != 0 and b"aligned" in L.r2dm_last_error()
    torch.cuda.synchronize()


# ---- 3. sample_from is the existing sampler -----------------------------------------------------------
@pytest.mark.parametrize("mode,return_all", [("ddpm", False), ("ddim", False), ("ddpm", True)])
def test_sample_from_a_fresh_draw_is_sample(mode, return_all):
    ddpm = model()[0]
    seeds = list(range(50, 50 + B))
    want = ddpm.sample(B, S, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV), mode=mode, return_all=return_all)
    g = r2dm_amd.setup_rng(seeds, DEV)
    x_T = ddpm.randn(B, *ddpm.sampling_shape, rng=g, device=DEV)
    got = ddpm.sample_from(x_T, S, progress=False, rng=g, mode=mode, return_all=return_all)
    assert got.shape == ((S + 1, *SHAPE) if return_all else SHAPE)
    assert torch.equal(got, want)
    assert ddpm._table_key(S, B, mode, 0.0, x_T.device) in ddpm.__dict__["_tables"]  # (one table serves both)


# ---- 4. invert / sample_from against the oracle in float64 -------------------------------------------------
@functools.lru_cache(maxsize=None)
def nets(objective):
    """(the oracle's U-Net in float32, in float64) with the synthetic checkpoint's weights on the device"""
    sd = O.strip_prefix(synthetic_ckpt(resolution=GOLDEN_RES, prediction_type=objective)["ema_weights"])
    sd32, sd64 = ({k: v.to(DEV, dt) for k, v in sd.items()} for dt in (torch.float32, torch.float64))
    cfg = O.UNetConfig(resolution=GOLDEN_RES)
    return (lambda x, c: O.unet_forward(sd32, cfg, x, c)), (lambda x, c: O.unet_forward(sd64, cfg, x, c))


def relative_bar(name, got, ref32, truth):
    """The project's relative bar (tests/test_hip_configs.py::test_ddim_32_step_final_sample_parity_full_size): the HIP result's distance to
    exact arithmetic (the oracle in float64) within 2x of the distance of the oracle's own float32 run in rms and at the 99th percentile,
    within 4x at the worst element."""
    (rms_h, q99_h, max_h), (rms_r, q99_r, max_r) = stats(got, truth), stats(ref32, truth)
    print(f"{name}: hip vs fp64 rms {rms_h:.3e} q99 {q99_h:.3e} max {max_h:.3e} | oracle fp32 vs fp64 rms {rms_r:.3e} q99 {q99_r:.3e} max {max_r:.3e}")
    assert torch.isfinite(got).all()
    assert rms_h <= 2 * rms_r and q99_h <= 2 * q99_r and max_h <= 4 * max_r, (rms_h, q99_h, max_h, rms_r, q99_r, max_r)


@functools.lru_cache(maxsize=None)
def scan_like():
    """(B,2,H,W) in [-1, 1] on the device"""
    return torch.tanh(rnd(70, *SHAPE)).to(DEV)


@pytest.mark.parametrize("t_end", [1.0, 0.5])
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_invert_vs_fp64_oracle(objective, t_end):
    """Measured on the MI355X: see DESIGN.md section 4, 'Latent space'."""
    ddpm = model(objective)[0]
    net32, net64 = nets(objective)
    x_0 = scan_like()
    got = ddpm.invert(x_0, S, t_end=t_end, progress=False, return_all=True)
    assert got.shape == (S + 1, *SHAPE) and torch.equal(got[0], x_0)
    assert torch.equal(got[-1], ddpm.invert(x_0, S, t_end=t_end, progress=False))
    truth = LO.invert(net64, x_0.double(), S, t_end, objective)
    ref32 = LO.invert(net32, x_0, S, t_end, objective)
    relative_bar(f"invert {objective} t_end={t_end}", got[-1], ref32, truth)


@pytest.mark.parametrize("objective,mode", [("eps", "ddpm"), ("v", "ddpm"), ("x_0", "ddpm"), ("eps", "ddim")])
def test_sample_from_half_way_unclipped_vs_fp64_oracle(objective, mode):
    """``sample_from(t_start=0.5, clip=False)`` on one noise tape.  Measured on the MI355X: see DESIGN.md section 4, 'Latent space'."""
    ddpm = model(objective)[0]
    net32, net64 = nets(objective)
    x_t = scan_like()
    seeds = list(range(80, 80 + B))
    got = ddpm.sample_from(x_t, S, t_start=0.5, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV), mode=mode, clip=False)
    g = r2dm_amd.setup_rng(seeds, DEV)
    tape = [O.draw_noise(SHAPE, g, DEV, torch.float32) for _ in range(S)]
    truth = LO.sample_from(net64, x_t.double(), S, 0.5, tape, mode, 0.0, objective, clip=None)
    ref32 = LO.sample_from(net32, x_t, S, 0.5, tape, mode, 0.0, objective, clip=None)
    relative_bar(f"sample_from {objective} {mode} t_start=0.5", got, ref32, truth)
    # clip=None keeps the model's setting (the clamp at 1): another result, the clamped oracle's
    clipped = ddpm.sample_from(x_t, S, t_start=0.5, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV), mode=mode)
    truth_clipped = LO.sample_from(net64, x_t.double(), S, 0.5, tape, mode, 0.0, objective, clip=1.0)
    assert ddpm.clip_sample and stats(clipped, truth_clipped)[0] < 1e-3
    if stats(truth_clipped, truth)[2] > 1e-2:  # (the clamp acts on these inputs: then the two calls differ)
        assert not torch.equal(clipped, got)


# ---- 5. invert with the analytic denoiser -------------------------------------------------------------------
class AnalyticDenoiser(torch.nn.Module):
    """eps* of x_0 ~ N(0, s^2 I) as a denoiser: torch ops on the device"""
    resolution, in_channels = GOLDEN_RES, 2

    def forward(self, x, cond):
        return LO.analytic_eps(x, cond)


def test_invert_with_the_analytic_denoiser_is_first_order_and_the_oracles_loop():
    ddpm = r2dm_amd.ContinuousTimeGaussianDiffusion(AnalyticDenoiser(), prediction_type="eps", noise_schedule="cosine").to(DEV)
    x_0 = (LO.PRIOR_STD * rnd(7, *SHAPE)).to(DEV)
    want = LO.analytic_target(x_0)
    err = {}
    for n in (16, 64):
        got = ddpm.invert(x_0, n, progress=False)
        err[n] = stats(got, want)[0]
        loop = stats(got, LO.invert(LO.analytic_eps, x_0, n))[0]
        print(f"analytic denoiser, N = {n}: rms to the closed form {err[n]:.4f}, to the oracle's fp32 loop {loop:.2e}")
        assert loop <= 1e-5, loop
    assert err[64] <= err[16] / 3, err


def test_invert_with_the_schedule_scalars_on_the_device():
    """``schedule_on="device"``: the inversion's table holds the oracle's device-evaluated scalars bit for bit, and with a denoiser that is
    itself torch ops the whole loop is then the oracle's float32 loop on the device, bit for bit (the transfer kernel is its torch
    expression exactly)."""
    ddpm = r2dm_amd.ContinuousTimeGaussianDiffusion(AnalyticDenoiser(), prediction_type="eps", noise_schedule="cosine").to(DEV)
    ddpm.set_schedule_on("device")
    steps = torch.linspace(0.0, 0.5, S + 1, device=DEV)
    cond, coef = ddpm._transfer_table(steps, B, steps.device)
    lt = O.log_snr_cosine(steps)
    a, s = O.alpha_sigma(lt)
    assert cond.shape == (S, B) and coef.shape == (S, B, 4)
    assert torch.equal(cond[:, 1], lt[:-1]) and torch.equal(coef[:, 1], torch.stack([a[:-1], s[:-1], a[1:], s[1:]], dim=-1))
    x_0 = (LO.PRIOR_STD * rnd(7, *SHAPE)).to(DEV)
    got = ddpm.invert(x_0, S, t_end=0.5, progress=False, return_all=True)
    assert torch.equal(got, LO.invert(LO.analytic_eps, x_0, S, 0.5, return_all=True))


# ---- 6. latent.interpolate -----------------------------------------------------------------------------------
def test_interpolate_shapes_determinism_and_chunking():
    ddpm8, ddpm2 = model("eps", 8)[0], model("eps", 2)[0]
    x_a, x_b = scan_like(), torch.tanh(rnd(71, *SHAPE)).to(DEV)
    F = 3
    frames, latents = latent.interpolate(ddpm8, x_a, x_b, F, S, return_latents=True)
    assert frames.shape == (F, *SHAPE) and latents.shape == (F, *SHAPE) and torch.isfinite(frames).all()
    assert torch.equal(frames, latent.interpolate(ddpm8, x_a, x_b, F, S))
    # the end frames are the reconstructions of the inputs
    assert torch.equal(frames[0], latent.reconstruct(ddpm8, x_a, S)) and torch.equal(latents[0], ddpm8.invert(x_a, S, progress=False))
    # 6 inversions and 9 decodings: chunks of (6), (8, 1) here and of 2 there
    assert torch.equal(frames, latent.interpolate(ddpm2, x_a, x_b, F, S))
    half = latent.interpolate(ddpm8, x_a, x_b, F, S, t_end=0.5)
    assert half.shape == frames.shape and not torch.equal(half, frames)


# ---- 7. interpolate.py ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ckpt_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("ckpt") / "synthetic.pth"
    torch.save(synthetic_ckpt(resolution=GOLDEN_RES), p)
    return p


def _scan(seed, path):
    g = np.random.Generator(np.random.PCG64(seed))
    k = g.integers(0, 2 ** 24, size=(4, 20_000)) / 2.0 ** 24
    phi, theta, depth = np.deg2rad(-24.0 + 26.0 * k[0]), (2.0 * k[1] - 1.0) * np.pi, 2.0 + 60.0 * k[2]
    np.stack([depth * np.cos(phi) * np.cos(theta), depth * np.cos(phi) * np.sin(theta), depth * np.sin(phi), k[3]], 1).astype(np.float32).tofile(path)
    return path


def _run(cmd, cwd):
    r = subprocess.run([sys.executable] + [str(c) for c in cmd], cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def _png_size(path):
    head = open(path, "rb").read(24)
    assert head[:8] == b"\x89PNG\r\n\x1a\n"
    return struct.unpack(">II", head[16:24])


def test_interpolate_script(ckpt_file, tmp_path):
    H, W = GOLDEN_RES
    F = 3
    size = ((W + 2) * F + 2, 2 * H + W + 4)  # a column per frame (image over bird's-eye view), 2 pixels of padding around every cell
    a, b = _scan(9, tmp_path / "a.bin"), _scan(10, tmp_path / "b.bin")
    out = _run([f"{ROOT}/interpolate.py", "--ckpt", ckpt_file, "--scan_a", a, "--scan_b", b, "--frames", F, "--steps", 2, "--out_dir", tmp_path / "scans",
                "--points_dir", tmp_path / "points"], tmp_path)
    row = json.loads([line for line in out.splitlines() if line.startswith("{")][-1])
    assert set(row) >= {"frames", "steps", "t_end", "omega", "scan_a", "scan_b"} and len(row["omega"]) == 1 and 0 < row["omega"][0] < math.pi
    for end in ("scan_a", "scan_b"):
        assert set(row[end]) == {"mae_depth", "rmse_depth", "mae_reflectance", "rmse_reflectance"}
        assert all(len(v) == 1 and math.isfinite(v[0]) and v[0] >= 0 for v in row[end].values()), row[end]
    assert _png_size(tmp_path / "scans" / "interpolation.png") == size
    saved = torch.load(tmp_path / "scans" / "interpolation.pt")
    assert set(saved) == {"x_a", "x_b", "latents", "frames"}
    assert saved["x_a"].shape == saved["x_b"].shape == (1, 2, H, W) and saved["latents"].shape == saved["frames"].shape == (F, 1, 2, H, W)
    names = sorted(p.name for p in (tmp_path / "points").iterdir())
    assert names == [f"frame_{k:04d}.bin" for k in range(F)]
    for n in names:
        pts = np.fromfile(tmp_path / "points" / n, dtype=np.float32)
        assert pts.size % 4 == 0 and pts.size > 0 and np.isfinite(pts).all()
        assert pts.reshape(-1, 4).shape[1] == 4
    # two noise draws at t = 1 instead of two scans: no inversion, no JSON line
    out = _run([f"{ROOT}/interpolate.py", "--ckpt", ckpt_file, "--seed_a", 1, "--seed_b", 2, "--frames", F, "--steps", 2, "--out_dir", tmp_path / "seeds"], tmp_path)
    assert not [line for line in out.splitlines() if line.startswith("{")]
    assert _png_size(tmp_path / "seeds" / "interpolation.png") == size
    saved = torch.load(tmp_path / "seeds" / "interpolation.pt")
    assert set(saved) == {"latents", "frames"} and saved["latents"].shape == saved["frames"].shape == (F, 1, 2, H, W)
    g = r2dm_amd.setup_rng([1], DEV)
    assert torch.equal(saved["latents"][0, 0], torch.randn(2, H, W, generator=g[0], device=DEV).cpu())  # (w = 0: the first draw itself)
