"""-m gpu: data-consistent completion -- ``r2dm_posterior_step_known`` (r2dm_amd/csrc/posterior.hip) against its contract in torch ops
(tests/complete_oracle.py), what the entry refuses, ``ContinuousTimeGaussianDiffusion.complete`` against the oracle in float64 and, with a
denoiser that is itself torch ops, against the oracle's float32 loop bit for bit, its identities with ``sample`` / ``sample_from``, and the
``ddnm`` method of ``evaluate_completion``, ``completion_eval.py`` and ``completion_demo.py``.

Bars: the kernel and the loop with a torch denoiser are exact (one IEEE rounding per operation, no contraction, in the contract's order).
With the U-Net the bar is the project's relative one (``relative_bar`` of tests/test_hip_latent.py): the distance to the float64 oracle
within 2x of the float32 oracle's own in rms and at the 99th percentile, within 4x at the worst element."""
import functools
import json
import subprocess
import sys

import pytest
import torch

from conftest import GOLDEN_RES, ROOT, rnd, synthetic_ckpt

import complete_oracle as CO
import latent_oracle as LO
import test_hip_completion as TC  # (its two small scans)
import test_hip_latent as TL  # (the cached models and oracle nets, relative_bar, AnalyticDenoiser)

import r2dm_amd
from oracle import r2dm_oracle as O
from r2dm_amd import _lib, completion

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 3
H, W = GOLDEN_RES
SHAPE = (B, 2, H, W)
OBJECTIVES = ["eps", "v", "x_0"]


# ---- 1. r2dm_posterior_step_known -------------------------------------------------------------------------------------------------
# rows from t = 1 (alpha ~ 5.5e-4: the eps estimate is far outside the clamp), in between, and to t = 0 (c ~ 1, sigma_s ~ 5.5e-4)
T_ROWS, S_ROWS = [1.0, 0.4, 0.25], [0.75, 0.1, 0.0]
MODES = [("ddpm", 0.0), ("ddim", 0.0), ("ddim", 0.5)]
# 4096: one pass of four blocks.  1024 blocks x 256 threads x 4 elements is one pass of the capped grid: 4 KiB more is a second pass
PER_SAMPLE = [4096, 1024 * 256 * 4 + 4096]
C = 2


def kernel_case(per_sample, mask_c, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    plane = per_sample // C
    x, pr, z = (torch.randn(B, C, plane, generator=g, device=DEV) for _ in range(3))
    y = torch.tanh(torch.randn(B, C, plane, generator=g, device=DEV))
    m = torch.empty(B, mask_c, plane, device=DEV)
    m[0] = (torch.rand(mask_c, plane, generator=g, device=DEV) < 0.5).float()  # binary
    m[1] = 0.25  # the weight form
    m[2] = 1.0
    return x, pr, z, y, m


@pytest.mark.parametrize("per_sample", PER_SAMPLE)
@pytest.mark.parametrize("mask_c", [1, C])
@pytest.mark.parametrize("mode,eta", MODES)
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_posterior_step_known_bit_exact_vs_torch_ops(objective, mode, eta, mask_c, per_sample):
    ddpm = TL.model()[0]
    _, coef, mode_id = ddpm._coefficients(torch.tensor(T_ROWS), torch.tensor(S_ROWS), mode, eta)
    assert coef.shape == (B, 8) and mode_id == (0 if mode == "ddpm" else 1)
    if eta:
        assert (coef[:2, 6] > 0).all()  # c1 != 0: the noise enters the DDIM update
    coef = coef.to(DEV)
    x, pr, z, y, m = kernel_case(per_sample, mask_c, per_sample % 1000 + 10 * OBJECTIVES.index(objective) + mask_c)
    obj_id = OBJECTIVES.index(objective)
    k = {name: coef[:, j][:, None, None] for name, j in (("a_t", 0), ("s_t", 1), ("a_s", 2), ("c", 4), ("sd", 5), ("c1", 6), ("c2", 7))}
    for clip in (1.0, -1.0):
        got = _lib.posterior_step_known(x, pr, z, y, m, coef, mode_id, obj_id, clip)
        want = CO.posterior_known(x, pr, z, y, m, mode=mode, objective=objective, clip=clip, **k)  # (one rounding per torch op)
        assert got.dtype == torch.float32 and got.shape == x.shape and torch.isfinite(got).all()
        assert torch.equal(got, want), (clip, (got - want).abs().max().item())
        # nothing known: the plain posterior step
        zero = torch.zeros_like(m)
        assert torch.equal(_lib.posterior_step_known(x, pr, z, y, zero, coef, mode_id, obj_id, clip), _lib.posterior_step(x, pr, z, coef, mode_id, obj_id, clip))
    # all known (sample 2): the estimate is the measurement whatever the (clamped) prediction
    a, b = (_lib.posterior_step_known(x, q, z, y, m, coef, mode_id, obj_id, 1.0) for q in (pr, pr.flip(-1)))
    assert torch.equal(a[2], b[2]) and not torch.equal(a[0], b[0])


def test_posterior_step_known_refusals():
    """each refusal is a non-zero status with its message in ``r2dm_last_error``; nothing is launched, nothing faults"""
    L = _lib.lib()
    n = 4096
    buf = torch.zeros(2 * n + 4, device=DEV)
    ok, off = buf[:2 * n], buf[1:1 + 2 * n]
    assert off.data_ptr() % 16 == 4
    coef = torch.ones(2, 8, device=DEV)
    out = torch.empty(2 * n, device=DEV)
    stream = _lib.stream_ptr(torch.device(DEV, 0))

    def call(x=ok, pr=ok, z=ok, y=ok, m=ok, k=coef, o=out, batch=2, per_sample=n, channels=2, mask_c=1, mode=0, objective=0):
        p = lambda t: None if t is None else t.data_ptr()
        return L.r2dm_posterior_step_known(p(x), p(pr), p(z), p(y), p(m), p(k), p(o), batch, per_sample, channels, mask_c, mode, objective, 1.0, stream)

    def refused(text, **kw):
        assert call(**kw) != 0, kw
        msg = L.r2dm_last_error().decode()
        assert msg.startswith("posterior_step_known: ") and text in msg, (kw, msg)

    assert call() == 0 and call(mask_c=2, mode=1, objective=2) == 0
    for name in ("x", "pr", "z", "y", "m", "o"):
        refused("16-byte aligned", **{name: off})
    odd = coef.view(torch.uint8).flatten()[1:]
    assert odd.data_ptr() % 4 == 1
    refused("4-byte aligned", k=odd)
    refused("multiple of 4", per_sample=4098)
    refused("multiple of 4", per_sample=4092, channels=2, mask_c=1)  # a plane of 2046
    refused("mask_channels", mask_c=3, channels=2)
    refused("mode", mode=2)
    refused("mode", mode=-1)
    refused("objective", objective=3)
    refused("batch", batch=0)
    refused("batch", batch=65536)
    for name in ("x", "pr", "z", "y", "m", "k", "o"):
        refused("null", **{name: None})
    # the wrapper: operands of one shape, a (B,8) row
    x4 = torch.zeros(2, 2, 16, 64, device=DEV)
    with pytest.raises(ValueError):
        _lib.posterior_step_known(x4, x4, x4, x4[:, :1], x4[:, :1], coef, 0, 0, 1.0)
    with pytest.raises(ValueError):
        _lib.posterior_step_known(x4, x4, x4, x4, x4[:, :1], coef[:, :2], 0, 0, 1.0)
    with pytest.raises(_lib.R2DMError, match="multiple of 4"):
        _lib.posterior_step_known(*([torch.zeros(2, 1, 4098, device=DEV)] * 5), coef, 0, 0, 1.0)
    torch.cuda.synchronize()


# ---- the inputs the sampler tests share ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scan():
    """(known (B,2,H,W) in [-1, 1], mask (B,1,H,W): about half ones, sample 1 every fourth row) on the device: computed once, left unchanged"""
    known = torch.tanh(rnd(70, *SHAPE))
    g = torch.Generator().manual_seed(5)
    mask = (torch.rand(B, 1, H, W, generator=g) < 0.5).float()
    mask[1] = 0
    mask[1, :, ::4] = 1
    return known.to(DEV), mask.to(DEV)


def tape_of(seeds, n):
    """the first ``n`` draws of ``setup_rng(seeds)``, as every sampler here draws them"""
    g = r2dm_amd.setup_rng(seeds, DEV)
    return [O.draw_noise(SHAPE, g, DEV, torch.float32) for _ in range(n)]


# ---- 3. complete against the oracle in float64 -----------------------------------------------------------------------------------------
RUNS = [(4, 1, 1, "ddpm", False, 1.0), (3, 2, 2, "ddpm", False, 1.0), (4, 2, 1, "ddim", False, 1.0), (3, 2, 1, "ddpm", True, 0.5)]


@pytest.mark.parametrize("S,r,j,mode,with_init,t_start", RUNS)
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_complete_vs_fp64_oracle(objective, S, r, j, mode, with_init, t_start):
    """The oracle's own float32-vs-float64 distance on the CPU (rms / max): eps ddpm 4.8e-6 / 1.1e-4, v ddpm 1.5e-6 / 8.1e-6, x_0 ddpm
    1.1e-7 / 9.0e-7, the ddim runs 2-3.4e-5 / 1.8e-4, the t_start = 0.5 runs ~1e-7 / 1e-6: none is zero, the bar is meaningful.  Measured
    on the MI355X: see DESIGN.md section 4, 'Data-consistent completion'."""
    ddpm = TL.model(objective)[0]
    net32, net64 = TL.nets(objective)
    known, mask = scan()
    init = 0.5 * known if with_init else None
    seeds = list(range(90, 90 + B))
    got = ddpm.complete(known, mask, S, r, j, t_start=t_start, init=init, mode=mode, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV))
    assert got.shape == SHAPE and got.dtype == torch.float32
    tape = tape_of(seeds, CO.num_draws(S, r, j))
    kw = dict(num_resample_steps=r, jump_length=j, t_start=t_start, mode=mode, objective=objective)
    truth = CO.complete(net64, known.double(), mask.double(), S, tape, init=None if init is None else init.double(), **kw)
    ref32 = CO.complete(net32, known, mask, S, tape, init=init, **kw)
    TL.relative_bar(f"complete {objective} S={S} r={r} j={j} {mode} t_start={t_start}", got, ref32, truth)
    on = mask.expand_as(known) == 1
    assert torch.equal(got[on], known[on])


# ---- 4. with a denoiser in torch ops and the schedule on the device: the oracle's float32 loop, bit for bit ----------------------------------
@pytest.mark.parametrize("S,r,j,mode,eta", [(3, 2, 2, "ddpm", 0.0), (4, 1, 1, "ddim", 0.0), (3, 2, 1, "ddim", 0.5)])
def test_complete_with_the_analytic_denoiser_is_the_oracles_loop(S, r, j, mode, eta):
    ddpm = r2dm_amd.ContinuousTimeGaussianDiffusion(TL.AnalyticDenoiser(), prediction_type="eps", noise_schedule="cosine").to(DEV)
    ddpm.set_schedule_on("device")
    known, mask = scan()
    seeds = list(range(120, 120 + B))
    tape = tape_of(seeds, CO.num_draws(S, r, j))
    got = ddpm.complete(known, mask, S, r, j, mode=mode, ddim_eta=eta, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV), return_all=True)
    want = CO.complete(LO.analytic_eps, known, mask, S, tape, r, j, mode=mode, ddim_eta=eta, return_all=True)
    assert got.shape == (1 + S * r - (r - 1), *SHAPE)
    assert torch.equal(got, want), (got - want).abs().max().item()
    # from a partially noised start, and without the final projection
    got = ddpm.complete(known, mask, S, r, j, t_start=0.5, init=0.5 * known, mode=mode, ddim_eta=eta, exact_known=False, progress=False,
                        rng=r2dm_amd.setup_rng(seeds, DEV))
    want = CO.complete(LO.analytic_eps, known, mask, S, tape, r, j, t_start=0.5, init=0.5 * known, mode=mode, ddim_eta=eta, exact_known=False)
    assert torch.equal(got, want), (got - want).abs().max().item()


# ---- 5. identities on the synthetic model ---------------------------------------------------------------------------------------------------
S4 = 4  # (linspace(1, 0, 5) and linspace(0.5, 0, 5) are exact, and so is t + 1 * (s - t): the sub-step grid is the step grid)


@pytest.mark.parametrize("mode", ["ddpm", "ddim"])
def test_complete_with_nothing_known_is_sample(mode):
    ddpm = TL.model()[0]
    known, _ = scan()
    zero = torch.zeros(B, 1, H, W, device=DEV)
    seeds = list(range(50, 50 + B))
    want = ddpm.sample(B, S4, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV), mode=mode, return_all=True)
    got = ddpm.complete(known, zero, S4, mode=mode, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV), return_all=True)
    assert got.shape == (S4 + 1, *SHAPE) and torch.equal(got, want)


def test_complete_from_an_init_with_nothing_known_is_sample_from():
    ddpm = TL.model()[0]
    known, _ = scan()
    zero = torch.zeros(B, 1, H, W, device=DEV)
    seeds = list(range(60, 60 + B))
    g = r2dm_amd.setup_rng(seeds, DEV)
    x_t, _ = ddpm.q_step_from_x_0(known, torch.full((B,), 0.5), rng=g)
    want = ddpm.sample_from(x_t, S4, t_start=0.5, progress=False, rng=g)  # (the generators carried on)
    got = ddpm.complete(known, zero, S4, t_start=0.5, init=known, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV))
    assert torch.equal(got, want)


def test_complete_is_batch_independent_reproducible_and_exact_on_the_mask():
    ddpm = TL.model()[0]
    known, mask = scan()
    S, r, j = 3, 2, 1
    seeds = list(range(70, 70 + B))
    run = lambda **kw: ddpm.complete(known, mask, S, r, j, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV), **kw)
    got = run()
    assert torch.equal(got, run())
    alone = ddpm.complete(known[1:2], mask[1:2], S, r, j, progress=False, rng=r2dm_amd.setup_rng(seeds[1:2], DEV))
    assert torch.equal(alone[0], got[1])
    on = mask.expand_as(known) == 1
    assert torch.equal(got[on], known[on]) and not torch.equal(got[~on], known[~on])
    # a (B,C,H,W) mask and a (1,1,H,W) one are the same masks spelled out
    assert torch.equal(ddpm.complete(known, mask.expand(-1, 2, -1, -1), S, r, j, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV)), got)
    one = ddpm.complete(known, mask[1:2], S, r, j, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV))
    assert torch.equal(one[1], got[1])
    # without the final projection: the known pixels carry the last step's sigma(0) z
    raw = run(exact_known=False)
    a0, s0 = ddpm._alpha_sigma_rows(torch.zeros(1))[0].tolist()
    z_max = max(t.abs().max().item() for t in tape_of(seeds, CO.num_draws(S, r, j)))
    dev = (raw - a0 * known)[on].abs().max().item()
    print(f"exact_known=False: max |x - alpha(0) known| on the mask {dev:.3e}; sigma(0) = {s0:.3e}, max|z| = {z_max:.2f}")
    assert not torch.equal(raw[on], known[on]) and dev <= 6 * s0 * z_max
    assert torch.equal(raw[~on], got[~on])
    # the stack repaint returns: the start, then the x_s of every resampling
    stack = run(return_all=True)
    assert stack.shape == (1 + S * r - (r - 1), *SHAPE) and torch.equal(stack[-1], got)
    rp = ddpm.repaint(known, mask, S, r, j, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV), return_all=True)
    assert rp.shape == stack.shape and torch.equal(rp[0], stack[0])  # (the same first draw)


def test_a_tripped_range_guard_repeats_the_call_on_the_wide_split():
    """The guard's bound is raised behind the third of the five denoiser calls (the C ABI's test hook, as tests/test_hip_range.py uses it): the
    deferred check at the loop's end trips, the model switches to 'fp32-bf16x3' with ONE RuntimeWarning and the whole call runs again from
    the snapshotted generator states -- the result of a model that ran the wide split from the start, bit for bit, and no exception.  With
    ``strict_range`` the trip raises."""
    import warnings

    known, mask = scan()
    S, r, j = 3, 2, 1
    seeds = list(range(130, 130 + B))
    ck = synthetic_ckpt(resolution=GOLDEN_RES)
    wide = r2dm_amd.setup_model(ck, device=DEV, show_info=False, max_batch=B, precision="fp32-bf16x3")[0]
    want = wide.complete(known, mask, S, r, j, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV))

    def tripping(**kw):
        ddpm = r2dm_amd.setup_model(ck, device=DEV, show_info=False, max_batch=B, **kw)[0]
        calls, fwd = [], ddpm.model.forward

        def forward(*a, **k):
            y = fwd(*a, **k)
            calls.append(1)
            if len(calls) == 3:
                _lib.check(_lib.lib().r2dm_test_raise_range_bound(ddpm.model._engine.h, 1.0e5, _lib.stream_ptr(y.device)))
            return y

        ddpm.model.forward = forward
        return ddpm, calls

    ddpm, calls = tripping()
    rng = r2dm_amd.setup_rng(seeds, DEV)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = ddpm.complete(known, mask, S, r, j, progress=False, rng=rng)
    assert sum(issubclass(i.category, RuntimeWarning) and "fp32-bf16x3" in str(i.message) for i in w) == 1
    assert len(calls) == 10 and ddpm.model.precision == "fp32-bf16x3" and ddpm.model.range_fallbacks == 1
    assert torch.equal(got, want)
    strict, _ = tripping(strict_range=True)
    with pytest.raises(_lib.R2DMRangeError):
        strict.complete(known, mask, S, r, j, progress=False, rng=r2dm_amd.setup_rng(seeds, DEV))


# ---- 6. evaluate_completion, completion_eval.py, completion_demo.py -------------------------------------------------------------------
KINDS = ("beams:4", "random_points:0.5")
METHODS = ("ddnm", "repaint", "linear")
SEED = 5


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("complete")
    ckpt = tmp / "synthetic.pth"
    torch.save(synthetic_ckpt(resolution=GOLDEN_RES), ckpt)
    for k, s in enumerate(TC.small_scans()):
        d = tmp / "scans" / f"seq_{k}"
        d.mkdir(parents=True)
        s.tofile(d / f"{k:010d}.bin")
    return tmp, ckpt


def eval_args(tmp, ckpt, name):
    args = ["--ckpt", str(ckpt), "--real_scans", str(tmp / "scans"), "--methods", *METHODS, "--num_steps", "2", "--num_resample_steps", "1",
            "--batch_size", "2", "--seed", str(SEED), "--save_dir", str(tmp / name), "--out", str(tmp / name / "completion.json")]
    for kind in KINDS:
        args += ["--corruption", kind]
    return args


def test_completion_eval_with_the_ddnm_method(files):
    tmp, ckpt = files
    r = subprocess.run([sys.executable, f"{ROOT}/completion_eval.py", *eval_args(tmp, ckpt, "kept")], cwd=tmp, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert any("ddnm: MAE depth" in line for line in r.stdout.splitlines()), r.stdout
    doc = json.loads((tmp / "kept" / "completion.json").read_text())
    info = doc["info"]
    assert info["methods"] == list(METHODS) and (info["ddnm_resample_steps"], info["ddnm_init"], info["ddnm_t_start"]) == (1, "none", 1.0)
    ddpm, lidar, _ = r2dm_amd.setup_model(str(ckpt), device=DEV, show_info=False, max_batch=2)
    for kind in KINDS:
        e = doc["results"][kind]
        assert set(e["ddnm"]) == set(e["repaint"]) == {"counts", "sums", "micro", "macro"}
        assert all(set(e["ddnm"][g]) == set(e["repaint"][g]) for g in e["repaint"])
        assert all(e["ddnm"]["counts"][n] == e["repaint"]["counts"][n] for n in ("scans", "unknown", "evaluated")) and e["ddnm"]["counts"]["evaluated"] > 100
        k = torch.load(tmp / "kept" / (kind.replace(":", "_") + ".pt"))
        x_in, mask, x_out = k["x_in"].to(DEV), k["mask"].to(DEV), k["x_out"]["ddnm"].to(DEV)
        rng = r2dm_amd.setup_rng([completion.scan_seed(SEED, i) for i in range(2)], DEV)
        assert torch.equal(x_out, ddpm.complete(x_in, mask, 2, progress=False, rng=rng))
        on = mask.expand_as(x_in) == 1
        assert torch.equal(x_out[on], x_in[on]) and not torch.equal(x_out, k["x_out"]["repaint"].to(DEV))
        assert torch.equal(lidar.postprocess(x_out.clamp(-1, 1)).cpu(), k["pred"]["ddnm"])


def test_completion_eval_ddnm_from_the_interpolated_scan(files):
    """``--ddnm_init linear --ddnm_t_start 0.5`` (the script's ``main`` in this process): scored for whole rows, skipped for random points"""
    import completion_eval

    tmp, ckpt = files
    doc = completion_eval.main(eval_args(tmp, ckpt, "init") + ["--ddnm_init", "linear", "--ddnm_t_start", "0.5", "--ddnm_resample_steps", "2"])
    assert (doc["info"]["ddnm_resample_steps"], doc["info"]["ddnm_init"], doc["info"]["ddnm_t_start"]) == (2, "linear", 0.5)
    assert set(doc["results"]["beams:4"]["ddnm"]) == {"counts", "sums", "micro", "macro"}
    skipped = doc["results"]["random_points:0.5"]["ddnm"]
    assert set(skipped) == {"skipped"} and "whole rows" in skipped["skipped"]
    assert "skipped" not in doc["results"]["random_points:0.5"]["repaint"] and "skipped" in doc["results"]["random_points:0.5"]["linear"]
    k = torch.load(tmp / "init" / "beams_4.pt")
    x_in, mask, x_out = k["x_in"].to(DEV), k["mask"].to(DEV), k["x_out"]["ddnm"].to(DEV)
    assert "ddnm" not in torch.load(tmp / "init" / "random_points_0.5.pt")["x_out"]
    ddpm = r2dm_amd.setup_model(str(ckpt), device=DEV, show_info=False, max_batch=2)[0]
    init = completion.fill_beams(x_in, completion.rows_of_mask(mask), "linear", nodata=-1.0)
    rng = r2dm_amd.setup_rng([completion.scan_seed(SEED, i) for i in range(2)], DEV)
    assert torch.equal(x_out, ddpm.complete(x_in, mask, 2, 2, t_start=0.5, init=init, progress=False, rng=rng))


def test_completion_demo_with_the_ddnm_method(files):
    tmp, ckpt = files
    (tmp / "demo").mkdir()
    scan_file = next((tmp / "scans").rglob("*.bin"))
    r = subprocess.run([sys.executable, f"{ROOT}/completion_demo.py", "--ckpt", str(ckpt), "--scan", str(scan_file), "--method", "ddnm", "--num_steps", "2",
                        "--num_resample_steps", "1", "--seed", "3"], cwd=tmp / "demo", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    # the default name with the method's prefix; the size of the RePaint run's image (tests/test_hip_projection.py::test_completion_demo)
    assert TL._png_size(tmp / "demo" / "ddnm_completion_T-0002_r-0001_j-0001.png") == (4 * (W + 2) + 2, 4 * H + 2 * W + 4)
    state = torch.load(tmp / "demo" / "completion.pt")
    on = state["mask"] == 1
    assert state["x_out"].shape == (4, 2, H, W) and torch.equal(state["x_out"][on], state["x_in"][on].clamp(-1, 1))
