"""CPU model of the three summation classes the fused GroupNorm statistics come in (test_hip_conv_engine_paths.py's docstring), under a DC
offset: synthetic N(+-R sigma, sigma) groups of every case's size, the class's [sum, sum of squares] in numpy fp32 / fp64, then the
arithmetic of gn_moments / gn_affine (gn_math.h) and the fp32 fma(x, a, d) of the consumers -- against fp64 GroupNorm, under the bar of
gn_dc_cases.bar (errors relative to torch's fp32 GroupNorm of the same data).

  f32   a statistics slot's 512 values pairwise in fp32, fp64 from the slot on (conv_f16x2.hip's one-plane instance);
  four  (v0 + v1) + (v2 + v3) and fma(v3, v3, fma(v2, v2, fma(v1, v1, v0 v0))) in fp32, fp64 beyond (conv_epilogue_wide; conv_f16x2.hip's
        two-plane instance since this test exists);
  fp64  every addition in fp64 (conv_epilogue, the FIR and down-GEMM statistics, the streaming kernel).

It is a model, not a measurement: it says which (case, R) pairs the GPU ladder may assert (every one where 'four' meets the bar), and why
the parity path cannot keep the f32 class -- var = E[x^2] - mean^2 multiplies the sums' relative error by R^2."""
import functools

import numpy as np
import pytest
import torch

import gn_dc_cases as D

CLASSES = ("f32", "four", "fp64")


def pairwise_f32(a):
    """Pairwise fp32 sum along the last axis (a power of two long)."""
    a = a.astype(np.float32)
    while a.shape[-1] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


def four_pixel_sums(v):
    """v (..., 4) float32 -> the fp32 four-pixel sum and sum of squares of the kernels' epilogues."""
    v0, v1, v2, v3 = (v[..., i] for i in range(4))
    s = (v0 + v1) + (v2 + v3)
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)  # (a b is exact in fp64)
    q = fma(v3, v3, fma(v2, v2, fma(v1, v1, v0 * v0)))
    return s, q


def class_sums(y, cls):
    """[sum, sum of squares] per (sample, group) of y (B, groups, n) float32, as float64."""
    if cls == "fp64":
        t = y.astype(np.float64)
        return t.sum(-1), (t * t).sum(-1)
    if cls == "four":
        s, q = four_pixel_sums(y.reshape(*y.shape[:2], -1, 4))
        return s.astype(np.float64).sum(-1), q.astype(np.float64).sum(-1)
    t = y.reshape(*y.shape[:2], -1, 512)  # f32: 512 values per slot
    return pairwise_f32(t).astype(np.float64).sum(-1), pairwise_f32(t * t).astype(np.float64).sum(-1)


def normalise(y, s, q):
    """gn_moments + gn_affine (weight 1, shift 0) + the consumers' fp32 fma: y (B, groups, n) float32, s and q float64."""
    n = float(y.shape[-1])
    mean_d = s / n
    var_d = np.maximum(q / n - mean_d * mean_d, 0.0)
    mean, rstd = mean_d.astype(np.float32), (1.0 / np.sqrt(var_d + np.float64(np.float32(D.EPS)))).astype(np.float32)
    a = rstd * np.float32(1.0)
    d = (-mean.astype(np.float64) * a.astype(np.float64) + 0.0).astype(np.float32)  # fmaf(-mean, a, sh): one rounding
    return (y.astype(np.float64) * a.astype(np.float64)[..., None] + d.astype(np.float64)[..., None]).astype(np.float32)  # (one rounding too)


@functools.lru_cache(maxsize=None)
def model(case, R, draw=0):
    """{class: (ok, max ratio, rms ratio, max error, rms error)} of one draw of one (case, R)."""
    cin, cout, h, w, B, G, cpg = case
    g = torch.Generator().manual_seed(100003 * draw + 1000 * D.CASES.index(case) + R)
    y = torch.randn(B, G, cpg * h * w, generator=g, dtype=torch.float64) + (D.signs(G) * R)[None, :, None]
    y = y.float()
    ref64, ref_err = D.references(y.reshape(B, cout, h, w), G)
    out = {}
    for cls in CLASSES:
        s, q = class_sums(y.numpy(), cls)
        x_hat = torch.from_numpy(normalise(y.numpy(), s, q)).reshape(B, cout, h, w)
        out[cls] = D.bar(x_hat, ref64, ref_err)
    return out


def show(case, R, res):
    print(f"{D.case_id(case)} R={R:2d}: " + " | ".join(f"{cls} max x{res[cls][1]:.2f} ({res[cls][3]:.2e}) rms x{res[cls][2]:.2f}" for cls in CLASSES)
          + ("" if D.asserted(case, R) else "  [recorded, not asserted]"))


ASSERTED_DRAWS, RECORDED_DRAWS = 4, 32


@pytest.mark.parametrize("R", D.LADDER)
@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_four_and_fp64_classes_meet_the_bar_under_a_dc_offset(case, R):
    """Every pair the GPU ladder asserts: both classes meet the bar on every draw.  Every pair the table marks 'recorded': the mark is earned
    -- the 'four' class misses the bar on some of 32 draws -- and the exact class still meets it (the GPU ladder asserts the streaming
    statistics and the fp64 producers there)."""
    res = model(case, R)
    show(case, R, res)
    if D.asserted(case, R):
        for draw in range(ASSERTED_DRAWS):
            res = model(case, R, draw)
            assert res["four"][0], ("four", draw, res["four"])
            assert res["fp64"][0], ("fp64", draw, res["fp64"])
    else:
        misses = sum(not model(case, R, draw)["four"][0] for draw in range(RECORDED_DRAWS))
        print(f"    the four class misses the bar on {misses} of {RECORDED_DRAWS} draws")
        assert misses >= 1, f"{D.case_id(case)} R={R} is marked 'recorded' but the four class meets the bar on {RECORDED_DRAWS - misses} of {RECORDED_DRAWS} draws"
        assert all(model(case, R, draw)["fp64"][0] for draw in range(ASSERTED_DRAWS))


def test_recorded_pairs_are_the_top_of_the_ladder_and_explained():
    """The table marks R = 64 (every geometry, each with its reason: gn_dc_cases.RECORDED) and nothing below it."""
    assert set(D.RECORDED) == {(case, 64) for case in D.CASES}
    assert all(len(reason) > 40 for reason in D.RECORDED.values())


@pytest.mark.parametrize("case", [c for c in D.CASES if c[6] * c[2] * c[3] <= 16384], ids=D.case_id)
def test_f32_class_misses_the_bar_at_r16_on_the_small_groups(case):
    """Why conv_f16x2.hip's parity instances left the f32 class: with 4 ... 32 slots per group the fp32 roundoff of a slot's 512-value sums,
    times R^2 = 256, is several times the error of an fp32 GroupNorm.  Kept as an assertion so that the model stays honest: if this passes
    the bar, the model no longer tells the classes apart."""
    for draw in range(ASSERTED_DRAWS):
        res = model(case, 16, draw)
        show(case, 16, res)
        assert not res["f32"][0], res["f32"]
        assert res["f32"][1] > res["four"][1] and res["f32"][2] > res["four"][2]
