"""The fp16 range guard's GroupNorm bound on the CPU: range_cases.py's mirror of gn_moments / gn_affine / gn_bound (gn_math.h) over its table of
data cases, for the statistics of every summation class the producers have and for both ways gn_finalize_kernel gets its M.  The mirror is
the contract that test_hip_range_producers.py holds the kernels to; here the contract itself is checked:

  soundness   bound (1 + 2^-20) >= float32(max|a x + d|) with the mirror's own (a, d), the product in fp64.  The slack is derived: the bound
              carries two or three fp32 roundings of 2^-24; the guard's threshold 65504 sits 2.4e-4 below 65520, where an fp16 conversion
              first overflows.
  tightness   wherever the variance has not cancelled (gn_moments' well_conditioned) the bound is at most (1 + 1e-5) min(|a| M + |d|, W) with
              W = |w| sqrt(n (1 + 2^-18 (1 + mean^2 rstd^2))) + |sh| in fp64, the worst case as widened for computed statistics; for
              |mean| rstd < 1 that is within (1 + 1e-5) of the unwidened |w| sqrt(n) + |sh| too, and asserted so.  Zero-mean unit noise at
              w = 1, sh = 0 stays below 0.05 x 65504 (test_hip_range.py asserts that figure on a model).
  non-finite  an inf or a NaN in the data gives a bound that !(bound < 65504) catches, with a positive sign: it travels through atomicMax on
              int bits.

What this table found: Samuelson's |x_hat| <= sqrt(n - 1) holds for the exact variance, and gn_bound used it with a margin of 1e-6 wherever
var > 1e-6 mean^2.  A spike on a pedestal of 600 ... 900 sigma (case d) sits at sqrt(n - 1) to five digits while the computed variance is off
by (sums' relative error) x mean^2 / var: the 'four' class exceeded that bound by up to 5e-4, the 'f32' class by a few 1e-3
(test_unwidened_worst_case_bound_is_exceeded_by_computed_statistics keeps the old formula and the finding).  gn_bound now widens the
worst-case bound by sqrt(1 + 2^-18 (1 + mean^2 rstd^2)) -- range_cases.py's docstring derives the 2^-18."""
import numpy as np
import pytest

import range_cases as RC

M_SOURCES = ("sink", "stream")  # M = sqrt(largest slot energy) | the exact max|x|


def run(name, cls, source, bound_fn=RC.bound):
    x, w, sh = RC.TABLE[name]()
    slots = RC.slot_sums(x, cls, RC.F32_SLOT if cls == "f32" else 512) if source == "sink" else None
    return x, w, sh, RC.Result(x, w, sh, slots, bound_fn)


def sources(cls):
    return M_SOURCES if cls == "fp64" else ("sink",)  # (the streaming pass is fp64 from the first addition)


GRID = [(n, c, s) for n in RC.FINITE for c in RC.CLASSES for s in sources(c)]


@pytest.mark.parametrize("name,cls,source", GRID, ids=["-".join(g) for g in GRID])
def test_bound_is_sound_and_tight(name, cls, source):
    x, w, sh, res = run(name, cls, source)
    print(RC.line(f"{name} {cls} {source}", res))
    assert res.sound(), (float(res.record), float(res.applied))
    if bool(res.wc):
        r = float(res.mean) * float(res.rstd)
        w64, sh64 = np.abs(w).astype(np.float64), np.abs(sh).astype(np.float64)
        widened = w64 * np.sqrt(res.n * (1.0 + RC.SUMS_EPS * (1.0 + r * r))) + sh64
        assert (res.bound.astype(np.float64) <= (1.0 + 1e-5) * np.minimum(res.data_bound.astype(np.float64), widened)).all(), (res.bound, widened)
        if abs(r) < 1.0:
            assert (res.bound.astype(np.float64) <= (1.0 + 1e-5) * np.minimum(res.data_bound.astype(np.float64), w64 * np.sqrt(float(res.n)) + sh64)).all()
    assert bool(res.wc) == (name[0] != "c"), name
    if name == "a-noise":
        assert float(res.record) < 0.05 * RC.FP16_MAX


def test_case_d_is_what_it_claims():
    """var / mean^2 in [1.2e-6, 3e-6], in fp64 on the data themselves: gn_moments calls such a group well conditioned; and the spike's exact
    normalised value is within 1e-4 of Samuelson's sqrt(n - 1)."""
    for name in [k for k in RC.TABLE if k.startswith("d-")]:
        x = RC.TABLE[name]()[0].astype(np.float64)
        mean, var = x.mean(), x.var()
        assert 1.2e-6 <= var / mean ** 2 <= 3e-6, (name, var / mean ** 2)
        assert 1.0 - 1e-4 < np.abs(x - mean).max() / np.sqrt(var) / np.sqrt(x.size - 1.0) <= 1.0
        for cls in RC.CLASSES:
            s = RC.slot_sums(x.astype(np.float32), cls, RC.F32_SLOT if cls == "f32" else 512).sum(0)
            assert bool(RC.moments(s[0], s[1], x.size)[2]), (name, cls)


def test_case_e_takes_the_worst_case_branch():
    """The spike on zero-mean noise: the worst-case bound is the smaller one, whichever M."""
    for cls, source in (("fp64", "sink"), ("fp64", "stream"), ("four", "sink")):
        res = run("e-spike", cls, source)[3]
        assert set(res.branch.reshape(-1).tolist()) == {"worst"} and bool(res.wc)


def test_constant_group_takes_the_cancelled_variance_form():
    for name in ("c-const3.25", "c-const0.1", "c-const1e-3-shift1"):
        for cls in RC.CLASSES:
            res = run(name, cls, "sink")[3]
            assert not bool(res.wc) and res.sound()
    res = run("c-const1e-3-shift1", "fp64", "stream")[3]  # (the shift cancels mean * a in d: the form that never cancels is three times the data bound)
    assert set(res.branch.reshape(-1).tolist()) == {"safe"} and float(res.record) > 2.9 > 1.1 > float(res.data_bound.max())


def test_unwidened_worst_case_bound_is_exceeded_by_computed_statistics():
    """The finding, kept: gn_bound as it was (range_cases.bound_before) is sound on the whole table for exact (fp64) statistics, and on case (d)
    it is exceeded for the four-pixel class on some draws and for the fp32-slot class on some draws by more than 1e-3 -- where the bound of today
    is sound on every one."""
    excess = {cls: [] for cls in RC.CLASSES}
    for name in RC.FINITE:
        for cls in RC.CLASSES:
            old, new = run(name, cls, "sink", RC.bound_before)[3], run(name, cls, "sink")[3]
            assert new.sound()
            if not name.startswith("d-"):
                assert old.sound(), (name, cls)
            else:
                excess[cls].append(float(old.applied) / float(old.record) - 1.0)
    print({cls: [f"{e:+.2e}" for e in v] for cls, v in excess.items()})
    assert max(excess["fp64"]) <= 2.0 ** -20
    assert max(excess["four"]) > 1e-4 and sum(e > 2.0 ** -20 for e in excess["four"]) >= 2
    assert max(excess["f32"]) > 1e-3 and sum(e > 2.0 ** -20 for e in excess["f32"]) >= 2


@pytest.mark.parametrize("name", ["g-inf", "h-nan"])
@pytest.mark.parametrize("cls,source", [(c, s) for c in RC.CLASSES for s in sources(c)])
def test_non_finite_data_give_a_bound_the_guard_catches(name, cls, source):
    res = run(name, cls, source)[3]
    print(RC.line(f"{name} {cls} {source}", res))
    for b in res.bound.reshape(-1):
        assert not (b < np.float32(RC.FP16_MAX))
        bits = int(np.float32(b).view(np.int32))
        assert bits > 0 and bits >= int(np.float32(RC.FP16_MAX).view(np.int32)), hex(bits & 0xFFFFFFFF)  # (what atomicMax compares)


def test_mirror_rounds_like_fp32():
    """The mirror's operations stay float32 (numpy would silently promote a Python float operand)."""
    x, w, sh = RC.TABLE["f-adagn6000"]()
    res = RC.Result(x, w, sh, RC.slot_sums(x, "four", 512))
    for t in (res.mean, res.rstd, res.a, res.d, res.gmax, res.bound, res.data_bound):
        assert t.dtype == np.float32
    assert RC.ulps(1.0, np.nextafter(np.float32(1), np.float32(2))) == 1
