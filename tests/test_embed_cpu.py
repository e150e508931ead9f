"""CPU: the reference of test_hip_embed.py is right, and its inputs and bound would reject a subtly wrong kernel.

  * embed_oracle's stages against the reference's golden vectors, the torch oracle and the package's frequency table;
  * on every input set of test_hip_embed.py: a float64 model of the kernels (their summation order, unrounded) is inside the derived
    bound with a margin of four, and the mutants of embed_oracle -- each a wrong kernel restated -- are outside it; the table at the end
    says which input set rejects which mutant.  Every mutant must die on at least one set, and on the network's own shape;
  * the exact cases are exact: integers below 2^24 throughout, and results that tell samples and rows apart.
"""
import collections
import types

import numpy as np
import pytest
import torch

import embed_oracle as E
from conftest import GOLDEN_RES, synthetic_ckpt

MARGIN = 4.0
_table = collections.OrderedDict()  # mutant -> {set label: killed?}


def record(mutant, label, killed):
    _table.setdefault(mutant, collections.OrderedDict())[label] = killed


def model_margin(w, a, bias, stage):
    """The float64 kernel model against the wide reference, in units of the float64 share of the bound (delta): <= 1 / MARGIN."""
    pre = getattr(stage, "pre", stage)
    with np.errstate(invalid="ignore"):
        err = np.abs(E.dot_kernel_order(w, a, bias, np.float64) - pre.value) / pre.delta
    return float(np.nanmax(err))


def silu_store(p):
    """What a SiLU stage stores for the float32 pre-activation p."""
    return E.f32(E.silu64(p))


@pytest.fixture(scope="module")
def sd():
    from oracle import r2dm_oracle as O

    return O.strip_prefix(synthetic_ckpt(resolution=GOLDEN_RES)["ema_weights"])


# ---- the oracle against the golden files ------------------------------------------------------------------------------------------------------
def test_sinusoid_against_the_reference(golden):
    g = golden("ops")
    emb = E.sinusoid(g["sin_t"].numpy(), E.freqs(64))
    assert emb.shape == g["sin_y"].shape
    assert E.ulps(emb, g["sin_y"].numpy()) <= 2  # the reference's own float32 sin / cos


def test_composed_embedding_against_the_reference(golden, sd):
    from oracle import r2dm_oracle as O

    g = golden("ops")
    w = [sd[f"time_embedding.{i}.{n}"].numpy() for i in (1, 3) for n in ("weight", "bias")]
    emb, hid, act = E.time_embedding(g["sin_t"].numpy(), E.freqs(64), *w)
    temb = act.pre.value  # Linear -> SiLU -> Linear: the pre-activation of the second SiLU
    assert np.abs(temb - g["temb_y"].double().numpy()).max() < 1e-6
    ref = O.time_embedding(sd, O.UNetConfig(resolution=GOLDEN_RES), g["sin_t"])
    assert np.abs(temb - ref.double().numpy()).max() < 1e-6
    assert np.abs(act.value - torch.nn.functional.silu(g["temb_y"].double()).numpy()).max() < 1e-6


@pytest.mark.parametrize("base", [8, 32, 64, 128])
def test_frequency_table_is_the_package_s(base):
    from r2dm_amd.unet import EfficientUNet

    me = types.SimpleNamespace(geometry=types.SimpleNamespace(coords_encoding=None, base_channels=base))
    table = EfficientUNet._constants(me, {})["__sin_freqs"]
    assert table.dtype == torch.float32 and np.array_equal(table.numpy().view(np.int32), E.freqs(base).view(np.int32))
    assert E.freqs(base)[0] == 1.0 and abs(float(E.freqs(base)[-1]) - 1e-4) < 1e-10


def test_wide_sum_is_wider_than_float64():
    """dot_wide against math.fsum (exact) on cancelling terms, where a float64 sum in any order loses digits."""
    import math

    g = E.rng(3)
    w = (g.standard_normal((4, 300)) * 2.0 ** g.integers(-20, 20, (4, 300))).astype(np.float32)
    a = g.standard_normal((3, 300)).astype(np.float32)
    bias = g.standard_normal(4).astype(np.float32)
    wide, mass = E.dot_wide(w, a, bias)
    for b in range(3):
        for r in range(4):
            exact = math.fsum([float(x) * float(y) for x, y in zip(w[r], a[b])] + [float(bias[r])])
            assert abs(wide[b, r] - exact) <= 2.0 ** -53 * abs(exact) + 2.0 ** -60 * mass[b, r]


def test_ulps_and_within_bound():
    one = np.float32(1.0)
    assert E.ulps(np.nextafter(one, np.float32(2)), one) == 1.0 and E.ulps(one, one) == 0.0
    assert E.ulps(np.float32("nan"), one) == float("inf") and E.ulps(np.float32("nan"), np.float32("nan")) == 0.0
    st = E.dot_stage(np.ones((1, 4), np.float32), np.full((1, 4), 0.25, np.float32), np.zeros(1, np.float32))
    assert E.within_bound(np.float32([[1.0]]), st)[:2] == (True, 0.0)
    ok, worst, flips = E.within_bound(np.nextafter(np.float32([[1.0]]), np.float32(2)), st)
    assert not ok and 1.9 < worst <= 2.0 and flips == 1
    assert not E.within_bound(np.float32([[np.nan]]), st)[0]


# ---- mutants on the GPU test's inputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base,T", E.TIME_SHAPES)
def test_time_embedding_sets_reject_the_mutants(base, T):
    fr = E.freqs(base)
    w1, b1, w2, b2 = E.time_weights(base, T)
    for B in E.TIME_BATCHES:
        t = E.conds(B)
        label = f"time ({base},{T}) B={B}"
        emb, hid, act = E.time_embedding(t, fr, w1, b1, w2, b2)
        for name, st, (w, a, bias) in (("hidden", hid, (w1, emb, b1)), ("act", act, (w2, hid.ref, b2))):
            assert model_margin(w, a, bias, st) <= 1 / MARGIN, (label, name)
            ok, worst, _ = E.within_bound(silu_store(E.f32(E.dot_kernel_order(w, a, bias, np.float64))), st)
            assert ok, (label, name, worst)
            for m, f in E.DOT_MUTANTS.items():
                record(m, f"{label} {name}", not E.within_bound(silu_store(f(w, a, bias)), st)[0])
        for m, f in E.SINUSOID_MUTANTS.items():
            record(m, f"{label} hidden", not E.within_bound(silu_store(E._dot(w1, f(t, fr), b1)), hid)[0])


def sinusoid_sets(golden):
    return dict(E.SIN_CONDS, golden=golden("ops")["sin_t"].numpy())


@pytest.mark.parametrize("base", [64, 8])
def test_sinusoid_sets_reject_the_mutants(golden, base):
    """The one-hot case sees the embedding through SiLU alone: one ulp of f32(silu64(emb)) tells the [sin | cos] order and a float32
    sinusoid from the kernel's."""
    fr = E.freqs(base)
    for name, t in sinusoid_sets(golden).items():
        want = silu_store(E.sinusoid(t, fr))
        for m, f in E.SINUSOID_MUTANTS.items():
            record(m, f"one-hot base {base} {name}", E.ulps(silu_store(f(t, fr)), want) > 1)
    assert all(_table["sin / cos halves swapped"][f"one-hot base {base} {n}"] for n in ("unit", "discrete", "extreme", "golden"))
    assert _table["fp32 sin / cos"][f"one-hot base {base} discrete"] and _table["fp32 sin / cos"][f"one-hot base {base} extreme"]


@pytest.mark.parametrize("base,T", E.TIME_SHAPES)
def test_time_exact_case_is_exact(base, T):
    w1, b1, n = E.time_exact(base, T)
    emb = E.sinusoid(np.zeros(3, np.float32), E.freqs(base))
    assert np.array_equal(emb, np.concatenate([np.zeros((3, base // 2)), np.ones((3, base // 2))], 1))
    assert np.abs(w1).sum(axis=1).max() + np.abs(b1).max() < 2 ** 24
    want = silu_store(n.astype(np.float64))
    label = f"time exact ({base},{T})"
    got = silu_store(E.dot_kernel_order(w1, emb, b1, np.float64))
    assert np.array_equal(got, np.broadcast_to(want, got.shape))
    for m, f in E.DOT_MUTANTS.items():
        if m != "fp32 accumulation":  # (integers: an fp32 sum is exact too)
            mutant = silu_store(f(w1, emb, b1))
            record(m, label, E.ulps(mutant, np.broadcast_to(want, mutant.shape)) > 1)
    if T >= 64:  # (rows enough that some |n| is small: one ulp of silu(n) separates n from n +- w)
        assert _table["last term dropped"][label] and _table["term T-1 twice"][label] and _table["bias of row r+1"][label]


@pytest.mark.parametrize("T,B,rows", E.ada_cases())
def test_ada_proj_sets_reject_the_mutants(T, B, rows):
    label = f"ada_proj T={T} B={B} rows={rows}"
    # exact: integers throughout, results that tell samples and rows apart, and every mutant changes bits
    act, w, bias, out = E.ada_exact(T, B, rows)
    assert (np.abs(act.astype(np.int64)) @ np.abs(w.astype(np.int64)).T + np.abs(bias.astype(np.int64))[None, :]).max() < 2 ** 24
    assert all(len(set(out[:, r])) == B for r in range(rows)) and all(len(set(out[b])) == rows for b in range(B))
    assert np.array_equal(E.dot_kernel_order(w, act, bias, np.float64), out) and np.array_equal(E._dot(w, act, bias), out)
    for m, f in {**E.DOT_MUTANTS, **E.SAMPLE_MUTANTS}.items():
        if m == "fp32 accumulation":
            continue
        mutant = f(w, act, bias)
        if mutant is not None:
            record(m, label + " exact", not np.array_equal(mutant, out.astype(np.float32)))
            assert _table[m][label + " exact"], (label, m)
    # random
    act, w, bias = E.ada_random(T, B, rows)
    st = E.dot_stage(w, act, bias)
    assert model_margin(w, act, bias, st) <= 1 / MARGIN, label
    assert E.within_bound(E.f32(E.dot_kernel_order(w, act, bias, np.float64)), st)[0]
    for m, f in {**E.DOT_MUTANTS, **E.SAMPLE_MUTANTS}.items():
        mutant = f(w, act, bias)
        if mutant is not None:
            record(m, label + " random", not E.within_bound(mutant, st)[0])
            if m != "fp32 accumulation" or B * rows >= 45:  # (a single fp32 sum is the correctly rounded one about one time in three)
                assert _table[m][label + " random"], (label, m)


def test_checkpoint_projections_reject_the_mutants(sd):
    """The golden-resolution checkpoint's own 24 projections, packed as the engine packs them."""
    w, bias = E.packed_ada({k: v.numpy() for k, v in sd.items()})
    assert w.shape == (sum(v.shape[0] for k, v in sd.items() if k.endswith("norm2.proj.1.bias")), 256) and bias.shape == w.shape[:1]
    act = E.ada_random(256, 9, 5)[0]
    st = E.dot_stage(w, act, bias)
    assert model_margin(w, act, bias, st) <= 1 / MARGIN
    for m, f in {**E.DOT_MUTANTS, **E.SAMPLE_MUTANTS}.items():
        record(m, "ada_proj checkpoint B=9", not E.within_bound(f(w, act, bias), st)[0])


def test_every_mutant_dies_and_the_table(capsys):
    """(last in the file: the tests above fill the table)  Every mutant is rejected by some input set and by the network's own shape."""
    names = list(E.DOT_MUTANTS) + list(E.SAMPLE_MUTANTS) + list(E.SINUSOID_MUTANTS)
    with capsys.disabled():
        print("\nmutant: rejected by / applicable input sets; the sets it survives")
        for m in names:
            sets = _table.get(m, {})
            alive = [s for s, k in sets.items() if not k]
            print(f"  {m:26s} {sum(sets.values()):4d} / {len(sets):4d}" + (f"  survives: {'; '.join(alive[:12])}{' ...' if len(alive) > 12 else ''}" if alive else ""))
    for m in names:
        assert any(_table.get(m, {}).values()), f"no input set rejects the mutant '{m}'"
    net = {"hidden": "time (64,256) B=33 hidden", "act": "time (64,256) B=33 act", "proj": "ada_proj T=256 B=33 rows=130 random"}
    for m in E.DOT_MUTANTS:
        for s in net.values():
            assert _table[m][s], (m, s)
    for m in E.SAMPLE_MUTANTS:
        assert _table[m][net["proj"]] and _table[m]["ada_proj T=256 B=33 rows=130 exact"], m
    for m in E.SINUSOID_MUTANTS:
        assert _table[m][net["hidden"]], m
