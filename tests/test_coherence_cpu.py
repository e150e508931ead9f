"""The ensemble coherence scores' host side, without a GPU: the numpy specification (tests/coherence_oracle.py) on the identities it must
satisfy, ``derived_coherence`` / ``aggregate_coherence`` against it, the fixed input that shows what the feature is for, the refusals of
``evaluate_completion`` and of the script, and the C ABI's argument checks.

Tolerances: counts are exact.  ``derived_coherence`` against the oracle's direct formulas: both work on the same float64 sums and differ
only in the order of at most 64 * 63 additions of non-negative roots and in one division more or less, a few 1e-14 at the most; 1e-12
relative.  The invariance under a permutation of the members is bitwise.

The shuffle input (``coherence_oracle.shuffle_inputs(SEED)``: 8 scans of 8 x 32, K = 16, members = a smooth field + one N(0,1) offset per
member + N(0, 0.05^2) per pixel, the truth drawn the same way; the shuffled ensemble holds the same K values at every pixel, permuted
independently).  The two factors asked of it, 1.05 x on the energy score and 10 x on the variogram score, are conditions on the INPUT, set
below the least ratios seen over 30 such groups (1.07 and 21 x); with SEED = 0 the oracle gives 1.157 and 28.0.  They are not tolerances of
the kernel: tests/test_hip_coherence.py holds the kernel to the oracle on this input and so inherits the separation."""
import ctypes
import functools
import json
import math

import numpy as np
import pytest
import torch

import coherence_oracle as O
import completion_oracle as CO

LO, HI = 1.45, 80.0
SEED = 0
OFFSETS = ((0, 1), (0, 2), (0, 4), (0, 8), (1, 0), (2, 0), (1, 1), (1, -1))
ENERGY_FACTOR, VARIOGRAM_FACTOR = 1.05, 10.0


def close(a, b, rel=1e-12):
    return np.allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rel, atol=0, equal_nan=True)


def _random(rng, B, K, H, W, spread):
    base = rng.uniform(2, 70, (B, 1, H, W))
    samples = np.zeros((B, K, 5, H, W), np.float32)
    samples[:, :, 0] = base + spread * rng.standard_normal((B, K, H, W))
    samples[:, :, 0][rng.random((B, K, H, W)) < 0.2] = 0
    samples[:, :, 4] = rng.random((B, K, H, W))
    samples[:, :, 4][rng.random((B, K, H, W)) < 0.05] = np.nan
    target = np.zeros((B, 5, H, W), np.float32)
    target[:, 0] = base[:, 0] + spread * rng.standard_normal((B, H, W))
    target[:, 0][rng.random((B, H, W)) < 0.15] = 0
    target[:, 4] = rng.random((B, H, W))
    known = (rng.random((B, 1, H, W)) < 0.3).astype(np.float32)
    return samples, target, known


@functools.lru_cache(maxsize=None)
def shuffle_case():
    """the fixed input and the oracle's sums on both ensembles, computed once and shared (tests/test_hip_coherence.py reads it too)"""
    coherent, shuffled, target, known = O.shuffle_inputs(SEED)
    return (coherent, shuffled, target, known), O.scores(coherent, target, known, LO, HI, OFFSETS), O.scores(shuffled, target, known, LO, HI, OFFSETS)


def separation(of_coherent, of_shuffled):
    """the two ratios shuffled / coherent of the means over the scans: energy_depth and variogram_total_depth"""
    return (of_shuffled["energy_depth"].mean() / of_coherent["energy_depth"].mean(),
            of_shuffled["variogram_total_depth"].mean() / of_coherent["variogram_total_depth"].mean())


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------------
def test_one_member_is_the_point_forecast():
    """At K = 1 the energy score is the RMSE of ``completion_errors`` (the depth channel; a NaN member reflectance counts as 0 here)."""
    s, t, k = _random(np.random.default_rng(0), 2, 1, 6, 40, 0.5)
    counts, dist, vario = O.scores(s, t, k, LO, HI, ((0, 1), (1, 0)))
    d, c = O.derived(counts, dist, vario), CO.derived(CO.error_sums(s[:, 0], t, k, LO, HI))
    assert close(d["energy_depth"], c["rmse_depth"]) and close(d["member_rmse_depth"][:, 0], c["rmse_depth"]) and (c["rmse_depth"] > 0).all()
    assert close(d["best_rmse_depth"], c["rmse_depth"])
    assert np.array_equal(counts, CO.error_sums(s[:, 0], t, k, LO, HI)[:, :2])
    for name in ("energy_fair_depth", "diversity_depth", "spread_skill_energy_depth"):
        assert np.isnan(d[name]).all(), name
    assert close(dist[:, 0, 0, 1], CO.error_sums(s[:, 0], t, k, LO, HI)[:, 5])


def test_identical_members():
    """K copies of one member: the energy score is that member's RMSE, the diversity 0, the variogram sums those of the one member."""
    s, t, k = _random(np.random.default_rng(1), 2, 1, 5, 24, 0.5)
    one = O.derived(*O.scores(s, t, k, LO, HI, OFFSETS[:5]))
    five = O.derived(*O.scores(np.repeat(s, 5, axis=1), t, k, LO, HI, OFFSETS[:5]))
    assert close(five["energy_depth"], one["member_rmse_depth"][:, 0]) and close(five["energy_reflectance"], one["energy_reflectance"])
    assert (five["diversity_depth"] == 0).all() and (five["spread_skill_energy_depth"] == 0).all()
    assert close(five["variogram_depth"], one["variogram_depth"], 1e-13) and np.isfinite(one["variogram_total_depth"]).all()


def test_dist_and_vario_by_hand():
    """2 x 3, K = 2, every pixel unknown but (1, 2); the target has no return at (0, 0)"""
    samples = np.zeros((1, 2, 5, 2, 3), np.float32)
    samples[0, 0, 0] = [[5, 6, 9], [2, 0, 4]]      # member 0's 0 at (1, 1): a dropped ray
    samples[0, 1, 0] = [[7, 10, 9], [2, 100, 8]]   # 100 is outside the window: 0
    target = np.zeros((1, 5, 2, 3), np.float32)
    target[0, 0] = [[0, 6, 5], [6, 9, 3]]
    known = np.zeros((1, 1, 2, 3), np.float32)
    known[0, 0, 1, 2] = 1
    counts, dist, vario = O.scores(samples, target, known, 1.0, 80.0, ((0, 1), (1, 0), (1, -1)))
    # E = (0,1) (0,2) (1,0) (1,1): member 0 = 6 9 2 0, member 1 = 10 9 2 0, target = 6 5 6 9
    assert counts.tolist() == [[5, 4]]
    assert dist[0, 0].tolist() == [[0, 16, 16 + 16 + 81], [16, 0, 16 + 16 + 16 + 81], [113, 129, 0]]
    assert (dist[0, 1] == 0).all()
    # offset (0, 1), wrapping: pairs (0,1)-(0,2), (1,0)-(1,1), (1,1)-(1,2)x, (0,2)-(0,0)x, (1,2)x -> 2 pairs
    r = math.sqrt
    a, m = [1.0, r(3)], [(r(3) + 1) / 2, (r(2) + r(2)) / 2]
    want = [2, sum((x - y) ** 2 for x, y in zip(a, m)), sum(x * x for x in a), sum(y * y for y in m)]
    assert vario[0, 0, 0, 0] == 2 and close(vario[0, 0, 0], want, 1e-14)
    # offset (1, 0), no wrap: (0,1)-(1,1) only ((0,2)-(1,2) is known, (0,0) has no return); offset (1, -1): (0,1)-(1,0), (0,2)-(1,1)
    assert vario[0, 0, 1, 0] == 1 and close(vario[0, 0, 1, 1:], [(r(3) - (r(6) + r(10)) / 2) ** 2, 3, ((r(6) + r(10)) / 2) ** 2], 1e-14)
    assert vario[0, 0, 2, 0] == 2 and close(vario[0, 0, 2, 2], 0 + 4, 1e-14)


# ---- the library's host side against it ---------------------------------------------------------------------------------------------------
def test_derived_and_aggregate_against_the_oracle():
    from r2dm_amd.completion import COHERENCE_DERIVED_NAMES, DEFAULT_OFFSETS, aggregate_coherence, derived_coherence, jsonable

    assert DEFAULT_OFFSETS == OFFSETS and len(COHERENCE_DERIVED_NAMES) == 18
    for K in (1, 2, 7):
        s, t, k = _random(np.random.default_rng(3 + K), 3, K, 6, 20, 0.5)
        k[2] = 1  # a scan with nothing to fill in
        counts, dist, vario = O.scores(s, t, k, LO, HI, OFFSETS[:6])
        got = derived_coherence(*(torch.from_numpy(a) for a in (counts, dist, vario)))
        want = O.derived(counts, dist, vario)
        assert tuple(got) == COHERENCE_DERIVED_NAMES and set(want) == set(got)
        for name in got:
            assert got[name].dtype == torch.float64 and got[name].shape == want[name].shape, name
            assert close(got[name].numpy(), want[name]), (K, name, got[name], want[name])
            assert got[name][2].isnan().all(), name
        assert got["member_rmse_depth"].shape == (3, K) and got["variogram_depth"].shape == (3, 6)
        a = aggregate_coherence(counts, dist, vario, OFFSETS[:6])
        assert set(a) == {"counts", "offsets", "sums", "micro", "macro"} and a["offsets"] == [list(o) for o in OFFSETS[:6]]
        assert a["counts"] == {"scans": 3, "members": K, "unknown": int(counts[:, 0].sum()), "evaluated": int(counts[:, 1].sum()),
                               "pairs": vario[:, 0, :, 0].sum(0).astype(int).tolist()}
        # the energy family is macro only; the variogram values come both ways
        assert set(a["macro"]) == set(COHERENCE_DERIVED_NAMES) and set(a["micro"]) == {n for n in COHERENCE_DERIVED_NAMES if n.startswith("variogram")}
        micro = O.derived(counts.sum(0), np.zeros_like(dist[0]), vario.sum(0))
        assert all(close(a["micro"][n], micro[n]) for n in a["micro"])
        with np.errstate(invalid="ignore"):
            for n in COHERENCE_DERIVED_NAMES:
                every = np.isnan(want[n][:2]).all(0)
                mean = np.where(every, np.nan, np.nanmean(np.where(every, 0.0, want[n][:2]), axis=0))
                assert close(np.asarray(a["macro"][n], np.float64), mean), (K, n, a["macro"][n], mean)
        assert close(a["sums"]["depth"], vario[:, 0, :, 1:].sum(0)) and np.shape(a["sums"]["reflectance"]) == (6, 3)
        assert "NaN" not in json.dumps(jsonable(a), allow_nan=False)
    empty = aggregate_coherence(torch.zeros(0, 2), torch.zeros(0, 2, 4, 4), torch.zeros(0, 2, 3, 4), OFFSETS[:3])
    assert empty["counts"]["scans"] == 0 and empty["counts"]["pairs"] == [0, 0, 0] and math.isnan(empty["macro"]["energy_depth"])


def test_derived_is_bitwise_invariant_under_a_permutation_of_the_members():
    from r2dm_amd.completion import derived_coherence

    for K in (2, 5, 16):
        rng = np.random.default_rng(K)
        s, t, k = _random(rng, 2, K, 6, 20, 0.5)
        counts, dist, vario = O.scores(s, t, k, LO, HI, OFFSETS[:3])
        perm = rng.permutation(K)
        rows = np.concatenate([perm, [K]])
        permuted = np.ascontiguousarray(dist[:, :, rows][:, :, :, rows])
        assert not np.array_equal(permuted, dist)
        a = derived_coherence(*(torch.from_numpy(x) for x in (counts, dist, vario)))
        b = derived_coherence(*(torch.from_numpy(x) for x in (counts, permuted, vario)))
        for name in a:
            if name.startswith("member_rmse"):
                assert a[name][:, perm].numpy().tobytes() == b[name].numpy().tobytes(), name
            else:
                assert a[name].numpy().tobytes() == b[name].numpy().tobytes(), (K, name)


def test_the_shuffle_input_separates_in_the_oracle():
    """What the per-pixel scores cannot see: the same K values at every pixel, and the oracle alone orders the two ensembles."""
    (coherent, shuffled, target, known), of_coherent, of_shuffled = shuffle_case()
    assert coherent.shape == (8, 16, 5, 8, 32) and known.shape == (8, 1, 8, 32)
    assert np.array_equal(np.sort(coherent, axis=1), np.sort(shuffled, axis=1)) and not np.array_equal(coherent, shuffled)
    energy, variogram = separation(O.derived(*of_coherent), O.derived(*of_shuffled))
    print("shuffled / coherent: energy_depth", energy, "variogram_total_depth", variogram)
    assert energy >= ENERGY_FACTOR and variogram >= VARIOGRAM_FACTOR
    assert np.array_equal(of_coherent[0], of_shuffled[0]) and (of_coherent[0][:, 1] == 6 * 32).all()
    # the truth is exchangeable with the coherent members
    assert 0.8 < O.derived(*of_coherent)["spread_skill_energy_depth"].mean() < 1.25


# ---- wiring -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_without_a_gpu():
    import r2dm_amd
    from r2dm_amd._lib import R2DMError

    s, t, k = torch.zeros(1, 3, 5, 4, 8), torch.zeros(1, 5, 4, 8), torch.zeros(1, 1, 4, 8)
    with pytest.raises(R2DMError, match="no CPU fallback"):
        r2dm_amd.ensemble_coherence(s, t, k, 1.0, 80.0)
    with pytest.raises(ValueError, match="give ensemble = K as well"):
        r2dm_amd.evaluate_completion(None, None, torch.zeros(1, 6, 4, 8), ["full"], ensemble_coherence=True)
    with pytest.raises(R2DMError, match="no CPU fallback"):
        r2dm_amd.evaluate_completion(None, None, torch.zeros(1, 6, 4, 8), ["full"], ensemble=2, ensemble_coherence=True)
    for bad in (((0, 0),), ((4, 0),), ((0, 8),), ((0, -8),), ((0.5, 1),), ((1,),), tuple((0, 1) for _ in range(17))):
        with pytest.raises(ValueError):
            r2dm_amd.completion._check_offsets(bad, 4, 8)
    assert r2dm_amd.completion._check_offsets([[3, -7], (0, 1)], 4, 8) == ((3, -7), (0, 1))


def test_parser_flags():
    import completion_eval

    p = completion_eval.build_parser()
    base = ["--ckpt", "m.pth", "--real_dir", "d"]
    plain = p.parse_args(base)
    assert not hasattr(plain, "ensemble_coherence") and not hasattr(plain, "coherence_offsets")  # the parsed arguments without it are what they were
    assert completion_eval.coherence_settings(p, plain) == {} and completion_eval.coherence_settings(p, p.parse_args(base + ["--ensemble", "4"])) == {}
    on = p.parse_args(base + ["--ensemble", "4", "--ensemble_coherence"])
    assert completion_eval.coherence_settings(p, on) == {"ensemble_coherence": True, "coherence_offsets": None}
    on = p.parse_args(base + ["--ensemble", "4", "--ensemble_coherence", "--coherence_offsets", "0,1 0,2 1,-1"])
    assert completion_eval.coherence_settings(p, on) == {"ensemble_coherence": True, "coherence_offsets": ((0, 1), (0, 2), (1, -1))}
    for bad in (["--ensemble_coherence"], ["--ensemble", "4", "--coherence_offsets", "0,1"], ["--coherence_offsets", "0,1"],
                ["--ensemble", "4", "--ensemble_coherence", "--coherence_offsets", "0;1"],
                ["--ensemble", "4", "--ensemble_coherence", "--coherence_offsets", "0,1,2"]):
        with pytest.raises(SystemExit):
            completion_eval.coherence_settings(p, p.parse_args(base + bad))


def test_header_and_signatures_declare_the_call():
    import os
    import re

    from conftest import ROOT
    from r2dm_amd import _lib

    header = open(os.path.join(ROOT, "include", "r2dm_hip.h")).read()
    for name in ("r2dm_ensemble_coherence", "r2dm_ensemble_coherence_scratch_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name
    assert len(_lib.SIGNATURES["r2dm_ensemble_coherence"][1]) == 16 and len(_lib.SIGNATURES["r2dm_ensemble_coherence_scratch_bytes"][1]) == 5


def _abi():
    from r2dm_amd import _lib

    return _lib.lib()


def _host(offsets):
    flat = [v for o in offsets for v in o]
    return (ctypes.c_int32 * max(len(flat), 1))(*flat)


def test_c_abi_refuses_bad_arguments_with_a_status():
    """Every refusal is the invalid-argument status and a message, decided before anything touches a GPU (the device pointers here are made-up
    addresses; the offsets are a real host array, which the call reads)."""
    L = _abi()
    M = 1 << 20

    def err(samples=M, target=2 * M, known=3 * M, B=2, K=4, H=4, W=16, offsets=((0, 1), (1, 0)), n=None, scratch=4 * M, counts=5 * M, dist=6 * M,
            vario=7 * M, host=True):
        arr = _host(offsets)
        return (L.r2dm_ensemble_coherence(samples, target, known, 1.0, 80.0, B, K, H, W, ctypes.cast(arr, ctypes.c_void_p) if host else None,
                                          len(offsets) if n is None else n, scratch, counts, dist, vario, None), L.r2dm_last_error().decode())

    for null in ("samples", "target", "known", "scratch", "counts"):
        rc, msg = err(**{null: None})
        assert rc == 1 and "null argument" in msg, null
    rc, msg = err(host=False)
    assert rc == 1 and "null argument" in msg
    for K in (0, -3, 65):
        rc, msg = err(K=K)
        assert rc == 1 and "members must be in [1, 64]" in msg, K
    for B in (0, -1, 65536):
        rc, msg = err(B=B)
        assert rc == 1 and "batch must be in [1, 65535]" in msg, B
    for H, W in ((0, 16), (4, 0), (-1, 16), (1 << 16, 1 << 15), (46341, 46341)):
        rc, msg = err(H=H, W=W)
        assert rc == 1 and "height * width < 2^31" in msg, (H, W)
    rc, msg = err(offsets=tuple((0, 1 + o % 8) for o in range(17)))
    assert rc == 1 and "offsets must be in [0, 16]" in msg
    rc, msg = err(n=-1)
    assert rc == 1 and "offsets must be in [0, 16]" in msg
    for bad in ((0, 0), (0, 16), (0, -16), (4, 0), (-4, 0), (1 << 30, 1)):  # (0, 0); |dw| = W; |dh| = H
        rc, msg = err(offsets=((0, 1), bad))
        assert rc == 1 and "offset 1 = " in msg and "not be (0, 0)" in msg, bad
    rc, msg = err(B=65535, K=64, H=1 << 10, W=1 << 10)
    assert rc == 1 and "2^40 elements" in msg
    for name in ("samples", "target", "known"):
        rc, msg = err(**{name: 9 * M + 4})
        assert rc == 1 and "16-byte aligned" in msg, name
        rc, msg = err(**{name: 9 * M + 2}, H=3, W=15)
        assert rc == 1 and "4-byte aligned" in msg, name
    for name in ("scratch", "counts", "dist", "vario"):
        rc, msg = err(**{name: 9 * M + 4})
        assert rc == 1 and "8-byte aligned" in msg, name


def test_scratch_bytes():
    f = _abi().r2dm_ensemble_coherence_scratch_bytes
    for empty in ((0, 4, 8, 32, 8), (65536, 4, 8, 32, 8), (2, 0, 8, 32, 8), (2, 65, 8, 32, 8), (2, 4, 0, 32, 8), (2, 4, 8, 0, 8), (2, 4, 8, 32, -1),
                  (2, 4, 8, 32, 17), (1, 1, 1 << 16, 1 << 15, 0), (65535, 64, 1 << 10, 1 << 10, 8)):  # the last: samples of more than 2^40 elements
        assert f(*empty) == 0, empty
    # one slab, one pair of tiles, two channels of 64 sums; one block of nine sums per offset (one without offsets, for the counts)
    assert f(1, 1, 1, 1, 0) == (2 * 64 + 9) * 8 and f(1, 7, 1, 1, 0) == f(1, 1, 1, 1, 0) and f(1, 1, 1, 1, 1) == f(1, 1, 1, 1, 0)
    assert f(1, 8, 1, 1, 0) == (2 * 3 * 64 + 9) * 8 and f(1, 64, 1, 1, 16) == (2 * 45 * 64 + 16 * 9) * 8
    shapes = [(1, 1), (2, 5), (8, 128), (8, 129), (64, 1024), (512, 512), (1 << 10, 1 << 12)]
    for K in (1, 8, 16, 64):
        for n in (0, 3, 16):
            sizes = [f(1, K, H, W, n) for H, W in shapes]
            assert all(s > 0 and s % 8 == 0 for s in sizes) and sizes == sorted(sizes)
            assert all(f(7, K, H, W, n) == 7 * f(1, K, H, W, n) for H, W in shapes)  # the partials of a scan depend on (H, W) alone
    assert f(1, 16, 512, 512, 8) == f(1, 16, 1 << 10, 1 << 12, 8)  # the grid is capped
    assert f(1, 16, 64, 1024, 8) == f(1, 16, 1024, 64, 8)
