"""The ensemble scores' host side, without a GPU: the numpy specification on cases worked out by hand, the identities it must satisfy, the
member seeds, the aggregation, the refusal of CPU tensors and the C ABI's argument checks.

Tolerances: counts and the rank histogram are exact.  The hand-worked values are sums of a handful of float64 terms, compared to 1e-14
relative.  The sorted-gap form of the pair term against the double loop: both are sums of at most 64 * 63 / 2 non-negative float64 terms of
widened float32 values, so each is within ~K^2 * 2^-53 of the exact value; 1e-13 relative leaves a factor of ten."""
import math

import numpy as np
import pytest
import torch

import completion_oracle as CO
import ensemble_oracle as O

LO, HI = 1.0, 80.0


def close(a, b, rel=1e-14):
    return np.allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rel, atol=0, equal_nan=True)


def _case(depths, refls, target_d, target_r, known):
    K, P = len(depths), len(target_d)
    samples = np.zeros((1, K, 5, 1, P), np.float32)
    samples[0, :, 0, 0], samples[0, :, 4, 0] = depths, refls
    target = np.zeros((1, 5, 1, P), np.float32)
    target[0, 0, 0], target[0, 4, 0] = target_d, target_r
    return samples, target, np.asarray(known, np.float32).reshape(1, 1, 1, P)


def test_the_oracle_on_hand_worked_cases():
    # K = 2: pixel 1 has a dropped member (stored 0), pixel 2 is unknown but has no real return (outside E)
    s, t, k = _case([[12, 0, 5], [9, 22, 0]], [[0.25, 0.75, 1], [0.75, 0.25, 0]], [10, 20, 0], [0.5, 0.25, 0], [0, 0, 0])
    raw, member, rank, maps = O.scores(s, t, k, LO, HI)
    assert raw[0].tolist() == [3, 2, 25, 25, 81.25, 246.5, 1.0, 1.0, 0.0625, 0.25, 0.5, 1.5, 0.5]
    assert member[0].tolist() == [[22, 3], [0.75, 0.25]] and rank[0].tolist() == [0, 2, 0]
    assert maps[0, :, 0].tolist() == [[1, 0.5, 0.5], [10.5, 22, 5], [1.5, 0, 0], [10.5, 22, 5], [9, 22, 5], [12, 22, 5], [0.5, 0.5, 0.5],
                                      [0.25, 0.25, 0.5]]
    d = O.derived(raw, member)
    assert d["crps_depth"][0] == (25 / 2 - 25 / 4) / 2 and d["crps_fair_depth"][0] == (25 / 2 - 25 / 2) / 2
    assert d["mae_depth_members"][0] == 25 / 4 and d["best_mae_depth"][0] == 1.5 and d["brier_return"][0] == 0.5 / 3
    assert d["return_recall"][0] == 0.75 and d["false_return_rate"][0] == 0.5
    assert close(d["spread_skill_depth"][0], math.sqrt(1.5 * 246.5 / 81.25)) and close(d["rmse_depth_mean"][0], math.sqrt(81.25 / 2))
    # K = 3: pixel 1 has a NaN (dropped) member and a NaN reflectance, pixel 2 is known (outside U); a depth of exactly lo does not return
    nan = math.nan
    s, t, k = _case([[8, 31, 1], [10, nan, 2], [14, 33, 3]], [[0, nan, 0], [0, 0.5, 0], [0, 1, 0]], [10, 30, 40], [0, 0.5, 0], [0, 0, 1])
    raw, member, rank, maps = O.scores(s, t, k, LO, HI)
    assert raw[0, :2].tolist() == [2, 2] and rank[0].tolist() == [0, 2, 0, 0]
    assert close(raw[0, 2:6], [40, 78, 680 / 9, 1055 / 3])
    # reflectance at pixel 1: 0 (NaN), 0.5, 1 against 0.5 -> abs 1, pairs 0.5 + 1 + 0.5, mean 0.5, variance 0.25
    assert close(raw[0, 6:10], [1, 2, 0, 0.25]) and close(raw[0, 10:], [1 / 9, 1 + 2 / 3, 0])
    assert member[0].tolist() == [[2 + 1, 0 + 30, 4 + 3], [0.5, 0, 0.5]]
    want = np.array([[1, 2 / 3, 2 / 3], [32 / 3, 32, 2.5], [math.sqrt(56 / 9), 1, 0.5], [10, 32, 2.5], [8, 31, 2], [14, 33, 3], [0, 0.5, 0],
                     [0, math.sqrt(1 / 6), 0]]).astype(np.float32)
    assert np.abs(maps[0, :, 0].view(np.int32).astype(np.int64) - want.view(np.int32)).max() <= 1
    assert math.isnan(O.derived(raw, member)["false_return_rate"][0])  # no unknown pixel without a real return


def _random(rng, B, K, P, spread):
    base = rng.uniform(2, 70, (B, 1, P))
    d = (base + spread * rng.standard_normal((B, K, P))).astype(np.float32)
    d[rng.random((B, K, P)) < 0.2] = 0
    samples = np.zeros((B, K, 5, 1, P), np.float32)
    samples[:, :, 0, 0] = d
    samples[:, :, 4, 0] = rng.random((B, K, P))
    target = np.zeros((B, 5, 1, P), np.float32)
    target[:, 0, 0] = base[:, 0] + spread * rng.standard_normal((B, P))
    target[:, 0, 0][rng.random((B, P)) < 0.15] = 0
    target[:, 4, 0] = rng.random((B, P))
    known = (rng.random((B, 1, 1, P)) < 0.3).astype(np.float32)
    return samples, target, known


def test_one_member_is_the_point_forecast():
    """At K = 1 the ensemble scores are the completion metrics: CRPS is the MAE, the expected returns are the counted ones."""
    s, t, k = _random(np.random.default_rng(0), 2, 1, 500, 0.5)
    raw, member, rank, _ = O.scores(s, t, k, LO, HI)
    d, c = O.derived(raw, member), CO.derived(CO.error_sums(s[:, 0], t, k, LO, HI))
    for mine, theirs in (("crps_depth", "mae_depth"), ("return_recall", "return_recall"), ("false_return_rate", "false_return_rate"),
                         ("rmse_depth_mean", "rmse_depth"), ("crps_reflectance", "mae_reflectance"), ("mae_depth_members", "mae_depth")):
        assert close(d[mine], c[theirs]), (mine, d[mine], c[theirs])
    assert np.isnan(d["crps_fair_depth"]).all() and (raw[:, [3, 5, 7, 9]] == 0).all()
    assert np.array_equal(raw[:, :2], CO.error_sums(s[:, 0], t, k, LO, HI)[:, :2]) and np.array_equal(rank.sum(1), raw[:, 1])


def test_identical_members_and_the_rank_histogram():
    rng = np.random.default_rng(1)
    s, t, k = _random(rng, 1, 1, 300, 0.5)
    s5 = np.repeat(s, 5, axis=1)
    r1, m1, _, _ = O.scores(s, t, k, LO, HI)
    r5, m5, rank, maps = O.scores(s5, t, k, LO, HI)
    d1, d5 = O.derived(r1, m1), O.derived(r5, m5)
    assert close(d5["crps_depth"], d1["crps_depth"]) and close(d5["crps_depth"], d5["mae_depth_members"]) and r5[0, 3] == 0 and r5[0, 5] == 0
    assert set(np.nonzero(rank[0])[0].tolist()) <= {0, 5}  # all members on one side
    assert (maps[0, 2] == 0).all() and np.array_equal(maps[0, 3], maps[0, 4])
    for K in (2, 7, 16):
        s, t, k = _random(rng, 2, K, 200, 1.0)
        raw, _, rank, _ = O.scores(s, t, k, LO, HI)
        assert np.array_equal(rank.sum(1), raw[:, 1].astype(np.int64)) and rank.shape == (2, K + 1)


@pytest.mark.parametrize("spread", [1e-3, 0.5])
def test_the_gap_form_is_the_double_loop(spread):
    rng = np.random.default_rng(2)
    for K in (1, 2, 3, 8, 9, 33, 64):
        x = (20 + spread * rng.standard_normal((K, 1024))).astype(np.float32)
        x[rng.random((K, 1024)) < 0.2] = 0
        x = x.astype(np.float64)
        a, b = O.pair_brute(x), O.pair_gaps(x)
        assert np.allclose(a, b, rtol=1e-13, atol=0) and (b >= 0).all(), K
        # CRPS at K = 1 is the absolute error exactly
        if K == 1:
            assert (a == 0).all() and (b == 0).all()


def test_member_seeds():
    from r2dm_amd.completion import member_seed, scan_seed

    assert all(member_seed(s, i, 0) == scan_seed(s, i) for s in (0, 3) for i in (0, 7, 2 ** 32 - 1))
    grid = [member_seed(s, i, k) for s in range(4) for i in range(4) for k in range(8)]
    assert len(set(grid)) == len(grid) and all(isinstance(v, int) and 0 <= v < 2 ** 63 for v in grid)
    assert member_seed(1, 2, 3) == member_seed(1, 2, 3)
    assert member_seed(1, 2, 3) == int(np.random.SeedSequence([1, 2, 3]).generate_state(1, np.uint64)[0]) >> 1  # the documented function
    torch.Generator().manual_seed(member_seed(2 ** 31 - 1, 2 ** 32 - 1, 63))  # what a generator takes
    for bad in ((-1, 0, 1), (0, 2 ** 32, 1), (0, 0, -1), (0, 0, 2 ** 32)):
        with pytest.raises(ValueError):
            member_seed(*bad)


def test_derived_and_aggregate_against_the_oracle():
    from r2dm_amd.completion import (ENSEMBLE_DERIVED_NAMES, ENSEMBLE_RAW_NAMES, aggregate_ensemble, derived_ensemble, jsonable)

    assert ENSEMBLE_RAW_NAMES == O.RAW and len(ENSEMBLE_DERIVED_NAMES) == 17
    s, t, k = _random(np.random.default_rng(3), 3, 4, 120, 0.5)
    k[2] = 1  # a scan with nothing to fill in
    raw, member, rank, _ = O.scores(s, t, k, LO, HI)
    got = derived_ensemble(torch.from_numpy(raw), torch.from_numpy(member))
    want = O.derived(raw, member)
    assert tuple(got) == ENSEMBLE_DERIVED_NAMES and set(want) == set(got)
    for name in got:
        assert got[name].dtype == torch.float64 and close(got[name].numpy(), want[name], 1e-15), name
        assert math.isnan(got[name][2])
    a = aggregate_ensemble(raw, member, rank)
    assert a["counts"] == {"scans": 3, "members": 4, "unknown": int(raw[:, 0].sum()), "evaluated": int(raw[:, 1].sum()),
                           "unknown_without_return": int(raw[:, 0].sum() - raw[:, 1].sum())}
    assert a["rank_histogram"] == rank.sum(0).tolist() and sum(a["rank_histogram"]) == a["counts"]["evaluated"]
    micro = O.derived(raw.sum(0), member.sum(0))
    assert all(close(a["micro"][n], micro[n], 1e-15) for n in ENSEMBLE_DERIVED_NAMES)
    assert all(close(a["macro"][n], np.nanmean(want[n][:2]), 1e-15) for n in ENSEMBLE_DERIVED_NAMES)
    assert close(a["sums"]["pair_depth"], raw[:, 3].sum(), 1e-15) and set(a["sums"]) == set(O.RAW[2:])
    one = aggregate_ensemble(*O.scores(s[:, :1], t, k, LO, HI)[:3])
    assert math.isnan(one["micro"]["crps_fair_depth"]) and "NaN" not in __import__("json").dumps(jsonable(one), allow_nan=False)
    assert aggregate_ensemble(torch.zeros(0, 13), torch.zeros(0, 2, 4), torch.zeros(0, 5))["counts"]["scans"] == 0


def test_cpu_tensors_raise():
    import r2dm_amd
    from r2dm_amd._lib import R2DMError

    s, t, k = torch.zeros(1, 3, 5, 4, 8), torch.zeros(1, 5, 4, 8), torch.zeros(1, 1, 4, 8)
    with pytest.raises(R2DMError, match="no CPU fallback"):
        r2dm_amd.ensemble_scores(s, t, k, 1.0, 80.0)
    with pytest.raises(R2DMError, match="no CPU fallback"):
        r2dm_amd.evaluate_completion(None, None, torch.zeros(1, 6, 4, 8), ["full"], ensemble=4)
    for bad in (0, 65, 2.0, -1):
        with pytest.raises(ValueError, match="ensemble must be"):
            r2dm_amd.evaluate_completion(None, None, torch.zeros(1, 6, 4, 8), ["full"], ensemble=bad)
    with pytest.raises(ValueError):
        r2dm_amd.ensemble_consensus(torch.zeros(1, 7, 4, 8), None)


def test_parser_flags():
    import completion_demo
    import completion_eval

    p = completion_eval.build_parser()
    assert not hasattr(p.parse_args(["--ckpt", "m.pth", "--real_dir", "d"]), "ensemble")  # the parsed arguments without it are what they were
    assert p.parse_args(["--ckpt", "m.pth", "--real_dir", "d", "--ensemble", "16"]).ensemble == 16
    p = completion_demo.parser()
    assert not hasattr(p.parse_args(["--ckpt", "m.pth", "--scan", "s.bin"]), "ensemble")  # the parsed arguments without it are what they were
    assert p.parse_args(["--ckpt", "m.pth", "--scan", "s.bin", "--ensemble", "4"]).ensemble == 4


def _abi():
    from r2dm_amd import _lib

    return _lib.lib()


def test_c_abi_refuses_bad_arguments_with_a_status():
    """Every refusal is a status and a message, decided before anything touches a GPU (the pointers here are made-up addresses)."""
    L = _abi()
    M = 1 << 20

    def err(samples=M, target=2 * M, known=3 * M, B=2, K=4, plane=64, scratch=4 * M, raw=5 * M, member=6 * M, rank=7 * M, maps=8 * M):
        return (L.r2dm_ensemble_score(samples, target, known, 1.0, 80.0, B, K, plane, scratch, raw, member, rank, maps, None),
                L.r2dm_last_error().decode())

    for null in ("samples", "target", "known", "scratch", "raw", "member", "rank"):
        rc, msg = err(**{null: None})
        assert rc == 1 and "null argument" in msg, null
    for name in ("samples", "target", "known", "maps"):
        rc, msg = err(**{name: 9 * M + 4})
        assert rc == 1 and "16-byte aligned" in msg, name
        rc, msg = err(**{name: 9 * M + 2}, plane=63)
        assert rc == 1 and "4-byte aligned" in msg, name
    for name in ("scratch", "raw", "member", "rank"):
        rc, msg = err(**{name: 9 * M + 4})
        assert rc == 1 and "8-byte aligned" in msg, name
    for B in (0, -1, 65536):
        rc, msg = err(B=B)
        assert rc == 1 and "batch must be in [1, 65535]" in msg, B
    for K in (0, -3, 65):
        rc, msg = err(K=K)
        assert rc == 1 and "members must be in [1, 64]" in msg, K
    for plane in (0, -4, (1 << 40) + 4):
        rc, msg = err(plane=plane)
        assert rc == 1 and "plane must be in [1, 2^40]" in msg, plane
    rc, msg = err(plane=1 << 40)
    assert rc == 1 and "2^40 elements" in msg
    # maps over any part of an input
    for maps in (M, M + 2 * 4 * 5 * 64 * 4 - 16, 2 * M + 64, 3 * M, M - 2 * 8 * 64 * 4 + 16):
        rc, msg = err(maps=maps)
        assert rc == 1 and "maps must not alias an input" in msg, maps


def test_scratch_bytes():
    f = _abi().r2dm_ensemble_score_scratch_bytes
    for empty in ((0, 4, 2048), (-1, 4, 2048), (2, 0, 2048), (2, 65, 2048), (2, 4, 0), (2, 4, -5), (65536, 4, 64), (2, 4, 1 << 40), (1, 1, (1 << 40) + 1)):
        assert f(*empty) == 0, empty
    assert f(1, 1, 1) == (13 + 2) * 8  # one block: thirteen sums and one member's two
    planes = [1, 3, 35, 255, 256, 257, 1025, 2080, 65536, 1 << 17, (1 << 17) + 1, 1 << 24]
    for K in (1, 8, 9, 64):
        for B in (1, 2, 7):
            sizes = [f(B, K, p) for p in planes]
            assert all(s > 0 and s % ((13 + 2 * K) * 8) == 0 for s in sizes) and sizes == sorted(sizes)
            assert all(f(B, K, p) == B * f(1, K, p) for p in planes)  # the blocks of a scan depend on the plane alone
    assert f(8, 16, 1 << 17) == f(8, 16, 1 << 24)  # the grid is capped
    assert f(1, 16, 65536) // ((13 + 32) * 8) == f(1, 3, 65536) // ((13 + 6) * 8) == 256  # ... and does not depend on K
