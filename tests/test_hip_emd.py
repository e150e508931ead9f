"""-m gpu: the earth mover's distance (r2dm_amd/csrc/emd.hip: a forward auction per cloud pair) and what r2dm_amd/geometry.py and
geometry_eval.py build on it, against the numpy / float64 oracle of tests/emd_oracle.py on the same float32 inputs.

The kernel does not promise the minimum; it returns a permutation, its cost and a certified lower bound.  Bars (derived, not tuned):
  * ``assignment`` is a permutation of 0..n-1: exact.
  * ``emd`` within 1e-6 relative of the oracle's cost of that permutation / n: per-term fp32 error of d^2 <= 5 * 2^-24, non-negative terms
    summed in float64 (the argument of SUM_BAR in tests/test_hip_geometry.py).
  * ``lower`` within 1e-6 * (C_max + P_max) of the oracle's dual bound of the returned prices / n.
  * the guarantee ``emd - lower <= eps + rho``, ``rho = 2^-20 (C_max + P_max)``, C_max from the oracle, P_max the largest returned price:
    every compared value c + p carries the cost's rounding (<= 4 * 2^-24 C) and one addition (2^-24 (C + P)), a bid three more roundings,
    so eps-complementary slackness holds with eps + 13 * 2^-24 (C + P), rounded up to 16 * 2^-24.
  * for n <= 257 the bracket ``lower (1 - 1e-6) <= optimum <= emd (1 + 1e-6)`` against the exact O(n^3) solver; larger n rely on the
    certificate alone (O(n^2) host work).
  * a pair's numbers do not depend on the call it is in, and two calls give the same bits: ``torch.equal``.
Sizes are the smallest that cross each boundary of the kernel: one lane, one quad, one wave's stride of 64 quads (256 points), 255 / 256 quads
(1020 / 1023 points: from 256 quads on a person's objects are split over several waves when few persons bid), the block (1024 threads),
2048, and the limit of 3072 points."""
import json
import math

import numpy as np
import pytest
import torch

import emd_oracle as O
import geometry_oracle as GO
from r2dm_amd import _lib, geometry

pytestmark = pytest.mark.gpu
DEV = "cuda"
LIMIT = 3072
EMD_BAR = 1e-6
RHO = 2.0 ** -20

CASES = tuple(("gaussian", n, 0.01) for n in (1, 2, 7, 63, 64, 65, 257, 1020, 1023, 1025, 2048, LIMIT)) + \
    tuple(("rings", n, 0.01) for n in (257, 1025, 2048)) + (("clusters", 257, 1.7e-5),)


def clouds(kind, n, seed=0):
    if kind == "gaussian":
        return O.gaussian(1000 + 2 * seed + n, n), O.gaussian(1001 + 2 * seed + n, n)
    if kind == "rings":
        return O.rings(2000 + 2 * seed + n, n), O.rings(2001 + 2 * seed + n, n)
    return O.gaussian(3000 + 2 * seed + n, n, 0.05, 70.0), O.gaussian(3001 + 2 * seed + n, n, 0.05, 70.0)  # two 5 cm clusters 70 m from the origin


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def solve(a, b, **kw):
    return geometry.emd_pairs(dev(a), [0, len(a)], dev(b), [0, len(b)], return_assignment=True, return_prices=True, **kw)


def ragged(cl):
    return dev(np.concatenate(cl)), np.concatenate([[0], np.cumsum([len(c) for c in cl])]).astype(np.int64)


NAMES = ("emd", "lower", "rounds", "converged", "assignment", "prices")


def same_bits(got, k, alone, n, what):
    """entry k of a batched result against a pair's own call (row 0 of ``alone``)"""
    for name in NAMES:
        x, y = got[name][k], alone[name][0]
        if name in ("assignment", "prices"):
            rest = x[n:]
            assert (rest == -1).all() if name == "assignment" else rest.isnan().all(), (what, name)
            x, y = x[:n], y[:n]
        assert torch.equal(x, y), (what, name)


def check_pair(a, b, eps, got, what, k=0):
    n = len(a)
    C = O.cost_matrix(a, b)
    s, prices = got["assignment"][k, :n].cpu().numpy(), got["prices"][k, :n].cpu().numpy().astype(np.float64)
    emd, lower, rounds = got["emd"][k].item(), got["lower"][k].item(), got["rounds"][k].item()
    assert got["converged"][k].item() and got["assignment"].dtype == torch.int32 and got["prices"].dtype == torch.float32
    assert O.is_permutation(s, n), what
    assert (prices >= 0).all() and np.isfinite(prices).all()
    want, bound = O.cost_of(C, s) / n, O.dual_bound(C, prices) / n
    scale = C.max() + prices.max()
    print(what, "rounds", rounds, "emd", emd, "lower", lower, "gap / eps", (emd - lower) / eps, "P_max / C_max", prices.max() / max(C.max(), 1e-30),
          "emd error", abs(emd - want) / max(want, 1e-30), "lower error / scale", abs(lower - bound) / max(scale, 1e-30))
    assert abs(emd - want) <= EMD_BAR * want
    assert abs(lower - bound) <= 1e-6 * scale
    assert emd - lower <= eps + RHO * scale
    assert 1 <= rounds < (1 << 20)
    if n <= 257:
        best = O.hungarian(C)[1] / n
        print(what, "optimum", best, "emd - optimum", emd - best)
        assert lower * (1 - 1e-6) <= best <= emd * (1 + 1e-6)


# ---- (a) one pair at a time ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_pair_against_the_oracle(case):
    kind, n, eps = case
    a, b = clouds(kind, n)
    got = solve(a, b, eps=eps)
    assert all(tuple(got[k].shape) == (1,) for k in NAMES[:4]) and tuple(got["assignment"].shape) == (1, n) == tuple(got["prices"].shape)
    check_pair(a, b, eps, got, case)
    # the fourth column is not read
    a2 = a.copy()
    a2[:, 3] = np.nan
    again = solve(a2, b, eps=eps)
    same_bits(again, 0, got, n, case)


def test_the_limit_is_the_stated_one():
    assert geometry.emd_max_points() == LIMIT
    a = O.gaussian(1, LIMIT + 1)
    with pytest.raises(ValueError, match=f"1 to {LIMIT} points"):
        solve(a, a)
    with pytest.raises(ValueError, match="1 to"):
        geometry.emd_pairs(dev(a), [0, 0], dev(a), [0, 0])  # n = 0


# ---- (b) calls -----------------------------------------------------------------------------------------------------------------------------
COUNTS = (1, 2, 7, 63, 64, 65, 257, 300, 1023, 1025, 64, 5)
#          a cloud, b cloud: every cloud pair with itself, shuffled, and two cross pairs of equal size (64 and 64)
SHUFFLED = ((8, 8), (0, 0), (4, 10), (11, 11), (6, 6), (2, 2), (9, 9), (10, 4), (1, 1), (7, 7), (3, 3), (5, 5))


def test_ragged_batch_equals_the_pairs_alone_bit_for_bit():
    A = [O.gaussian(500 + k, n) if k % 3 else O.rings(500 + k, n) for k, n in enumerate(COUNTS)]
    B = [O.gaussian(600 + k, n) if k % 3 else O.rings(600 + k, n) for k, n in enumerate(COUNTS)]
    (a, oa), (b, ob) = ragged(A), ragged(B)
    got = geometry.emd_pairs(a, oa, b, ob, pairs=np.array(SHUFFLED), return_assignment=True, return_prices=True)
    assert tuple(got["assignment"].shape) == (len(SHUFFLED), max(COUNTS))
    for k, (i, j) in enumerate(SHUFFLED):
        same_bits(got, k, solve(A[i], B[j]), COUNTS[i], (k, i, j))
    for k in (1, 3, 6):  # (the others' values are pinned to calls that (a) checks in kind; three here against the oracle directly)
        i, j = SHUFFLED[k]
        check_pair(A[i], B[j], 0.01, got, ("ragged", k), k)
    again = geometry.emd_pairs(a, oa, b, ob, pairs=np.array(SHUFFLED), return_assignment=True, return_prices=True)
    for name in NAMES:
        x, y = (again[name], got[name]) if name != "prices" else (again[name].nan_to_num(-1.0), got[name].nan_to_num(-1.0))  # (NaN padding)
        assert torch.equal(x, y), name
    # pairs=None pairs cloud k with cloud k
    diag = geometry.emd_pairs(a, oa, b, ob)
    for k, (i, j) in enumerate(SHUFFLED):
        if i == j:
            assert diag["emd"][i].item() == got["emd"][k].item() and diag["lower"][i].item() == got["lower"][k].item()


def test_pairwise_matrix_and_set_metrics(monkeypatch):
    n = 257
    A = np.stack([O.rings(700 + k, n) if k % 2 else O.gaussian(700 + k, n, 12.0) for k in range(6)])
    B = np.stack([O.rings(800 + k, n) if k % 2 else O.gaussian(800 + k, n, 12.0) for k in range(5)])
    dA, dB, cA, cB = dev(A), dev(B), [n] * 6, [n] * 5
    D, gap = geometry.pairwise_emd(dA, cA, dB, cB)
    assert D.dtype == torch.float64 and tuple(D.shape) == (6, 5) == tuple(gap.shape)
    flatA, flatB = dev(A.reshape(-1, 4)), dev(B.reshape(-1, 4))
    offA, offB = np.arange(7) * n, np.arange(6) * n
    pairs = np.array([(i, j) for i in range(6) for j in range(5)])
    per = geometry.emd_pairs(flatA, offA, flatB, offB, pairs=pairs, return_assignment=True, return_prices=True)
    assert torch.equal(D.reshape(-1), per["emd"]) and torch.equal(gap.reshape(-1), per["emd"] - per["lower"])
    for k in (0, 7, 29):
        check_pair(A[pairs[k, 0]], B[pairs[k, 1]], 0.01, per, ("matrix", k), k)
    monkeypatch.setattr(geometry, "EMD_SLAB_PAIRS", 7)
    D7, gap7 = geometry.pairwise_emd(dA, cA, dB, cB)
    assert torch.equal(D7, D) and torch.equal(gap7, gap)
    # a set against itself: only i < j is solved
    Dgg, ggap = geometry.pairwise_emd(dA, cA)
    Drr, _ = geometry.pairwise_emd(dB, cB)
    assert torch.equal(Dgg, Dgg.t()) and torch.equal(ggap, ggap.t()) and (Dgg.diagonal() == 0).all() and (ggap.diagonal() == 0).all()
    upper = np.array([(i, j) for i in range(6) for j in range(i + 1, 6)])
    own = geometry.emd_pairs(flatA, offA, flatA, offA, pairs=upper)
    assert torch.equal(Dgg[upper[:, 0], upper[:, 1]], own["emd"]) and torch.equal(ggap[upper[:, 0], upper[:, 1]], own["emd"] - own["lower"])
    assert (Dgg[upper[:, 0], upper[:, 1]] > 0).all()
    monkeypatch.undo()
    # the set metrics take these matrices as they take cd_sq's
    got = geometry.set_metrics(Dgg, D, Drr)
    want = GO.set_metrics(Dgg.cpu().numpy(), D.cpu().numpy(), Drr.cpu().numpy())
    print("set metrics under EMD", got, "oracle", want)
    # (1-NNA is a count over the 11 clouds: the device's mean of 11 zeros and ones and the oracle's quotient may differ in the last bit)
    assert got["cov"] == want["cov"] and got["mmd"] == want["mmd"] and abs(got["1-nna"] - want["1-nna"]) <= 2.0 ** -52
    assert round(got["1-nna"] * 11) == round(want["1-nna"] * 11)
    with pytest.raises(ValueError, match="same number"):
        geometry.pairwise_emd(dA, [n] * 5 + [n - 1], dB, cB)
    with pytest.raises(ValueError, match="same number"):
        geometry.pairwise_emd(dA, cA, dB[:, :100].contiguous(), [100] * 5)


def test_a_permuted_copy_is_at_distance_zero():
    n, eps = 65, 0.01
    a = O.gaussian(900, n)
    perm = np.random.Generator(np.random.PCG64(901)).permutation(n)
    b = a[perm]
    C = O.cost_matrix(a, a)
    d_min = (C + np.diag(np.full(n, np.inf))).min()
    # on the oracle alone: a permutation other than the copy's moves at least two points by at least d_min each, more than the n (eps + rho)
    # that the certificate allows above the optimum 0 -- so the answer below is forced
    got = solve(a, b, eps=eps)
    bar = eps + RHO * (C.max() + got["prices"].max().item())
    print("permuted copy: d_min", d_min, "n * bar", n * bar, "lower", got["lower"].item(), "rounds", got["rounds"].item())
    assert n * bar < 2 * d_min
    assert got["emd"].item() == 0.0 and -bar <= got["lower"].item() <= 1e-9  # (two float64 sums of the same prices in different orders)
    assert np.array_equal(got["assignment"][0].cpu().numpy(), np.argsort(perm))


def near_pair():
    """one point against itself moved by 1 cm: the bounding box is 1 cm, the auction starts at eps and ends after one round"""
    a = np.array([[3.0, -2.0, 1.0, 0.0]], np.float32)
    return a, a + np.array([[0.01, 0.0, 0.0, 0.0]], np.float32)


def test_round_cap():
    a, b = clouds("gaussian", 64)
    pa, pb = near_pair()
    (x, ox), (y, oy) = ragged([a, pa]), ragged([b, pb])
    with pytest.raises(_lib.R2DMError, match=r"1 pairs \[0\] did not converge"):
        geometry.emd_pairs(x, ox, y, oy, max_rounds=3)
    got = geometry.emd_pairs(x, ox, y, oy, max_rounds=3, allow_unconverged=True, return_assignment=True, return_prices=True)
    assert got["converged"].tolist() == [False, True] and got["rounds"].tolist() == [3, 1]
    assert math.isnan(got["emd"][0].item()) and math.isnan(got["lower"][0].item())
    assert (got["assignment"][0] == -1).all() and got["prices"][0].isnan().all()
    same_bits(got, 1, solve(pa, pb), 1, "the pair beside the capped one")
    assert abs(got["emd"][1].item() - 0.01) <= 1e-6 * 0.01
    # the cap is a total over the phases, and one round more than needed changes nothing
    full = solve(a, b)
    need = int(full["rounds"].item())
    assert need > 3
    same_bits(solve(a, b, max_rounds=need), 0, full, 64, "exactly enough rounds")
    short = solve(a, b, max_rounds=need - 1, allow_unconverged=True)
    assert not short["converged"].item() and short["rounds"].item() == need - 1 and math.isnan(short["emd"].item())


def launch(A, B, pairs, eps=0.01, max_points=None):
    """the call below emd_pairs: nothing checked on the host, nothing raised for what the device refuses"""
    (a, oa), (b, ob) = ragged(A), ragged(B)
    width = max_points or max(len(c) for c in A + B)
    res = geometry._emd_launch(a, dev(oa), len(A), b, dev(ob), len(B), dev(np.asarray(pairs, np.int64)), width, eps, 1 << 20, True, True)
    out = res["out"]
    res.update(emd=out[:, 0], lower=out[:, 1], rounds=out[:, 2].long(), converged=out[:, 3] != 0)
    return res


def refused(res, k, code):
    assert res["out"][k, :2].isnan().all() and res["out"][k, 2:].tolist() == [0.0, 0.0] and res["code"][k].item() == code
    assert (res["assignment"][k] == -1).all() and res["prices"][k].isnan().all()


def test_refusals_leave_the_pair_beside_them_alone():
    a, b = clouds("clusters", 65)
    alone = solve(a, b, eps=1e-4)
    wide_a, wide_b = clouds("gaussian", 65)
    # eps below the floor of the wide pair (2^-18 of a diagonal of some 300 m is 1e-3), not of the 5 cm clusters
    res = launch([a, wide_a], [b, wide_b], [(1, 1), (0, 0)], eps=1e-4)
    assert res["status"].tolist() == [0, 0, 0, 1, 0]
    refused(res, 0, 4)
    same_bits(res, 1, alone, 65, "beside eps below the floor")
    with pytest.raises(ValueError, match=r"below 2\^-18 of the bounding-box diagonal of 1 pairs \[0\]"):
        geometry.emd_pairs(*ragged([a, wide_a]), *ragged([b, wide_b]), pairs=[(1, 1), (0, 0)], eps=1e-4)
    # unequal counts, an empty pair, a cloud above max_points
    big = O.gaussian(7, 66, 0.05, 70.0)
    res = launch([a, wide_a[:64], a[:0], big], [b, wide_b, b[:0], big], [(1, 1), (0, 0), (2, 2), (3, 3), (2, 0)], eps=1e-4, max_points=65)
    assert res["status"].tolist() == [2, 2, 0, 0, 0]
    refused(res, 0, 2), refused(res, 2, 1), refused(res, 3, 1), refused(res, 4, 2)
    same_bits(res, 1, alone, 65, "beside unequal counts")
    with pytest.raises(ValueError, match="differ in size"):
        geometry.emd_pairs(*ragged([a, wide_a[:64]]), *ragged([b, wide_b]), eps=1e-4)
    res = launch([a, wide_a], [b, wide_b], [(0, 0), (1, 1)], eps=1e-2, max_points=65)
    assert res["status"].tolist() == [0] * 5 and res["code"].tolist() == [0, 0]
    # a NaN / an infinite coordinate; the fourth column may hold anything
    for bad in (math.nan, math.inf):
        poisoned = wide_b.copy()
        poisoned[40, 1] = bad
        res = launch([a, wide_a], [b, poisoned], [(0, 0), (1, 1)], eps=1e-4)
        assert res["status"].tolist() == [0, 0, 1, 0, 0]
        refused(res, 1, 3)
        same_bits(res, 0, alone, 65, "beside a non-finite coordinate")
        with pytest.raises(ValueError, match=r"1 pairs \[1\] with a non-finite coordinate"):
            geometry.emd_pairs(*ragged([a, wide_a]), *ragged([b, poisoned]), eps=1e-2)
    # a pair index out of range, on either side
    res = launch([a, wide_a], [b, wide_b], [(2, 0), (0, 0), (0, -1), (1 << 40, 1)], eps=1e-4)
    assert res["status"].tolist() == [3, 0, 0, 0, 0]
    refused(res, 0, 1), refused(res, 2, 1), refused(res, 3, 1)
    same_bits(res, 1, alone, 65, "beside an index out of range")
    with pytest.raises(ValueError, match="an index outside"):
        geometry.emd_pairs(*ragged([a, wide_a]), *ragged([b, wide_b]), pairs=[(2, 0), (0, 0)], eps=1e-4)
    # offsets that do not check out: descending, beyond the rows
    (x, ox), (y, oy) = ragged([a, wide_a]), ragged([b, wide_b])
    for off, cloud in (([0, 130, 65], 1), ([0, 65, 131], 1), ([-1, 65, 130], 0)):
        res = geometry._emd_launch(x, dev(np.array(off, np.int64)), 2, y, dev(oy), 2, dev(np.array([(0, 0), (1, 1)], np.int64)), 65, 1e-4, 1 << 20, True, True)
        assert res["status"][0].item() >= 1 and res["code"][cloud].item() == 1 and res["out"][cloud, :2].isnan().all(), off


# ---- (c) the command line ------------------------------------------------------------------------------------------------------------------
def write_samples(folder, seed, count, H=16, W=128):
    """(5,H,W) [depth, x, y, z, reflectance] files of synthetic scans: every pixel a return between 2 and 50 m along its own ray"""
    folder.mkdir()
    g = np.random.Generator(np.random.PCG64(seed))
    el = np.deg2rad(np.linspace(3.0, -25.0, H))[:, None]
    az = np.linspace(math.pi, -math.pi, W, endpoint=False)[None, :]
    for k in range(count):
        depth = g.uniform(2.0, 50.0, (H, W)) * (0.6 + 0.4 * np.cos(az + k))
        img = np.stack([depth, depth * np.cos(el) * np.cos(az), depth * np.cos(el) * np.sin(az), depth * np.sin(el) * np.ones_like(az),
                        g.uniform(0, 1, (H, W))]).astype(np.float32)
        torch.save(torch.from_numpy(img), folder / f"samples_{k:04d}.pth")


def test_geometry_eval_end_to_end(tmp_path, capsys):
    import geometry_eval

    write_samples(tmp_path / "gen", 1, 4)
    write_samples(tmp_path / "real", 2, 4)
    common = ["--sample_dir", str(tmp_path / "gen"), "--real_dir", str(tmp_path / "real"), "--points", "256", "--limit", "4", "--num_workers", "0"]
    doc = geometry_eval.main(common + ["--distance", "emd", "--out", str(tmp_path / "emd.json")])
    assert json.load(open(tmp_path / "emd.json")) == doc
    files = [sorted((tmp_path / d).glob("*.pth")) for d in ("gen", "real")]
    (G, nG), (R, nR) = (geometry_eval.clouds_of_files(f, 256, 0, 64, 0, torch.device(DEV)) for f in files)
    assert nG.tolist() == [256] * 4 == nR.tolist()
    (Dgr, gap_gr), (Dgg, gap_gg), (Drr, gap_rr) = geometry.pairwise_emd(G, nG, R, nR), geometry.pairwise_emd(G, nG), geometry.pairwise_emd(R, nR)
    want = geometry.set_metrics(Dgg, Dgr, Drr)
    assert {k: doc[k] for k in want} == want and want == GO.set_metrics(Dgg.cpu().numpy(), Dgr.cpu().numpy(), Drr.cpu().numpy())
    assert doc["distance"] == "emd" and doc["emd_eps"] == 0.01 and doc["points"] == 256 and doc["#fake"] == 4 == doc["#real"]
    assert doc["emd_max_gap"] == max(g.max().item() for g in (gap_gr, gap_gg, gap_rr)) > 0
    # the certificate's bar, with C_max and P_max over every pair of the eight clouds
    every = torch.cat([G, R]).reshape(-1, 4)
    host = every.cpu().numpy().reshape(8, 256, 4)
    pairs = np.array([(i, j) for i in range(8) for j in range(8) if i != j])
    p_max = geometry.emd_pairs(every, np.arange(9) * 256, every, np.arange(9) * 256, pairs=pairs, return_prices=True)["prices"].max().item()
    c_max = max(O.cost_matrix(host[i], host[j]).max() for i, j in pairs)
    print("emd document", doc, "C_max", c_max, "P_max", p_max)
    assert doc["emd_max_gap"] <= 0.01 + RHO * (c_max + p_max)
    capsys.readouterr()
    # without the flag: the document of before -- its keys, and the values of the squared Chamfer distance
    doc = geometry_eval.main(common + ["--out", str(tmp_path / "cd.json")])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    Dgr, Dgg, Drr = geometry.pairwise_chamfer(G, nG, R, nR), geometry.pairwise_chamfer(G, nG, G, nG), geometry.pairwise_chamfer(R, nR, R, nR)
    want = dict(geometry.set_metrics(Dgg, Dgr, Drr))
    want.update({"#fake": 4, "#real": 4, "points": 256, "seed": 0, "distance": "cd_sq", "min_depth": 0.5, "max_depth": 63.0,
                 "directory": str(tmp_path / "gen"), "real": str(tmp_path / "real")})
    assert doc == want and list(doc) == list(want) and json.load(open(tmp_path / "cd.json")) == want
    assert line == f"COV {want['cov']:.4f}  MMD {want['mmd']:.6f}  1-NNA {want['1-nna']:.4f}  (4 generated, 4 real) -> {tmp_path / 'cd.json'}"
    # a scan with fewer points than asked for ends an EMD run (not a Chamfer run)
    with pytest.raises(SystemExit, match="4 generated and 4 real scans have fewer than --points = 4096"):
        geometry_eval.main(common[:4] + ["--points", "4096", "--limit", "4", "--num_workers", "0", "--distance", "emd"])
