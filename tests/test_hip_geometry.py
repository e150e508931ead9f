"""-m gpu: the nearest-neighbour search (r2dm_amd/csrc/geometry.hip), what r2dm_amd/geometry.py builds on it and
``evaluate_completion(chamfer=True)``, against the numpy / float64 brute force of tests/geometry_oracle.py on the same float32 inputs.

Tolerances (stated, derived from the number formats, not from the code under test):
  * per-point d^2: relative 8 * 2^-24 of the oracle.  The kernel evaluates (ax-bx)^2 + (ay-by)^2 + (az-bz)^2 in fp32: three rounded
    differences, then squares and sums with or without FMA contraction -- each term carries at most (1 + 2^-24)^3 and each of the two
    additions one more rounding, all terms non-negative: below 5 * 2^-24.  The oracle's own float64 error is 2^-29 times smaller.
  * per-point index: EQUAL to the oracle's.  Asserted first, on the oracle alone: the relative gap between best and second-best d^2 of
    every query exceeds 4e-6, an order above what two values each within 5 * 2^-24 = 3e-7 can close, so a wrong index is the kernel's.
  * sums of d^2 and d: relative 1e-6 (per-term error <= 3e-7 on non-negative terms; the float64 summation adds n * 2^-53).
  * counts of d <= tau: exact; tau is chosen so that no oracle distance lies within 1e-6 relative of it (asserted first).
  * one pair's numbers do not depend on the call it is in, and two calls give the same bits: ``torch.equal``.
"""
import math
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, GOLDEN_RES, synthetic_ckpt

sys.path.insert(0, GOLDEN)
import make_golden_projection as MG  # noqa: E402  (read-only: the integer-only generator of the free cloud)

import geometry_oracle as O  # noqa: E402
import r2dm_amd  # noqa: E402
from r2dm_amd import completion, geometry  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
D2_BAR = 8 * 2.0 ** -24
GAP_BAR = 4e-6
SUM_BAR = 1e-6
#        seed |A|  |B|  scale offset
CASES = ((0, 257, 1000, 30.0, 0.0), (1, 1000, 257, 30.0, 0.0), (2, 65, 64, 30.0, 0.0), (3, 1025, 1023, 30.0, 0.0), (5, 2049, 2047, 30.0, 0.0),
         (4, 513, 511, 0.05, 70.0))  # the last: two 5 cm clusters 70 m from the origin, where |a|^2 + |b|^2 - 2ab errs by several times the distance itself


def clouds(seed, na, nb, scale, offset):
    g = np.random.Generator(np.random.PCG64(seed))
    a = (g.standard_normal((na, 4)) * scale + offset).astype(np.float32)
    b = (g.standard_normal((nb, 4)) * scale + offset).astype(np.float32)
    return a, b


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def search_pair(a, b, **kw):
    return geometry.nearest_neighbors(dev(a), [0, len(a)], dev(b), [0, len(b)], return_index=True, **kw)


def check_per_point(a, b, got_d2, got_idx, what):
    want_d2, want_idx = O.nearest(a, b)
    got_d2, got_idx = got_d2.cpu().numpy().astype(np.float64), got_idx.cpu().numpy()
    assert got_d2.shape == want_d2.shape and got_idx.dtype == np.int32
    if len(b) == 0:
        assert np.isposinf(got_d2).all() and (got_idx == -1).all(), what
        return
    rel = np.abs(got_d2 - want_d2) / want_d2
    print(what, "max relative error of d^2", rel.max() if rel.size else 0.0, "wrong indices", int((got_idx != want_idx).sum()))
    assert (rel <= D2_BAR).all(), (what, rel.max())
    assert np.array_equal(got_idx, want_idx), (what, np.flatnonzero(got_idx != want_idx)[:8])


def check_sums(got, want, what):
    """(8,) raw values: counts exact, sums within SUM_BAR, infinities and zeros exact"""
    print(what, "got", got.tolist(), "want", want.tolist())
    assert np.array_equal(got[[2, 5, 6, 7]], want[[2, 5, 6, 7]]), what
    for k in (0, 1, 3, 4):
        if want[k] == 0 or math.isinf(want[k]):
            assert got[k] == want[k], (what, k)
        else:
            assert abs(got[k] - want[k]) <= SUM_BAR * want[k], (what, k, got[k], want[k])


def tau_clear_of(distances, start):
    """the first of start, start * 1.01, ... that no distance lies within 1e-6 relative of"""
    tau = start
    while (np.abs(distances - tau) <= 1e-6 * tau).any():
        tau *= 1.01
    return tau


# ---- (a) the per-point search ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"seed{c[0]}-{c[1]}x{c[2]}")
def test_per_point_search_against_the_float64_oracle(case):
    a, b = clouds(*case)
    gap = min(O.second_best_gap(a, b), O.second_best_gap(b, a))
    print(case, "smallest relative gap between best and second best", gap)
    assert gap > GAP_BAR  # (on the oracle: a wrong index below is the kernel's)
    out = search_pair(a, b)
    assert out["start_ab"].tolist() == [0, len(a)] and out["start_ba"].tolist() == [0, len(b)]
    check_per_point(a, b, out["d2_ab"], out["idx_ab"], (case, "a->b"))
    check_per_point(b, a, out["d2_ba"], out["idx_ba"], (case, "b->a"))
    dab, dba = np.sqrt(O.nearest(a, b)[0]), np.sqrt(O.nearest(b, a)[0])
    tau = tau_clear_of(np.concatenate([dab, dba]), float(np.median(dab)))
    assert not (np.abs(np.concatenate([dab, dba]) - tau) <= 1e-6 * tau).any()
    check_sums(geometry.chamfer_sums(dev(a), [0, len(a)], dev(b), [0, len(b)], tau=tau)[0].cpu().numpy(), O.raw_sums(a, b, tau), case)
    # the fourth column is not read
    a2 = a.copy()
    a2[:, 3] = np.nan
    assert torch.equal(search_pair(a2, b)["d2_ab"], out["d2_ab"])


def test_many_chunks_of_query_points():
    """70 000 points against 33: 69 blocks of queries one way, one tile streamed by 1 block the other way (same bars)"""
    a, b = clouds(11, 70_000, 33, 30.0, 0.0)
    assert min(O.second_best_gap(a, b), O.second_best_gap(b, a)) > GAP_BAR
    out = search_pair(a, b)
    check_per_point(a, b, out["d2_ab"], out["idx_ab"], "70000->33")
    check_per_point(b, a, out["d2_ba"], out["idx_ba"], "33->70000")
    check_sums(out["sums"][0].cpu().numpy(), O.raw_sums(a, b, 0.2), "70000x33")


# ---- (b) a ragged batch ------------------------------------------------------------------------------------------------------------------
COUNTS_A, COUNTS_B = (0, 1, 64, 257, 1000), (3, 0, 65, 256, 999)
SHUFFLED = ((3, 2), (0, 4), (4, 4), (2, 0), (1, 1), (4, 3), (1, 0))


def ragged():
    g = np.random.Generator(np.random.PCG64(21))
    A = [(g.standard_normal((n, 4)) * 30).astype(np.float32) for n in COUNTS_A]
    B = [(g.standard_normal((n, 4)) * 30).astype(np.float32) for n in COUNTS_B]
    return A, B, np.concatenate([[0], np.cumsum(COUNTS_A)]), np.concatenate([[0], np.cumsum(COUNTS_B)])


@pytest.mark.parametrize("pairs", (None, SHUFFLED), ids=("default", "shuffled"))
def test_ragged_batch(pairs):
    A, B, offa, offb = ragged()
    plist = [(k, k) for k in range(5)] if pairs is None else list(pairs)
    finite = np.concatenate([np.sqrt(O.nearest(x, y)[0]) for i, j in plist for x, y in ((A[i], B[j]), (B[j], A[i])) if len(x) and len(y)])
    tau = tau_clear_of(finite, 8.0)
    assert not (np.abs(finite - tau) <= 1e-6 * tau).any() and (finite <= tau).any() and (finite > tau).any()
    pa, pb = dev(np.concatenate(A)), dev(np.concatenate(B))
    out = geometry.nearest_neighbors(pa, offa, pb, torch.from_numpy(offb), pairs=None if pairs is None else torch.tensor(pairs),
                                     return_index=True, tau=tau)
    sums = out["sums"].cpu().numpy()
    assert sums.shape == (len(plist), 8) and out["start_ab"][-1] == sum(COUNTS_A[i] for i, _ in plist)
    for p, (i, j) in enumerate(plist):
        sab, sba = out["start_ab"], out["start_ba"]
        check_per_point(A[i], B[j], out["d2_ab"][sab[p]:sab[p + 1]], out["idx_ab"][sab[p]:sab[p + 1]], (p, i, j, "a->b"))
        check_per_point(B[j], A[i], out["d2_ba"][sba[p]:sba[p + 1]], out["idx_ba"][sba[p]:sba[p + 1]], (p, i, j, "b->a"))
        check_sums(sums[p], O.raw_sums(A[i], B[j], tau), (p, i, j))
        # the pair alone in a call: the same bits
        one = geometry.nearest_neighbors(pa, offa, pb, offb, pairs=[[i, j]], return_index=True, tau=tau)
        assert torch.equal(one["sums"][0], out["sums"][p]), (p, i, j)
        assert torch.equal(one["d2_ab"], out["d2_ab"][sab[p]:sab[p + 1]]) and torch.equal(one["idx_ba"], out["idx_ba"][sba[p]:sba[p + 1]])
    # the empty-cloud rules, spelled out: (empty a, 3 points) and (1 point, empty b)
    e0 = sums[plist.index((0, 4)) if pairs is not None else 0]
    assert e0[:3].tolist() == [0.0, 0.0, 0.0] and math.isinf(e0[3]) and math.isinf(e0[4]) and e0[5] == 0 and e0[6] == 0
    e1 = sums[plist.index((1, 1))]
    assert math.isinf(e1[0]) and math.isinf(e1[1]) and e1[2] == 0 and e1[3:6].tolist() == [0.0, 0.0, 0.0] and e1[6:].tolist() == [1.0, 0.0]
    derived = geometry.chamfer_from_sums(out["sums"])
    for p, (i, j) in enumerate(plist):
        want = O.chamfer(A[i], B[j], tau)
        for name in geometry.DERIVED_NAMES:
            got = derived[name][p].item()
            assert (math.isnan(got) and math.isnan(want[name])) or abs(got - want[name]) <= SUM_BAR * abs(want[name]), (p, name, got, want[name])
    assert geometry.chamfer_sums(pa, offa, pb, offb, pairs=np.zeros((0, 2), np.int64)).shape == (0, 8)


# ---- (c) exact ties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ("interleaved", "appended"))
def test_exact_ties_go_to_the_lowest_index(layout):
    a, base = clouds(31, 300, 700, 30.0, 0.0)
    b = np.repeat(base, 2, axis=0) if layout == "interleaved" else np.concatenate([base, base])  # 1400 points: the copies span two tiles
    out = search_pair(a, b)
    idx = out["idx_ab"].cpu().numpy()
    want = O.nearest(a, base)[1]
    assert np.array_equal(idx, 2 * want if layout == "interleaved" else want)
    assert np.array_equal(idx, O.nearest(a, b)[1])  # (numpy's argmin: the first occurrence)
    back = out["idx_ba"].cpu().numpy()
    assert np.array_equal(back, O.nearest(b, a)[1]) and np.array_equal(back[0::2], back[1::2]) == (layout == "interleaved")


# ---- (d) determinism ---------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    A, B, offa, offb = ragged()
    pa, pb = dev(np.concatenate(A)), dev(np.concatenate(B))
    one = geometry.nearest_neighbors(pa, offa, pb, offb, pairs=SHUFFLED, return_index=True)
    two = geometry.nearest_neighbors(pa, offa, pb, offb, pairs=SHUFFLED, return_index=True)
    for name in ("d2_ab", "d2_ba", "idx_ab", "idx_ba", "sums"):
        assert torch.equal(one[name], two[name]), name
    assert torch.equal(geometry.chamfer_sums(pa, offa, pb, offb, pairs=SHUFFLED), one["sums"])  # with and without the per-point outputs


# ---- (e) the pairwise matrix -------------------------------------------------------------------------------------------------------------
def test_pairwise_matrix_and_set_metrics(monkeypatch):
    n = 300
    nA, nB = (300, 299, 150, 1, 257, 64), (300, 255, 65, 300, 2)
    g = np.random.Generator(np.random.PCG64(41))
    A = (g.standard_normal((6, n, 4)) * np.linspace(1.0, 2.0, 6)[:, None, None]).astype(np.float32)
    B = (g.standard_normal((5, n, 4)) * np.linspace(1.2, 2.4, 5)[:, None, None]).astype(np.float32)
    A[:, :, 3] = 7.0
    for k, c in enumerate(nA):
        A[k, c:] = 1e6  # rows past the count must not be read as points
    for k, c in enumerate(nB):
        B[k, c:] = -1e6
    la, lb = [A[k, :c] for k, c in enumerate(nA)], [B[k, :c] for k, c in enumerate(nB)]
    dA, dB, cA, cB = dev(A), dev(B), torch.tensor(nA, device=DEV), torch.tensor(nB)
    D = geometry.pairwise_chamfer(dA, cA, dB, cB)
    want = O.chamfer_matrix(la, lb)
    assert D.shape == (6, 5) and D.dtype == torch.float64 and D.is_cuda
    rel = np.abs(D.cpu().numpy() - want) / want
    print("pairwise cd_sq: max relative error", rel.max())
    assert (rel <= SUM_BAR).all()
    # the per-pair path: the same bits
    pa, offa = dev(np.concatenate(la)), np.concatenate([[0], np.cumsum(nA)])
    pb, offb = dev(np.concatenate(lb)), np.concatenate([[0], np.cumsum(nB)])
    pairs = [(i, j) for i in range(6) for j in range(5)]
    per_pair = geometry.chamfer_from_sums(geometry.chamfer_sums(pa, offa, pb, offb, pairs=pairs))["cd_sq"].reshape(6, 5)
    assert torch.equal(per_pair, D)
    assert torch.equal(geometry.chamfer_from_sums(geometry.chamfer_sums(pa, offa, pb, offb, pairs=[(4, 2)]))["cd_sq"][0], D[4, 2])
    # in slabs of a few pairs: the same bits again
    monkeypatch.setattr(geometry, "SLAB_BYTES", 7 * (16 + 64 + 64))
    assert torch.equal(geometry.pairwise_chamfer(dA, cA, dB, cB), D)
    monkeypatch.undo()
    # the set metrics
    Dgg, Drr = geometry.pairwise_chamfer(dA, cA, dA, cA), geometry.pairwise_chamfer(dB, cB, dB, cB)
    assert (Dgg.diagonal() == 0).all() and (Drr.diagonal() == 0).all()
    got = geometry.set_metrics(Dgg, D, Drr)
    assert got == O.set_metrics(Dgg.cpu().numpy(), D.cpu().numpy(), Drr.cpu().numpy())  # the oracle's definitions on the same matrices: exact
    ref = O.set_metrics(O.chamfer_matrix(la, la), want, O.chamfer_matrix(lb, lb))       # ... and on the oracle's own matrices
    print("set metrics", got, "oracle", ref)
    assert got["cov"] == ref["cov"] and got["1-nna"] == ref["1-nna"] and abs(got["mmd"] - ref["mmd"]) <= SUM_BAR * ref["mmd"]


# ---- (f) non-finite input ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", (math.nan, math.inf))
def test_a_non_finite_coordinate_raises(value):
    a, b = clouds(51, 100, 120, 30.0, 0.0)
    for which, row, col in (("a", 17, 0), ("b", 119, 2)):
        x, y = a.copy(), b.copy()
        (x if which == "a" else y)[row, col] = value
        with pytest.raises(ValueError, match="non-finite"):
            geometry.chamfer_sums(dev(x), [0, 100], dev(y), [0, 120])
    with pytest.raises(ValueError, match="non-finite"):
        x = np.stack([a, a])
        x[1, 5, 1] = value
        geometry.pairwise_chamfer(dev(x), [100, 100], dev(b[None]), [120])


# ---- (g) evaluate_completion(chamfer=True) -----------------------------------------------------------------------------------------------
def cloud_of_image(img, lo, hi, keep=None):
    """the oracle's reading of a (5,H,W) image: the pixels with lo < depth < hi (and keep), in image order, as [x, y, z] rows"""
    m = (img[0] > lo) & (img[0] < hi)
    if keep is not None:
        m &= keep
    return img[1:4][:, m].T.astype(np.float32)


def test_evaluate_completion_with_chamfer():
    H, W = GOLDEN_RES
    ddpm, lidar, cfg = r2dm_amd.setup_model(synthetic_ckpt(resolution=GOLDEN_RES), device=DEV, show_info=False, max_batch=2)
    pts = MG.make_cloud("free_64x1024")
    scans = [np.ascontiguousarray(pts[0:25000]), np.ascontiguousarray(pts[30000:52000])]
    unfolding, width = r2dm_amd.parse_projection(cfg.data.projection)
    flat = np.concatenate(scans)
    off = np.array([0, len(scans[0]), len(scans[0]) + len(scans[1])], np.int64)
    planes = torch.nn.functional.interpolate(
        r2dm_amd.project_scans(flat, off, H=64, W=width, scan_unfolding=unfolding, min_depth=lidar.min_depth, max_depth=lidar.max_depth, device=DEV),
        size=(H, W), mode="nearest-exact")
    kw = dict(methods=("target", "nearest"), seed=5, batch_size=2, keep=True)
    plain, _ = completion.evaluate_completion(ddpm, lidar, planes, ["beams:2"], **kw)
    res, kept = completion.evaluate_completion(ddpm, lidar, planes, ["beams:2"], chamfer=True, fscore_threshold=0.3, **kw)
    # off: today's dict; on: the same entries plus "geometry"
    assert all("geometry" not in e for e in plain["beams:2"].values())
    for method, e in res["beams:2"].items():
        assert set(e) == set(plain["beams:2"][method]) | {"geometry"} and set(e["geometry"]) == {"all", "inpainted"}
        assert completion.jsonable({k: v for k, v in e.items() if k != "geometry"}) == completion.jsonable(plain["beams:2"][method])
        for where in ("all", "inpainted"):
            g = e["geometry"][where]
            assert set(g) == {"scans", "empty", "micro", "macro"} and (g["scans"], g["empty"]) == (2, 0)
            assert set(g["micro"]) == set(g["macro"]) == set(geometry.DERIVED_NAMES)
    # the target's own planes as the prediction: distance exactly 0, every point within the threshold
    for where in ("all", "inpainted"):
        for avg in ("micro", "macro"):
            t = res["beams:2"]["target"]["geometry"][where][avg]
            assert t["cd"] == 0.0 and t["cd_sq"] == 0.0 and t["fscore"] == 1.0 and t["precision"] == 1.0 and t["recall"] == 1.0
    # nearest-beam interpolation: every number from the oracle on the kept tensors
    k = kept["beams:2"]
    lo, hi = float(lidar.min_depth), float(lidar.max_depth)
    pred, target, mask = k["pred"]["nearest"].numpy(), k["target"].numpy(), k["mask"].numpy()
    assert set(k["geometry_raw"]) == {"target", "nearest"}
    for where in ("all", "inpainted"):
        raw = k["geometry_raw"]["nearest"][where]
        assert raw.shape == (2, 8) and raw.dtype == torch.float64
        per_scan = []
        for i in range(2):
            keep = None if where == "all" else mask[i, 0] == 0
            x, y = cloud_of_image(pred[i], lo, hi, keep), cloud_of_image(target[i], lo, hi, keep)
            assert len(x) > 50 and len(y) > 50
            d = np.concatenate([np.sqrt(O.nearest(x, y)[0]), np.sqrt(O.nearest(y, x)[0])])
            assert not (np.abs(d - 0.3) <= 1e-6 * 0.3).any()
            check_sums(raw[i].numpy(), O.raw_sums(x, y, 0.3), (where, i))
            per_scan.append(O.chamfer(x, y, 0.3))
        g = res["beams:2"]["nearest"]["geometry"][where]
        for name in geometry.DERIVED_NAMES:
            macro = float(np.mean([s[name] for s in per_scan]))
            assert abs(g["macro"][name] - macro) <= SUM_BAR * abs(macro), (where, name)
        micro = geometry.chamfer_from_sums(raw.sum(0))
        assert all(g["micro"][name] == micro[name].item() for name in geometry.DERIVED_NAMES)
    inp = res["beams:2"]["nearest"]["geometry"]["inpainted"]["micro"]
    assert inp["cd"] > 0 and res["beams:2"]["nearest"]["geometry"]["all"]["micro"]["cd"] > 0
