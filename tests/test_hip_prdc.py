"""-m gpu: r2dm_feature_knn and the k-NN manifold metrics built on it against the numpy fp64 oracle in difference form
(tests/prdc_oracle.py): values within the derived tolerance, every decision equal (the cases hold no non-firm one:
tests/test_prdc_cpu.py), exact on integer lattices with true ties, reproducible, independent of the other rows and of the launch."""
import ctypes
import json
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN, GOLDEN_RES, ROOT, synthetic_ckpt

import prdc_oracle as O

from r2dm_amd import _lib, metrics

pytestmark = pytest.mark.gpu

METRICS = ("precision", "recall", "density", "coverage")
PER_SAMPLE = ("fake_in_real", "fake_count", "real_in_fake", "real_covered")


@pytest.fixture(scope="module")
def cases():
    """per case: (real, fake, k, the oracle's manifold_metrics), computed once and left unchanged"""
    out = {}
    for name in O.CASES:
        real, fake, k = O.make_case(name)
        out[name] = (real, fake, k, O.manifold_metrics(real, fake, k))
    return out


def raw_knn(x, y=None, k=0, r2=None, want=("kth2", "min2", "argmin", "count")):
    """The C entry itself: (outputs as numpy, status, (row tiles, column splits)); does not raise on a non-zero status."""
    same = y is None
    fx = torch.as_tensor(x).cuda().contiguous()
    fy = fx if same else torch.as_tensor(y).cuda().contiguous()
    (m, d), n = fx.shape, fy.shape[0]
    rad = None if r2 is None else torch.as_tensor(r2, dtype=torch.float64).cuda()
    out = {}
    if "kth2" in want and k:
        out["kth2"] = torch.full((m,), -1.0, dtype=torch.float64, device="cuda")
    if "min2" in want:
        out["min2"] = torch.full((m,), -1.0, dtype=torch.float64, device="cuda")
    if "argmin" in want:
        out["argmin"] = torch.full((m,), -5, dtype=torch.int32, device="cuda")
    if "count" in want and rad is not None:
        out["count"] = torch.full((m,), -5, dtype=torch.int32, device="cuda")
    L = _lib.lib()
    scratch = torch.empty(L.r2dm_feature_knn_scratch_bytes(m, n, d, k) // 8 + 1, dtype=torch.float64, device="cuda")
    status = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    chosen = (ctypes.c_int32 * 2)()
    _lib.check(L.r2dm_feature_knn(fx.data_ptr(), m, fy.data_ptr(), n, d, int(same), k, _lib.ptr(rad), _lib.ptr(out.get("kth2")),
                                  _lib.ptr(out.get("min2")), _lib.ptr(out.get("argmin")), _lib.ptr(out.get("count")), scratch.data_ptr(),
                                  scratch.numel() * 8, status.data_ptr(), chosen, _lib.stream_ptr(fx.device)))
    torch.cuda.synchronize()
    return {q: v.cpu().numpy() for q, v in out.items()}, int(status.item()), (chosen[0], chosen[1])


def _within(got, want, tol, what):
    err = np.abs(got - want)
    print(f"{what}: max |gpu - oracle| / tol = {(err / tol).max():.3e}")
    assert (err <= tol).all(), (what, float((err / tol).max()))


@pytest.mark.parametrize("name", list(O.CASES))
def test_passes_and_metrics_match_the_oracle(cases, name):
    real, fake, k, want = cases[name]
    # the two same-set passes: radii (and the nearest other sample) within the tolerance
    r2 = metrics.knn_radii(real, k)
    s2 = metrics.knn_radii(fake, k)
    for x, rad, what in ((real, r2, "real"), (fake, s2, "fake")):
        got, status, _ = raw_knn(x, None, k)
        ref = O.feature_knn(x, None, k)
        assert status == 0
        _within(got["kth2"], ref["kth2"], O.tol(x, x), f"{name} {what} x {what} kth2")
        _within(got["min2"], ref["min2"], O.tol(x, x), f"{name} {what} x {what} min2")
        assert np.array_equal(got["kth2"], rad.cpu().numpy())  # (knn_radii is that pass)
        assert (got["argmin"] != np.arange(len(x))).all()
    # the two cross passes, with the library's own radii: values within the tolerance, every decision the oracle's
    for x, y, rad, rad_ref, what in ((fake, real, r2, want["real_radius2"], "fake x real"), (real, fake, s2, want["fake_radius2"], "real x fake")):
        got, status, _ = raw_knn(x, y, k, rad)
        ref = O.feature_knn(x, y, k, rad_ref)
        assert status == 0
        _within(got["kth2"], ref["kth2"], O.tol(x, y), f"{name} {what} kth2")
        _within(got["min2"], ref["min2"], O.tol(x, y), f"{name} {what} min2")
        assert np.array_equal(got["argmin"], ref["argmin"]) and np.array_equal(got["count"], ref["count"]), what
        api = metrics.feature_knn(x, y, k, rad)
        assert all(np.array_equal(api[q].cpu().numpy(), got[q]) for q in got)
    m = metrics.manifold_metrics(real, fake, k, per_sample=True)
    for q in PER_SAMPLE:
        assert np.array_equal(m[q].cpu().numpy(), want[q]), q
    _within(m["real_radius2"].cpu().numpy(), want["real_radius2"], O.tol(real, real), f"{name} real_radius2")
    _within(m["fake_radius2"].cpu().numpy(), want["fake_radius2"], O.tol(fake, fake), f"{name} fake_radius2")
    for q in METRICS:
        assert isinstance(m[q], float) and m[q] == want[q], (q, m[q], want[q])
    assert {q: m[q] for q in METRICS} == metrics.manifold_metrics(torch.from_numpy(real).cuda(), torch.from_numpy(fake).cuda(), k)


def test_lattice_is_exact_with_ties_and_the_lowest_column():
    real, fake, k = O.make_lattice()
    want = O.manifold_metrics(real, fake, k)
    for x, y, rad in ((fake, real, want["real_radius2"]), (real, fake, want["fake_radius2"])):
        got, status, _ = raw_knn(x, y, k, rad)
        ref = O.feature_knn(x, y, k, rad)
        assert status == 0
        for q in ("kth2", "min2", "argmin", "count"):
            assert np.array_equal(got[q], ref[q]), q
    m = metrics.manifold_metrics(real, fake, k, per_sample=True)
    for q in PER_SAMPLE + ("real_radius2", "fake_radius2"):
        assert np.array_equal(m[q].cpu().numpy(), want[q]), q
    assert all(m[q] == want[q] for q in METRICS)


def test_lattice_duplicates_stay_neighbours_under_same():
    x, k = O.make_lattice(duplicates=True)
    ref = O.feature_knn(x, None, k)
    radii = ref["kth2"]
    ref = O.feature_knn(x, None, k, radii)
    got, status, _ = raw_knn(x, None, k, radii)
    assert status == 0
    for q in ("kth2", "min2", "argmin", "count"):
        assert np.array_equal(got[q], ref[q]), q
    assert (got["min2"] == 0).sum() >= 8 and (got["kth2"][39:43] == 0).all()  # copies at distance exactly 0 are kept
    assert got["argmin"][40] == 39 and got["argmin"][39] == 40  # the lowest other column on a tie at 0


def test_split_case_uses_row_tiles_and_column_splits(cases):
    real, fake, k, _ = cases["split"]
    for x, y in ((real, fake), (fake, real), (real, None)):
        _, _, chosen = raw_knn(x, y, k)
        assert chosen[0] > 1 and chosen[1] > 1, chosen
    launch = metrics.feature_knn(real, fake, k, return_launch=True)["launch"]
    assert launch[0] > 1 and launch[1] > 1


def test_same_bits_on_every_call_and_for_a_prefix_of_the_rows(cases):
    for name in ("gauss", "split"):
        real, fake, k, want = cases[name]
        a, _, _ = raw_knn(fake, real, k, want["real_radius2"])
        b, _, _ = raw_knn(fake, real, k, want["real_radius2"])
        p, _, _ = raw_knn(fake[:37], real, k, want["real_radius2"])
        for q in a:
            assert np.array_equal(a[q], b[q]), (name, q)
            assert np.array_equal(a[q][:37], p[q]), (name, q)
        s, _, _ = raw_knn(real, None, k)
        s2, _, _ = raw_knn(real, None, k)
        assert all(np.array_equal(s[q], s2[q]) for q in s)


def test_rows_do_not_depend_on_the_number_of_column_splits(cases):
    """Many row tiles against 9 column tiles run in fewer splits than 1 row tile against the same columns: the same bits."""
    _, fake, k, want = cases["split"]
    g = np.random.Generator(np.random.PCG64(9))
    x = g.standard_normal((16384, fake.shape[1])).astype(np.float32)
    full, _, c_full = raw_knn(x, fake, k, want["fake_radius2"])
    part, _, c_part = raw_knn(x[:37], fake, k, want["fake_radius2"])
    assert 1 < c_full[1] < c_part[1] and c_full[0] >= 64 and c_part[0] == 1, (c_full, c_part)
    for q in full:
        assert np.array_equal(full[q][:37], part[q]), q


def test_a_non_finite_row_of_x_touches_no_other_row(cases):
    real, fake, k, want = cases["gauss"]
    clean, status, _ = raw_knn(fake, real, k, want["real_radius2"])
    assert status == 0
    for bad in (np.nan, np.inf):
        dirty = fake.copy()
        dirty[41, 7] = bad
        got, status, _ = raw_knn(dirty, real, k, want["real_radius2"])
        assert status == 1
        keep = np.arange(len(fake)) != 41
        for q in clean:
            assert np.array_equal(got[q][keep], clean[q][keep]), q


def test_a_non_finite_row_of_y_is_counted_and_the_wrapper_raises(cases):
    real, fake, k, want = cases["gauss"]
    dirty = real.copy()
    dirty[3, 0] = np.nan
    dirty[100, 19] = -np.inf
    _, status, _ = raw_knn(fake, dirty, k, want["real_radius2"])
    assert status == 2
    _, status, _ = raw_knn(dirty, None, k)  # (the same set: its rows are counted once)
    assert status == 2
    with pytest.raises(_lib.R2DMError, match="non-finite"):
        metrics.feature_knn(fake, dirty, k)
    with pytest.raises(_lib.R2DMError, match="non-finite"):
        metrics.manifold_metrics(dirty, fake, k)
    with pytest.raises(_lib.R2DMError, match="fewer than k"):
        metrics.knn_radii(fake[:3], 3)
    radius = want["real_radius2"].copy()
    radius[:] = np.nan  # a NaN radius never counts
    got, status, _ = raw_knn(fake, real, 0, radius)
    assert status == 0 and (got["count"] == 0).all()


def test_evaluate_prdc_k_end_to_end(tmp_path):
    """evaluate.py --prdc_k 3 on synthetic sample directories and PointNet weights: the new keys are present, finite and equal to
    manifold_metrics on the same features; without the flag the key set is the one from before."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, GOLDEN)
    import evaluate
    import make_golden_pointnet as G

    from r2dm_amd import pointnet, synthetic

    state = synthetic.synthetic_pointnet_state(G.STATE_SEED)
    ckpt, weights = tmp_path / "synthetic.pth", tmp_path / "cls_model.pth"
    torch.save(synthetic_ckpt(resolution=GOLDEN_RES), ckpt)
    torch.save(state, weights)
    gen, real = tmp_path / "gen", tmp_path / "real"
    imgs = torch.from_numpy(np.concatenate([G.images(seed) for seed in (41, 42, 43, 44, 45)]))[:13]
    for out, part in ((gen, imgs[:6]), (real, imgs[6:])):
        out.mkdir()
        for i, img in enumerate(part):
            torch.save(img.clone(), out / f"samples_{i:04d}.pth")
    args = Namespace(ckpt=ckpt, sample_dir=str(gen), dataset="test", batch_size=4, num_workers=0, real_set=None, real_dir=str(real),
                     real_scans=None, pointnet_weights=str(weights), mmd_seed=7, prdc_k=3)
    r = json.loads(open(evaluate.evaluate(args)).read())
    extractor = pointnet.pretrained_pointnet(state, device="cuda")
    f_gen, f_real = pointnet.pointnet_features(extractor, imgs[:6].cuda()), pointnet.pointnet_features(extractor, imgs[6:].cuda())
    import random

    perm = list(range(7))
    random.Random(0).shuffle(perm)
    want = metrics.manifold_metrics(f_real[perm], f_gen, k=3)
    assert set(r["pts"]) == {"frechet_distance", "squared_mmd", *METRICS} and r["img"] == {}
    assert all(np.isfinite(r["pts"][q]) and r["pts"][q] == want[q] for q in METRICS)
    assert r["info"]["prdc_k"] == 3 and r["info"]["prdc_#real"] == 7
    # without the flag (and with a Namespace that does not have it): the document of before, key for key
    for plain in (Namespace(**{**vars(args), "prdc_k": None}), Namespace(**{q: v for q, v in vars(args).items() if q != "prdc_k"})):
        plain.sample_dir = args.sample_dir + "_again"
        os.rename(args.sample_dir, plain.sample_dir)
        q = json.loads(open(evaluate.evaluate(plain)).read())
        os.rename(plain.sample_dir, args.sample_dir)
        assert set(q["pts"]) == {"frechet_distance", "squared_mmd"} and q["img"] == {} and q["bev"] == r["bev"]
        assert set(q["info"]) == set(r["info"]) - {"prdc_k", "prdc_#real"}
        assert q["pts"]["frechet_distance"] == r["pts"]["frechet_distance"] and q["pts"]["squared_mmd"] == r["pts"]["squared_mmd"]
    # the parser has the option, absent by default
    assert evaluate.build_parser().parse_args(["--ckpt", "c", "--sample_dir", "d"]).prdc_k is None
    assert evaluate.build_parser().parse_args(["--ckpt", "c", "--sample_dir", "d", "--prdc_k", "3"]).prdc_k == 3
