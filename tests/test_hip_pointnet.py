"""-m gpu: the FPD on the GPU -- the fused PointNet extractor (r2dm_amd.pointnet, pointnet.hip) against the reference's recorded
features and fp64 oracles, and the distribution metrics of feature sets (r2dm_amd.metrics) against the reference's values
(tests/golden/pointnet.npz, tests/golden/make_golden_pointnet.py)."""
import json
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN, GOLDEN_RES, ROOT, rnd, synthetic_ckpt

sys.path.insert(0, GOLDEN)
import make_golden_pointnet as G  # noqa: E402  (the fixture's integer-only input generators)
import pointnet_oracle as O  # noqa: E402

from r2dm_amd import _lib, metrics, pointnet, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

STORED = [c[0] for c in G.CLOUD_CASES] + ["images"]


@pytest.fixture(scope="module")
def data():
    with np.load(os.path.join(GOLDEN, "pointnet.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def state():
    return synthetic.synthetic_pointnet_state(G.STATE_SEED)


@pytest.fixture(scope="module")
def extractor(state):
    return pointnet.pretrained_pointnet(state, device="cuda")


def _clouds(data, name):
    x = torch.from_numpy(data[f"x_{name}"])
    return O.sample_clouds(x) if name == "images" else x


def _check(name, got, want64, err):
    """rms <= 2x and max <= 4x the reference's own error against fp64 on the same inputs (the ratios of tests/test_hip_configs.py)"""
    d = got.double().cpu() - want64.double().cpu()
    rms, mx = d.pow(2).mean().sqrt().item(), d.abs().max().item()
    print(f"{name}: |hip - fp64| rms {rms:.3e} max {mx:.3e}; reference's own rms {err[0]:.3e} max {err[1]:.3e} "
          f"(ratios {rms / err[0]:.2f}, {mx / err[1]:.2f})")
    assert got.dtype == torch.float32 and got.is_cuda and torch.isfinite(got).all()
    assert rms <= 2 * err[0] and mx <= 4 * err[1]


@pytest.mark.parametrize("name", STORED)
def test_features_against_the_references_fp64(data, extractor, name):
    x = _clouds(data, name).cuda()
    got, trans = extractor.extract(x, 2, x.shape[2], return_trans=True)
    assert got.shape == (x.shape[0], 1808)
    _check(name, got, torch.from_numpy(data[f"f64_{name}"]), data[f"err_{name}"])
    assert (trans.double().cpu() - torch.from_numpy(data[f"trans_{name}"])).abs().max().item() < 1e-5
    assert torch.equal(extractor(x), got)  # the callable is the same path; the same bits on a second call
    # the reference's fp32 run is as far from fp64 as recorded, and this one is near it
    assert (got.cpu() - torch.from_numpy(data[f"f32_{name}"])).abs().max().item() <= 5 * data[f"err_{name}"][1]


def test_features_more_clouds_than_lanes(data, state, extractor):
    (name, seed, B, N), = [c for c in G.REGEN_CASES if c[0] == "b65"]
    x = torch.from_numpy(G.cloud(seed, B, N))
    want = O.features(state, x.double())
    got = extractor(x.cuda())
    assert got.shape == (65, 1808)
    _check(name, got, want, data[f"err_{name}"])
    # every cloud on its own: the batch does not mix clouds
    assert torch.equal(extractor(x[17:18].cuda()), got[17:18]) and torch.equal(extractor(x[64:].cuda()), got[64:])


def test_features_full_size_cloud(data, state, extractor):
    (name, seed, B, N), = [c for c in G.REGEN_CASES if c[0] == "full"]
    x = torch.from_numpy(G.cloud(seed, B, N)).cuda()
    want = O.features({k: v.cuda() for k, v in state.items()}, x.double())  # (the fp64 oracle, torch ops on the device)
    got = extractor(x)
    _check(name, got, want, data[f"err_{name}"])
    assert torch.equal(extractor(x), got)


def test_features_do_not_depend_on_the_order_of_the_points(data, extractor):
    x = _clouds(data, "n4097").cuda()
    got = extractor(x)
    perm = torch.from_numpy(np.random.Generator(np.random.PCG64(3)).permutation(x.shape[2])).cuda()
    assert torch.equal(extractor(x[:, :, perm].contiguous()), got)
    # a padded lane of the last tile is no point: appending a copy of an existing point changes nothing, appending (0,0,0) may
    more = torch.cat([x, x[:, :, :1]], dim=2).contiguous()
    assert torch.equal(extractor(more), got)


def test_sample_layout_equals_the_cloud_layout(data, extractor):
    img = torch.from_numpy(data["x_images"])
    clouds = O.sample_clouds(img)  # (B,3,HW) fp32: masked, divided by 80
    a = pointnet.pointnet_features(extractor, img.cuda())
    b = pointnet.pointnet_features(extractor, clouds.transpose(1, 2).contiguous().cuda())
    c = extractor(clouds.cuda())
    assert a.shape == (3, 1808) and torch.equal(a, b) and torch.equal(a, c)
    _check("images (sample layout)", a, torch.from_numpy(data["f64_images"]), data["err_images"])


def test_shapes_and_error_paths(state, extractor):
    assert extractor(torch.zeros(0, 3, 5, device="cuda")).shape == (0, 1808)
    assert pointnet.pointnet_features(extractor, torch.zeros(0, 5, 16, 128, device="cuda")).shape == (0, 1808)
    with pytest.raises(ValueError, match="at least one point"):
        extractor(torch.zeros(2, 3, 0, device="cuda"))
    with pytest.raises(ValueError, match="expected"):
        pointnet.pointnet_features(extractor, torch.zeros(2, 4, 16, 128, device="cuda"))
    x = torch.from_numpy(G.cloud(5, 2, 300))
    good = extractor(x.cuda())
    for bad in (float("inf"), float("-inf"), float("nan")):
        y = x.clone()
        y[1, 2, 150] = bad
        with pytest.raises(RuntimeError, match="non-finite coordinate"):
            extractor(y.cuda())
    assert torch.equal(extractor(x.cuda()), good)  # the flag does not stick
    big = dict(state)
    big["feat.conv1.weight"] = state["feat.conv1.weight"] * 1e6
    with pytest.raises(RuntimeError, match="fp16 operand range"):
        pointnet.pretrained_pointnet(big)(x.cuda())
    nan = dict(state)
    nan["feat.conv3.weight"] = state["feat.conv3.weight"].clone()
    nan["feat.conv3.weight"][5, 7, 0] = float("nan")
    with pytest.raises(ValueError, match="non-finite weight"):
        pointnet.pretrained_pointnet(nan)


# ---- weight packing ----------------------------------------------------------------------------
def _pack(entry, w):
    """One layer through r2dm_pointnet_pack or r2dm_rangenet_pack (one tap): (packed bytes, wscale as bits, flag)"""
    L, (cout, cin) = _lib.lib(), w.shape
    point = entry == "pointnet"
    nbytes = L.r2dm_pointnet_packed_bytes(cout, cin) if point else L.r2dm_rangenet_packed_bytes(cout, cin, 1)
    # (a byte the kernel skips keeps its filler, and the two entries' fillers differ)
    packed = torch.full((nbytes,), 0xA5 if point else 0x5A, dtype=torch.uint8, device="cuda")
    scale, flag = torch.zeros(2, dtype=torch.float32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    args = (_lib.ptr(packed), _lib.ptr(scale), _lib.ptr(flag), _lib.stream_ptr(torch.device("cuda")))
    _lib.check(L.r2dm_pointnet_pack(_lib.ptr(w), cout, cin, *args) if point else L.r2dm_rangenet_pack(_lib.ptr(w), cout, cin, 1, *args))
    return packed, scale.view(torch.int32), int(flag.item())


@pytest.mark.parametrize("cout,cin", [(32, 16), (64, 48), (1024, 128)])
def test_pointnet_and_rangenet_packers_agree(cout, cin):
    """The two packing entries share one kernel; where both apply (cout % 32 == 0, cin % 16 == 0, one tap: nothing is padded) they are one
    function -- size, every packed byte, both wscale words and the flag -- for small, unit and large weights.
    Weights outside the range: the entries' contract (include/r2dm_hip.h) is "*flag |= 4 if a weight is not finite", which covers both
    cases checked here -- one +inf (no power-of-two scale brings it into range; the layer's maximum is then not finite and the layer
    stays unscaled) and one NaN (caught by !(|v| < 65504)).  A large finite weight is no such case: it is rescaled."""
    L = _lib.lib()
    assert L.r2dm_pointnet_packed_bytes(cout, cin) == L.r2dm_rangenet_packed_bytes(cout, cin, 1) == cout * cin * 4
    for seed, s in enumerate((1e-3, 1.0, 300.0)):
        w = (rnd(700 + seed, cout, cin) * s).cuda()
        (pp, ps, pf), (rp, rs, rf) = _pack("pointnet", w), _pack("rangenet", w)
        assert torch.equal(pp, rp) and torch.equal(ps, rs) and pf == rf == 0
        assert ps[0].item() == w.abs().max().view(torch.int32).item()  # (wscale[0]: the bits of max|w|)
    for bad in (float("inf"), float("nan")):
        w = rnd(703, cout, cin)
        w[cout - 3, cin - 5] = bad
        (_, _, pf), (_, _, rf) = _pack("pointnet", w.cuda()), _pack("rangenet", w.cuda())
        assert pf & 4 and rf & 4, (bad, pf, rf)


# ---- distribution metrics ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def sets():
    return {c[0]: G.mmd_sets(c) for c in G.MMD_CASES}


@pytest.mark.parametrize("name", [c[0] for c in G.MMD_CASES])
def test_feature_moments_against_numpy_fp64(sets, name):
    f = sets[name][0]
    mean, cov = metrics.feature_moments(torch.from_numpy(f).cuda())
    assert mean.dtype == cov.dtype == torch.float64 and cov.shape == (f.shape[1], f.shape[1])
    f64 = f.astype(np.float64)
    want = np.cov(f64, rowvar=False)
    e_cov, e_mean = np.abs(cov.cpu().numpy() - want).max(), np.abs(mean.cpu().numpy() - f64.mean(0)).max()
    print(f"{name}: covariance max err {e_cov:.3e} (max |S| {np.abs(want).max():.3e}), mean max err {e_mean:.3e}")
    assert e_cov <= 1e-11 * np.abs(want).max() and e_mean <= 1e-11 * np.abs(f64).max()
    assert torch.equal(cov, cov.T)
    m2, c2 = metrics.feature_moments(torch.from_numpy(f).cuda())
    assert torch.equal(m2, mean) and torch.equal(c2, cov)
    mn, cn = metrics.feature_moments(f)  # (a numpy array -- the reference's cache -- is uploaded)
    assert torch.equal(mn, mean) and torch.equal(cn, cov)


def test_frechet_distance(data, sets):
    f1, f2 = sets["d48"]
    _, _, _, ref, f64, ref_err = data["values_d48"]
    got = metrics.compute_frechet_distance(torch.from_numpy(f1).cuda(), torch.from_numpy(f2).cuda())
    print(f"Frechet distance {got:.15g}; fp64 oracle {f64:.15g} (rel {abs(got - f64) / f64:.2e}); reference {ref:.15g} (own error {ref_err:.2e})")
    assert abs(got - f64) <= 1e-9 * abs(f64)
    assert abs(got - ref) <= 2 * ref_err
    assert metrics.compute_frechet_distance(torch.from_numpy(f1).cuda(), torch.from_numpy(f1).cuda()) < 1e-6 * f64


def test_squared_mmd_recorded_subsets(data, sets):
    f1, f2 = sets["d48"]
    idx1, idx2 = data["idx1_d48"], data["idx2_d48"]
    ref, f64, ref_err = data["values_d48"][:3]
    t1, t2 = torch.from_numpy(f1).cuda(), torch.from_numpy(f2).cuda()
    got = metrics.squared_mmd_from_indices(t1, t2, idx1, idx2)
    print(f"squared MMD {got:.15g}; fp64 oracle {f64:.15g} (err {abs(got - f64):.2e}); reference's own error {ref_err:.2e}")
    assert abs(got - f64) <= ref_err / 20
    assert metrics.squared_mmd_from_indices(t1, t2, idx1, idx2) == got
    # the public entry draws the same subsets from the recorded seed, as the reference does from numpy's global state
    assert metrics.compute_squared_mmd(t1, t2, rng=np.random.RandomState(G.MMD_CASES[0][5])) == got
    with pytest.raises(ValueError, match="outside"):
        metrics.squared_mmd_from_indices(t1, t2, idx1 + 300, idx2)


def test_squared_mmd_feature_width_and_full_subsets(data, sets):
    f1, f2 = sets["d1808"]
    idx1, idx2 = data["idx1_d1808"].astype(np.int64), data["idx2_d1808"].astype(np.int64)
    assert idx1.shape == (3, 1000)
    ref, _, ref_err = data["values_d1808"][:3]
    want = G.squared_mmd_fp64(f1, f2, idx1, idx2)
    got = metrics.squared_mmd_from_indices(torch.from_numpy(f1).cuda(), torch.from_numpy(f2).cuda(), idx1, idx2)
    print(f"squared MMD (D = 1808, m = 1000) {got:.15g}; numpy fp64 {want:.15g} (err {abs(got - want):.2e}); reference's own error {ref_err:.2e}")
    assert abs(got - want) <= ref_err / 20


# ---- evaluate.py -------------------------------------------------------------------------------
def test_evaluate_writes_the_fpd(tmp_path, state, extractor):
    sys.path.insert(0, ROOT)
    import evaluate

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
                     real_scans=None, pointnet_weights=str(weights), mmd_seed=7)
    r = json.loads(open(evaluate.evaluate(args)).read())
    f_gen, f_real = pointnet.pointnet_features(extractor, imgs[:6].cuda()), pointnet.pointnet_features(extractor, imgs[6:].cuda())
    assert set(r["pts"]) == {"frechet_distance", "squared_mmd"} and r["img"] == {}
    assert r["info"]["#real"] == 7 and r["info"]["#fake"] == 6
    assert "FRD" in r["info"]["note"] and "FPD" not in r["info"]["note"]
    assert r["pts"]["frechet_distance"] == metrics.compute_frechet_distance(f_real, f_gen)
    assert r["pts"]["squared_mmd"] == metrics.compute_squared_mmd(f_real, f_gen, rng=np.random.RandomState(7))
    assert np.isfinite(r["pts"]["frechet_distance"]) and np.isfinite(r["pts"]["squared_mmd"])
    # without the option: exactly as before
    args.pointnet_weights, args.sample_dir = None, str(gen) + "_again"
    os.rename(gen, args.sample_dir)
    q = json.loads(open(evaluate.evaluate(args)).read())
    assert q["pts"] == {} and q["img"] == {} and q["bev"] == r["bev"]
    assert q["info"]["note"] == "img (FRD) and pts (FPD) are not computed: they need the RangeNet-53 and PointNet weights"
