"""-m gpu: voxel occupancy (r2dm_amd/csrc/voxel.hip, r2dm_amd.geometry.voxel_occupancy_counts / voxel_iou, evaluate_completion(voxel_sizes=...))
against the numpy specification of tests/voxel_oracle.py.

Every comparison is exact integer equality: the kernel's only floating-point operations are one IEEE float32 division and one floor per
axis, which numpy's float32 ``/`` and ``floor`` reproduce bit for bit; everything after them is integers.  The shapes are the smallest at
which each part can go wrong (a few thousand points at the most); every case runs in well under a second."""
import copy
import json
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, GOLDEN_RES, synthetic_ckpt

sys.path.insert(0, GOLDEN)
import make_golden_projection as MG  # noqa: E402  (read-only: the integer-only generator of the free cloud)

import voxel_oracle as VO  # noqa: E402
import r2dm_amd  # noqa: E402
from r2dm_amd import completion, geometry  # noqa: E402
from r2dm_amd._lib import R2DMError  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ragged(clouds):
    """a list of (n,3) arrays -> ((total,4) float32 on the device, offsets)"""
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    pts = np.zeros((int(off[-1]), 4), np.float32)
    if off[-1]:
        pts[:, :3] = np.concatenate([np.asarray(c, np.float32).reshape(-1, 3) for c in clouds])
    pts[:, 3] = 7.0  # (the fourth value is not read)
    return torch.from_numpy(pts).to(DEV), off


def counts_of(res):
    return res["member"].cpu().numpy(), res["hist"].cpu().numpy()


def check_groups(a_clouds, b_clouds, members, targets, sizes):
    """run the groups, compare with the oracle, return the device's integers"""
    (a, off_a), (b, off_b) = ragged(a_clouds), ragged(b_clouds)
    res = geometry.voxel_occupancy_counts(a, off_a, b, off_b, members, targets, sizes)
    assert res["member"].dtype == torch.int64 and res["hist"].dtype == torch.int64 and res["member"].is_cuda
    member, hist = counts_of(res)
    wm, wh = VO.occupancy_groups(a.cpu().numpy(), off_a, b.cpu().numpy(), off_b, np.asarray(members), np.asarray(targets), sizes)
    print("member", member.reshape(-1)[:16].tolist(), "want", wm.reshape(-1)[:16].tolist(), "hist", hist.reshape(-1)[:16].tolist(), "want", wh.reshape(-1)[:16].tolist())
    assert np.array_equal(member, wm) and np.array_equal(hist, wh)
    assert (hist[:, :, 0, 0] == 0).all()
    return member, hist


def check_pairs(a_clouds, b_clouds, pairs, sizes):
    (a, off_a), (b, off_b) = ragged(a_clouds), ragged(b_clouds)
    res = geometry.voxel_iou(a, off_a, b, off_b, pairs, sizes)
    got = res["counts"].cpu().numpy()
    pr = [(k, k) for k in range(len(a_clouds))] if pairs is None else pairs
    want = np.array([[VO.iou_counts(a_clouds[i], b_clouds[j], s) for s in sizes] for i, j in pr], np.int64).reshape(len(pr), len(sizes), 3)
    print("counts", got.tolist(), "want", want.tolist())
    assert got.dtype == np.int64 and np.array_equal(got, want)
    derived = geometry.voxel_from_counts(torch.from_numpy(want))
    for name in geometry.VOXEL_NAMES:
        assert torch.equal(res[name].cpu().isnan(), derived[name].isnan()) and torch.equal(res[name].cpu().nan_to_num(-1), derived[name].nan_to_num(-1))
    return got, res


# ---- 1. cell faces and sign ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [0.25, 0.5, 0.1])
def test_cell_faces_and_sign(size):
    """The points fl32(k s) and their two float32 neighbours, k = -50 .. 50, on every axis, against the mirrored cloud: at s = 0.25 and 0.5 the
    quotient is exact and the point below a face belongs to the cell below (floor, not truncation, for k <= 0); at s = 0.1 the rounding of the
    float32 division decides (a division in higher precision or a reciprocal multiply gives other cells: tests/test_voxel_cpu.py)."""
    face = (np.arange(-50, 51) * np.float64(np.float32(size))).astype(np.float32)
    vals = np.concatenate([face, np.nextafter(face, np.float32(-np.inf)), np.nextafter(face, np.float32(np.inf))]).astype(np.float32)
    n = vals.size
    i = np.arange(n)
    cloud = np.stack([vals[i], vals[(7 * i + 3) % n], vals[(13 * i + 5) % n]], axis=1)  # (7 and 13 are coprime to 303: every axis meets every value)
    assert all(np.array_equal(np.sort(cloud[:, ax]), np.sort(vals)) for ax in range(3))
    got, _ = check_pairs([cloud, -cloud], [-cloud, cloud], [(0, 0), (0, 1), (1, 1)], [size])
    assert got[1, 0, 0] == got[1, 0, 1] == got[1, 0, 2]  # a cloud against itself
    member, _ = check_groups([cloud, -cloud], [cloud], [[0, 1]], [0], [size])
    assert member[0, 0, 0, 0] == member[0, 0, 0, 1]


# ---- 2. probing ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4096, 3, 5000])
def test_distinct_voxels_fill_the_table_to_its_load_factor(n):
    """n points in n distinct voxels against another n, half of them shared: 1.5 n keys in a table of the power of two >= 4 n slots"""
    g = np.random.Generator(np.random.PCG64(n))
    ids = np.unique(g.integers(-2000, 2000, (4 * n + 16, 3)), axis=0)
    ids = ids[g.permutation(len(ids))][:2 * n]
    assert len(ids) == 2 * n
    pts = (ids + 0.5) * 0.5
    a, b = pts[:n], pts[n // 2:n // 2 + n]
    got, res = check_pairs([a], [b], None, [0.5])
    assert got.tolist() == [[[n - n // 2, n, n]]]
    assert res["iou"].item() == (n - n // 2) / (n + n // 2)


# ---- 3. contention -------------------------------------------------------------------------------------------------------------------------
def test_many_points_in_few_voxels():
    g = np.random.Generator(np.random.PCG64(3))
    corners = np.array([[0.0, 0.0, 0.0], [-0.5, 0.0, 3.0], [10.0, -7.5, 0.5]])
    crowd = corners[g.integers(0, 3, 4096)] + g.uniform(0.01, 0.49, (4096, 3))
    one = np.array([[0.25, 0.25, 0.25]])
    got, _ = check_pairs([crowd, one, crowd], [one, crowd, crowd], None, [0.5])
    assert got.tolist() == [[[1, 3, 1]], [[1, 1, 3]], [[3, 3, 3]]]
    (a, off) = ragged([crowd])
    same = geometry.voxel_iou(a, off, a, off, sizes=[0.5])  # one allocation as both sides
    assert same["counts"].cpu().tolist() == [[[3, 3, 3]]] and same["iou"].item() == 1.0


# ---- 4. empty clouds -----------------------------------------------------------------------------------------------------------------------
def test_empty_clouds_inside_a_batch():
    g = np.random.Generator(np.random.PCG64(4))
    full = lambda n: g.uniform(-2, 2, (n, 3))
    none = np.zeros((0, 3))
    a, b = [full(70), none, full(50), none, full(300)], [full(80), full(60), none, none, full(300)]
    got, res = check_pairs(a, b, None, [0.5, 1.0])
    assert (got[1, :, :2] == 0).all() and (got[2, :, 0] == 0).all() and (got[2, :, 2] == 0).all() and (got[3] == 0).all() and (got[[0, 4], :, 0] > 0).all()
    iou, p, r = res["iou"].cpu(), res["precision"].cpu(), res["recall"].cpu()
    assert (iou[1] == 0).all() and p[1].isnan().all() and (r[1] == 0).all()                  # an empty prediction
    assert (iou[2] == 0).all() and (p[2] == 0).all() and r[2].isnan().all()                  # an empty target
    assert all(res[k][3].isnan().all() for k in geometry.VOXEL_NAMES)                        # both
    alone, _ = check_pairs([a[0], a[4]], [b[0], b[4]], None, [0.5, 1.0])
    assert np.array_equal(alone, got[[0, 4]])                                                # the neighbours are what they are alone
    # an ensemble whose clouds are all empty, next to one that has points
    member, hist = check_groups([none, none, a[0], a[2]], [none, b[0]], [[0, 1], [2, 3]], [0, 1], [0.5])
    assert (member[0] == 0).all() and (hist[0] == 0).all() and hist[1].sum() > 0
    d = geometry.occupancy_from_counts(torch.from_numpy(member), torch.from_numpy(hist))
    assert d["brier"][0].isnan().all() and d["any_iou"][0].isnan().all() and not d["brier"][1].isnan().any()


# ---- 5. members ----------------------------------------------------------------------------------------------------------------------------
def ensemble_case(K, seed=0):
    """two groups of K members around a target each: lattice points jittered inside their cells, so that members share many voxels"""
    g = np.random.Generator(np.random.PCG64(100 * K + seed))
    clouds, targets = [], []
    for _ in range(2):
        base = g.integers(-8, 8, (400, 3))
        alone = g.integers(20, 30, (15, 3))  # voxels of the target that no member reaches
        targets.append((np.concatenate([base[g.random(400) < 0.7], alone]) + g.uniform(0.05, 0.95, (1, 3))) * 0.25)
        for k in range(K):
            keep = base[g.random(400) < g.uniform(0.2, 0.9)]
            extra = g.integers(-9, 9, (int(g.integers(0, 40)), 3))
            pts = np.concatenate([keep, extra])
            clouds.append((pts + g.uniform(0.05, 0.95, pts.shape)) * 0.25)
    members = np.arange(2 * K).reshape(2, K)
    return clouds, targets, members, np.arange(2)


@pytest.mark.parametrize("K", [1, 2, 3, 16, 63])
def test_members_against_the_oracle_and_bitwise_properties(K):
    clouds, targets, members, tg = ensemble_case(K)
    sizes = [0.25, 0.6]
    member, hist = check_groups(clouds, targets, members, tg, sizes)
    assert hist[:, :, :, 1:].sum() > 0 and (K == 1 or hist[:, :, :, 2:].sum() > 0) and hist[:, :, 1, 0].sum() > 0
    # K = 1 is the pair
    if K == 1:
        assert np.array_equal(member[:, :, 0, 1], hist[:, :, 1, 1]) and np.array_equal(member[:, :, 0, 0], hist[:, :, 1, 1] + hist[:, :, 0, 1])
    # the members permuted: their rows permute, the histogram keeps its bits
    g = np.random.Generator(np.random.PCG64(K))
    perm = g.permutation(K)
    m2, h2 = check_groups(clouds, targets, members[:, perm], tg, sizes)
    assert m2.tobytes() == np.ascontiguousarray(member[:, :, perm]).tobytes() and h2.tobytes() == hist.tobytes()
    # the points of every cloud shuffled; the same call twice
    m3, h3 = check_groups([c[g.permutation(len(c))] for c in clouds], [t[g.permutation(len(t))] for t in targets], members, tg, sizes)
    m4, h4 = check_groups(clouds, targets, members, tg, sizes)
    assert m3.tobytes() == member.tobytes() == m4.tobytes() and h3.tobytes() == hist.tobytes() == h4.tobytes()


def test_more_than_63_members_are_refused():
    clouds, targets, _, _ = ensemble_case(1)
    (a, off_a), (b, off_b) = ragged(clouds), ragged(targets)
    with pytest.raises(ValueError, match="63"):
        geometry.voxel_occupancy_counts(a, off_a, b, off_b, np.zeros((1, 64), np.int64), [0], [0.5])


# ---- 6. several sizes, shared clouds, pairs in any order ---------------------------------------------------------------------------------
def test_sizes_groups_and_pairs():
    g = np.random.Generator(np.random.PCG64(6))
    clouds = [g.normal(0, 2.0, (int(n), 3)) for n in (500, 37, 1300, 256, 1)]
    sizes = [0.1, 0.2, 0.5]
    # five groups over one set: cloud 0 a member of groups 0 and 1 and the target of group 2, a group of one cloud against itself, a repeated member
    members, targets = [[0, 1, 2], [3, 0, 4], [1, 2, 3], [4, 4, 4], [2, 2, 0]], [3, 2, 0, 4, 1]
    member, hist = check_groups(clouds, clouds, members, targets, sizes)
    (a, off) = ragged(clouds)
    for s, size in enumerate(sizes):  # S = 3 in one call = three calls with S = 1
        one = geometry.voxel_occupancy_counts(a, off, a, off, members, targets, [size])
        m1, h1 = counts_of(one)
        assert np.array_equal(m1[:, 0], member[:, s]) and np.array_equal(h1[:, 0], hist[:, s])
    assert np.array_equal(member[3, :, :, 0], member[3, :, :, 1]) and (hist[3, :, 1, 3] == 1).all() and hist[3].sum() == len(sizes)
    pairs = [(4, 0), (2, 2), (0, 3), (3, 0), (1, 4), (2, 0)]
    got, _ = check_pairs(clouds, clouds[::-1], pairs, sizes)
    assert np.array_equal(got[2][:, [0, 2, 1]], check_pairs(clouds[::-1], clouds, [(3, 0)], sizes)[0][0])  # (a, b) swapped: the two counts swap
    # slabs: with a bound of one table per call every group goes alone, and the integers are the same
    bound, geometry.VOXEL_SLAB_BYTES = geometry.VOXEL_SLAB_BYTES, 1
    try:
        m2, h2 = counts_of(geometry.voxel_occupancy_counts(a, off, a, off, members, targets, sizes))
    finally:
        geometry.VOXEL_SLAB_BYTES = bound
    assert np.array_equal(m2, member) and np.array_equal(h2, hist)


# ---- 7. status -----------------------------------------------------------------------------------------------------------------------------
def test_points_that_do_not_count_are_refused():
    g = np.random.Generator(np.random.PCG64(7))
    good = g.uniform(-5, 5, (100, 3)).astype(np.float32)
    bad = good.copy()
    bad[17, 1], bad[60, 2] = np.nan, np.inf
    (a, off_a), (b, off_b) = ragged([bad]), ragged([good])
    with pytest.raises(ValueError, match="2 points with a non-finite"):
        geometry.voxel_iou(a, off_a, b, off_b, sizes=[0.5])
    with pytest.raises(ValueError, match="1 points with a non-finite"):
        geometry.voxel_iou(b, off_b, a[:50], [0, 50], sizes=[0.5])
    # the grid ends at 2^20 cells each way: floor(x / s) = 2^20 is outside, the float below it inside, and -2^20 is the first cell
    edge = np.float32(2 ** 19)  # / 0.5 = 2^20
    inside = good.copy()
    inside[3, 0], inside[4, 2], inside[5, 1] = np.nextafter(edge, np.float32(0)), -edge, np.nextafter(edge, np.float32(0))
    got, _ = check_pairs([inside], [good], None, [0.5])
    assert got[0, 0, 1] > got[0, 0, 0]
    for axis, value in ((0, edge), (1, edge), (2, edge), (0, np.nextafter(-edge, np.float32(-np.inf)))):
        outside = good.copy()
        outside[9, axis] = value
        a, off_a = ragged([outside])
        with pytest.raises(ValueError, match="1 points outside the grid"):
            geometry.voxel_iou(a, off_a, b, off_b, sizes=[0.5])
        with pytest.raises(ValueError, match="2 points outside the grid"):  # once per size: inside at 1 m, outside at 0.5 and 0.25
            geometry.voxel_iou(a, off_a, b, off_b, sizes=[0.5, 1.0, 0.25])


def test_a_group_that_does_not_check_out_is_skipped():
    clouds, targets, _, _ = ensemble_case(2)
    (a, off_a), (b, off_b) = ragged(clouds), ragged(targets)
    members = [[0, 1], [2, 4], [3, 2], [-1, 0]]  # a holds clouds 0 .. 3
    with pytest.raises(R2DMError, match="2 groups"):
        geometry.voxel_occupancy_counts(a, off_a, b, off_b, members, [0, 1, 1, 0], [0.25])
    with pytest.raises(R2DMError, match="1 groups"):
        geometry.voxel_occupancy_counts(a, off_a, b, off_b, [[0, 1], [2, 3]], [0, 2], [0.25])
    res = geometry.voxel_occupancy_counts(a, off_a, b, off_b, members, [0, 1, 1, 0], [0.25], _raise=False)
    assert res["status"].cpu().tolist() == [0, 0, 2, 0]
    member, hist = counts_of(res)
    wm, wh = VO.occupancy_groups(a.cpu().numpy(), off_a, b.cpu().numpy(), off_b, np.array([[0, 1], [3, 2]]), [0, 1], [0.25])
    assert np.array_equal(member[[0, 2]], wm) and np.array_equal(hist[[0, 2]], wh)
    assert (member[[1, 3]] == 0).all() and (hist[[1, 3]] == 0).all()  # nothing is written for the groups that are skipped


# ---- 8. images -----------------------------------------------------------------------------------------------------------------------------
LO, HI = 1.45, 80.0


def planes(B, H, W, seed):
    """(B,5,H,W) [depth, x, y, z, reflectance]: smooth walls a few metres away seen along a fan of rays, with some pixels outside the depth window"""
    g = np.random.Generator(np.random.PCG64(seed))
    az = np.linspace(-np.pi, np.pi, W, endpoint=False)[None, None, :]
    el = np.linspace(0.05, -0.4, H)[None, :, None]
    depth = 6.0 + 3.0 * np.sin(2 * az + g.uniform(0, 6, (B, 1, 1))) + 2.0 * el + g.normal(0, 0.02, (B, H, W))
    depth = np.where(g.random((B, H, W)) < 0.1, g.choice([0.0, 1.0, 90.0], (B, H, W)), depth)
    xyz = np.stack([depth * np.cos(el) * np.cos(az), depth * np.cos(el) * np.sin(az), depth * np.sin(el)], axis=1)
    return torch.from_numpy(np.concatenate([depth[:, None], xyz, g.random((B, 1, H, W))], axis=1).astype(np.float32)).to(DEV)


@pytest.mark.parametrize("shape", [(3, 8, 64), (2, 16, 128)])
def test_images_through_clouds_of_samples(shape):
    B, H, W = shape
    target = planes(B, H, W, 1)
    pred = target.clone()
    noise = planes(B, H, W, 2)
    pred[:, :, H // 2:] = noise[:, :, H // 2:]  # the lower half redrawn
    region = torch.zeros(B, 1, H, W, device=DEV)
    region[:, :, H // 4:] = 1
    sizes = [0.1, 0.2, 0.5]
    for reg in (None, region):
        pa, oa = geometry.clouds_of_samples(pred, LO, HI, reg)
        pb, ob = geometry.clouds_of_samples(target, LO, HI, reg)
        res = geometry.voxel_iou(pa, oa, pb, ob, sizes=sizes)
        a, b = pa.cpu().numpy(), pb.cpu().numpy()
        oa, ob = np.asarray(oa.cpu() if isinstance(oa, torch.Tensor) else oa), np.asarray(ob.cpu() if isinstance(ob, torch.Tensor) else ob)
        want = np.array([[VO.iou_counts(a[oa[k]:oa[k + 1]], b[ob[k]:ob[k + 1]], s) for s in sizes] for k in range(B)])
        got = res["counts"].cpu().numpy()
        print("counts", got.tolist(), "want", want.tolist())
        assert np.array_equal(got, want) and (got[..., 0] > 0).all() and (got[..., 0] < got[..., 1]).all()
        same = geometry.voxel_iou(pb, ob, pb, ob, sizes=sizes)
        assert (same["iou"] == 1).all() and (same["f1"] == 1).all() and torch.equal(same["counts"][..., 0], same["counts"][..., 2])


# ---- 9. evaluate_completion ----------------------------------------------------------------------------------------------------------------
SEED, KIND, METHODS, SIZES = 5, "beams:4", ("dpmpp", "linear", "target"), (0.2, 0.5)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """evaluate_completion on two small scans with a 2-step sampler and an ensemble of 3: with voxel sizes and without"""
    import completion_eval

    tmp = tmp_path_factory.mktemp("voxel")
    ckpt = tmp / "synthetic.pth"
    torch.save(synthetic_ckpt(resolution=GOLDEN_RES), ckpt)
    pts = MG.make_cloud("free_64x1024")
    for k, s in enumerate([np.ascontiguousarray(pts[0:25000]), np.ascontiguousarray(pts[30000:52000])]):
        d = tmp / "scans" / f"seq_{k}"
        d.mkdir(parents=True)
        s.tofile(d / f"{k:010d}.bin")
    ddpm, lidar, cfg = r2dm_amd.setup_model(str(ckpt), device=DEV, show_info=False, max_batch=2)
    scans = sorted((tmp / "scans").rglob("*.bin"))
    pl = completion_eval.planes_of_scans(scans, cfg, lidar, 2, torch.device(DEV))
    go = lambda **kw: completion.evaluate_completion(ddpm, lidar, pl, [KIND], methods=METHODS, num_steps=2, seed=SEED, batch_size=2, keep=True,
                                                     ensemble=3, **kw)
    return go(voxel_sizes=SIZES), go(), lidar


def clouds_of(img, lo, hi, region=None):
    """(N,5,H,W) numpy planes -> per image the (n,3) points of its returns (inside ``region``)"""
    keep = (img[:, 0] > np.float32(lo)) & (img[:, 0] < np.float32(hi)) & np.isfinite(img[:, 1:4]).all(axis=1)
    if region is not None:
        keep &= region[:, 0] != 0
    return [img[i, 1:4][:, keep[i]].T for i in range(img.shape[0])]


def test_the_kept_integers_equal_the_oracle_on_the_kept_predictions(runs):
    (res, kept), _, lidar = runs
    k = kept[KIND]
    lo, hi = float(lidar.min_depth), float(lidar.max_depth)
    target, unknown = k["target"].numpy(), (k["mask"] == 0).numpy()
    N = target.shape[0]
    for method in METHODS:
        entry = res[KIND][method]
        assert entry["voxel"]["sizes"] == [float(np.float32(s)) for s in SIZES] == entry["ensemble"]["occupancy"]["sizes"]
        pred = k["pred"][method].numpy()
        xs = k["ensemble"][method]["x_out"]
        K = 3 if method == "dpmpp" else 1
        if K == 3:
            members = lidar.postprocess(xs.to(DEV).flatten(0, 1).clamp(-1, 1)).reshape(N, K, *pred.shape[1:]).cpu().numpy()
            assert np.array_equal(members[:, 0], pred)
        else:
            members = pred[:, None]
        for where, region in (("all", None), ("inpainted", unknown)):
            tc = clouds_of(target, lo, hi, region)
            raw = k["voxel_raw"][method][where]
            want = np.array([[VO.iou_counts(p, t, s) for s in SIZES] for p, t in zip(clouds_of(pred, lo, hi, region), tc)])
            assert raw.dtype == torch.int64 and np.array_equal(raw.numpy(), want), (method, where)
            assert json.dumps(completion.jsonable(entry["voxel"][where]), sort_keys=True) == \
                json.dumps(completion.jsonable(geometry.aggregate_voxel(raw, SIZES)), sort_keys=True)
            occ = k["ensemble"][method]["occupancy"][where]
            assert tuple(occ["member"].shape) == (N, len(SIZES), K, 2) and tuple(occ["hist"].shape) == (N, len(SIZES), 2, K + 1)
            for i in range(N):
                mc = [clouds_of(members[i:i + 1, m], lo, hi, None if region is None else region[i:i + 1])[0] for m in range(K)]
                for s, size in enumerate(SIZES):
                    wm, wh = VO.occupancy(mc, tc[i], size)
                    assert np.array_equal(occ["member"][i, s].numpy(), wm) and np.array_equal(occ["hist"][i, s].numpy(), wh), (method, where, i, size)
            assert json.dumps(completion.jsonable(entry["ensemble"]["occupancy"][where]), sort_keys=True) == \
                json.dumps(completion.jsonable(geometry.aggregate_occupancy(occ["member"], occ["hist"], SIZES)), sort_keys=True)
            # member 0 is the prediction: its row is the pair's counts
            assert np.array_equal(occ["member"][:, :, 0, 1].numpy(), want[..., 0]) and np.array_equal(occ["member"][:, :, 0, 0].numpy(), want[..., 1])
    json.dumps(completion.jsonable(res), allow_nan=False)


def test_the_target_scores_one(runs):
    (res, kept), _, _ = runs
    e = res[KIND]["target"]
    for where in ("all", "inpainted"):
        v = e["voxel"][where]
        assert v["empty"] == 0 and all(v[avg][name] == [1.0, 1.0] for avg in ("micro", "macro") for name in geometry.VOXEL_NAMES), v
        o = e["ensemble"]["occupancy"][where]
        assert o["members"] == 1 and o["micro"]["brier"] == [0.0, 0.0] and o["micro"]["consensus_iou"] == [1.0, 1.0] and o["micro"]["member_iou"] == [[1.0], [1.0]]
    moved = res[KIND]["dpmpp"]["voxel"]["inpainted"]["micro"]["iou"]
    assert all(0.0 <= v < 1.0 for v in moved), moved


def test_without_voxel_sizes_the_document_is_what_it_was(runs):
    (res, kept), (res0, kept0), _ = runs
    assert all("voxel" not in e and "occupancy" not in e["ensemble"] for e in res0[KIND].values()) and "voxel_raw" not in kept0[KIND]
    stripped = copy.deepcopy(res)
    for e in stripped[KIND].values():
        del e["voxel"], e["ensemble"]["occupancy"]
    assert json.dumps(completion.jsonable(stripped), sort_keys=True) == json.dumps(completion.jsonable(res0), sort_keys=True)
    for method in METHODS:
        assert "occupancy" not in kept0[KIND]["ensemble"][method]
        assert torch.equal(kept[KIND]["pred"][method], kept0[KIND]["pred"][method])
