"""CPU tests of the geometry metrics: what is derived from the search's sums and from distance matrices (plain torch), the subsampling
draw, the refusal of malformed arguments by the Python layer and by the C ABI, and the command lines' flags.  (The search itself:
tests/test_hip_geometry.py, -m gpu.)"""
import inspect
import math

import numpy as np
import pytest
import torch

import geometry_oracle as O


def cloud(seed, n, scale=30.0, offset=0.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return (g.standard_normal((n, 4)) * scale + offset).astype(np.float32)


def test_raw_names_are_the_oracles():
    from r2dm_amd import geometry

    assert geometry.RAW_NAMES == O.RAW_NAMES and geometry.DERIVED_NAMES == ("cd_sq", "cd", "precision", "recall", "fscore")


def test_chamfer_from_sums_against_the_oracle_and_by_hand():
    from r2dm_amd.geometry import DERIVED_NAMES, chamfer_from_sums

    # by hand: a = {0, 1} and b = {0, 3} on the x axis, tau = 0.5.  a -> b: d = 0, 1; b -> a: d = 0, 2
    a = np.array([[0, 0, 0, 9], [1, 0, 0, 9]], np.float32)
    b = np.array([[0, 0, 0, 9], [3, 0, 0, 9]], np.float32)
    raw = O.raw_sums(a, b, 0.5)
    assert raw.tolist() == [1.0, 1.0, 1.0, 4.0, 2.0, 1.0, 2.0, 2.0]
    got = chamfer_from_sums(torch.from_numpy(raw))
    assert {k: v.item() for k, v in got.items()} == {"cd_sq": 0.5 + 2.0, "cd": 0.5 * (0.5 + 1.0), "precision": 0.5, "recall": 0.5, "fscore": 0.5}
    # against the oracle on random clouds, batched (..., 8)
    pairs = [(cloud(1, 40), cloud(2, 55)), (cloud(3, 7), cloud(4, 3)), (cloud(5, 1), cloud(6, 1))]
    raws = torch.from_numpy(np.stack([O.raw_sums(x, y, 25.0) for x, y in pairs]))
    got = chamfer_from_sums(raws.reshape(3, 1, 8))
    for k, (x, y) in enumerate(pairs):
        want = O.chamfer(x, y, 25.0)
        for name in DERIVED_NAMES:
            assert got[name].shape == (3, 1) and got[name].dtype == torch.float64
            assert got[name][k, 0].item() == pytest.approx(want[name], rel=1e-12, abs=0), (k, name)
    # nothing within tau on either side: P + R = 0 -> fscore 0, not NaN
    far = chamfer_from_sums(torch.tensor([9.0, 3.0, 0.0, 9.0, 3.0, 0.0, 1.0, 1.0]))
    assert far["fscore"].item() == 0.0 and far["precision"].item() == 0.0
    # an empty cloud (the search reports +inf sums against it): every value NaN, no exception, the others untouched
    e = chamfer_from_sums(torch.tensor([[math.inf, math.inf, 0.0, 0.0, 0.0, 0.0, 3.0, 0.0], [0.0, 0.0, 0.0, math.inf, math.inf, 0.0, 0.0, 2.0],
                                        [0.0] * 8, raw.tolist()]))
    for name in DERIVED_NAMES:
        assert e[name][:3].isnan().all() and e[name][3].item() == got_by_hand(name), name
    assert all(math.isnan(v) for v in O.chamfer(a[:0], b).values())
    with pytest.raises(ValueError):
        chamfer_from_sums(torch.zeros(3, 6))


def got_by_hand(name):
    return {"cd_sq": 2.5, "cd": 0.75, "precision": 0.5, "recall": 0.5, "fscore": 0.5}[name]


def test_aggregate_leaves_empty_scans_out():
    from r2dm_amd.geometry import aggregate_chamfer

    raw = torch.tensor([[1.0, 1.0, 1.0, 4.0, 2.0, 1.0, 2.0, 2.0], [math.inf, math.inf, 0.0, 0.0, 0.0, 0.0, 3.0, 0.0],
                        [3.0, 3.0, 0.0, 12.0, 6.0, 3.0, 6.0, 6.0]])
    a = aggregate_chamfer(raw)
    assert (a["scans"], a["empty"]) == (3, 1)
    assert a["micro"]["cd_sq"] == 4.0 / 8 + 16.0 / 8 and a["micro"]["precision"] == 1.0 / 8 and a["micro"]["recall"] == 0.5
    assert a["macro"]["cd_sq"] == 0.5 * (2.5 + 2.5) and a["macro"]["precision"] == 0.5 * (0.5 + 0.0)
    none = aggregate_chamfer(raw[1:2])
    assert none["empty"] == 1 and all(math.isnan(v) for g in ("micro", "macro") for v in none[g].values())
    assert aggregate_chamfer(torch.zeros(0, 8))["scans"] == 0


def test_set_metrics_by_hand_and_against_the_oracle():
    from r2dm_amd import geometry as G

    # generated 0 and 1 are both nearest to real 0, generated 2 to real 2: two of three real clouds are covered
    D = torch.tensor([[1.0, 5.0, 9.0], [2.0, 3.0, 4.0], [7.0, 8.0, 0.5]])
    assert G.coverage(D) == 2 / 3 and O.coverage(D.numpy()) == 2 / 3
    assert G.minimum_matching_distance(D) == (1.0 + 3.0 + 0.5) / 3
    # a tie goes to the lowest index: generated 1 ties between real 0 and real 1 -> real 0, so real 1 stays uncovered
    assert G.coverage(torch.tensor([[1.0, 2.0], [3.0, 3.0]])) == 0.5
    # every cloud the same cloud: all distances tie at 0, everyone's neighbour is the lowest other index -- generated 0 (generated 1 for
    # generated 0) -- which is right for the generated half and wrong for the real half: 0.5 by the tie rule
    z = torch.zeros(3, 3)
    assert G.one_nn_accuracy(z, z, z) == 0.5 and O.one_nn_accuracy(z.numpy(), z.numpy(), z.numpy()) == 0.5
    # two well-separated sets: everyone's neighbour is in its own set
    near, far = torch.full((3, 3), 1.0), torch.full((3, 3), 100.0)
    assert G.one_nn_accuracy(near, far, near) == 1.0
    # the real set a copy of the generated one, clouds distinct: everyone's neighbour is its copy in the other set
    own = torch.tensor([[0.0, 4.0, 5.0], [4.0, 0.0, 6.0], [5.0, 6.0, 0.0]])
    assert G.one_nn_accuracy(own, own, own) == 0.0
    # against the oracle on Chamfer matrices of random clouds, unequal set sizes, on float32 and float64 matrices
    gen = [cloud(10 + k, 30, scale=1.0 + 0.2 * k) for k in range(5)]
    real = [cloud(20 + k, 25, scale=1.0 + 0.3 * k) for k in range(4)]
    Dgg, Dgr, Drr = O.chamfer_matrix(gen, gen), O.chamfer_matrix(gen, real), O.chamfer_matrix(real, real)
    want = O.set_metrics(Dgg, Dgr, Drr)
    assert G.set_metrics(torch.from_numpy(Dgg), torch.from_numpy(Dgr), torch.from_numpy(Drr)) == want
    assert set(want) == {"cov", "mmd", "1-nna"} and 0 < want["cov"] <= 1 and 0 <= want["1-nna"] <= 1
    # refusals
    for bad in (lambda: G.coverage(torch.zeros(0, 3)), lambda: G.coverage(torch.zeros(3)), lambda: G.minimum_matching_distance(torch.tensor([[math.nan]])),
                lambda: G.one_nn_accuracy(torch.zeros(2, 2), torch.zeros(2, 3), torch.zeros(2, 2)),
                lambda: G.one_nn_accuracy(torch.zeros(1, 1), torch.zeros(1, 0), torch.zeros(0, 0))):
        with pytest.raises(ValueError):
            bad()


def test_subsample_does_not_depend_on_the_batch():
    from r2dm_amd.geometry import subsample, subsample_indices

    counts = [50, 8, 0, 33]
    off = np.concatenate([[0], np.cumsum(counts)])
    pts = torch.from_numpy(cloud(7, int(off[-1])))
    n, seed = 16, 3
    clouds, kept = subsample(pts, off, n, seed)
    assert clouds.shape == (4, n, 4) and kept.tolist() == [16, 8, 0, 16]
    for k, c in enumerate(counts):
        idx = subsample_indices(c, n, seed, k)
        assert idx.numel() == min(c, n) == idx.unique().numel() and (c <= n) == torch.equal(idx, torch.arange(min(c, n)))
        assert torch.equal(clouds[k, :idx.numel()], pts[int(off[k]) + idx]) and (clouds[k, idx.numel():] == 0).all()
        # the cloud alone, as cloud k of its set: the same draw
        alone, _ = subsample(pts[off[k]:off[k + 1]], [0, c], n, seed, first_index=k)
        assert torch.equal(alone[0], clouds[k])
    # the draw depends on the seed and on the cloud's index, on nothing else
    assert not torch.equal(subsample_indices(50, n, seed, 0), subsample_indices(50, n, seed, 1))
    assert not torch.equal(subsample_indices(50, n, seed, 0), subsample_indices(50, n, seed + 1, 0))
    assert torch.equal(subsample_indices(50, n, seed, 0), subsample_indices(50, n, seed, 0))
    for bad in (lambda: subsample(pts, off, 0, seed), lambda: subsample(pts[:, :3], off, n, seed), lambda: subsample(pts, off + 1, n, seed),
                lambda: subsample(pts, off[::-1].copy(), n, seed), lambda: subsample(pts, [0], n, seed)):
        with pytest.raises(ValueError):
            bad()


def test_malformed_arguments_are_refused_before_the_gpu_is_asked_for():
    """Shapes are judged first, then the device (no CPU fallback), then -- with the points on a GPU -- offsets, pairs and the threshold; the
    helpers that judge those are called here directly."""
    import r2dm_amd
    from r2dm_amd import geometry as G
    from r2dm_amd._lib import R2DMError

    p, off = torch.zeros(6, 4), [0, 2, 6]
    for call in (lambda: r2dm_amd.nearest_neighbors(p, off, p, off), lambda: r2dm_amd.chamfer_sums(p, off, p, off),
                 lambda: r2dm_amd.pairwise_chamfer(torch.zeros(2, 3, 4), [3, 3], torch.zeros(2, 3, 4), [3, 3]),
                 lambda: G.clouds_of_samples(torch.zeros(1, 5, 4, 8), 0.5, 63.0)):
        with pytest.raises(R2DMError, match="no CPU fallback"):
            call()
    for call in (lambda: r2dm_amd.chamfer_sums(torch.zeros(6, 3), off, p, off), lambda: r2dm_amd.chamfer_sums(torch.zeros(6), off, p, off),
                 lambda: G.clouds_of_samples(torch.zeros(1, 4, 4, 8), 0.5, 63.0),
                 lambda: G.clouds_of_samples(torch.zeros(1, 5, 4, 8), 0.5, 63.0, region=torch.ones(1, 1, 4, 4))):
        with pytest.raises(ValueError):
            call()
    for bad in ([0], [[0, 6]], [0.0, 6.0], [0, 7], [-1, 6], [0, 4, 2, 6]):
        with pytest.raises(ValueError, match="offsets"):
            G._host_offsets(bad, 6, "a_offsets")
    with pytest.raises(ValueError, match="2\\^21"):
        G._host_offsets([0, (1 << 21) + 1], 1 << 22, "a_offsets")
    assert G._host_offsets(torch.tensor([0, 0, 6]), 6, "a_offsets").tolist() == [0, 0, 6]
    assert G._pairs(None, 3, 3).tolist() == [[0, 0], [1, 1], [2, 2]] and G._pairs(torch.tensor([[1, 0]]), 2, 1).tolist() == [[1, 0]]
    for bad in (lambda: G._pairs(None, 2, 3), lambda: G._pairs([[0, 0, 0]], 2, 2), lambda: G._pairs([0, 1], 2, 2), lambda: G._pairs([[0.0, 1.0]], 2, 2),
                lambda: G._pairs([[2, 0]], 2, 2), lambda: G._pairs([[0, 2]], 2, 2), lambda: G._pairs([[-1, 0]], 2, 2)):
        with pytest.raises(ValueError, match="pairs"):
            bad()
    for tau in (-0.1, math.nan, math.inf):
        with pytest.raises(ValueError, match="threshold"):
            G._check_tau(tau)
    for bad in (lambda: G._compact(torch.zeros(2, 3, 3), [3, 3], "A"), lambda: G._compact(torch.zeros(2, 3, 4), [3], "A"),
                lambda: G._compact(torch.zeros(2, 3, 4), [3, 4], "A"), lambda: G._compact(torch.zeros(2, 3, 4), [-1, 3], "A"),
                lambda: G._compact(torch.zeros(2, 3, 4), [1.0, 3.0], "A"), lambda: G._compact(torch.zeros(0, 3, 4), [], "A")):
        with pytest.raises(ValueError, match="A:"):
            bad()
    pts, o = G._compact(torch.arange(24.0).reshape(2, 3, 4), [1, 3], "A")
    assert o.tolist() == [0, 1, 4] and pts[:, 0].tolist() == [0.0, 12.0, 16.0, 20.0]


def test_c_abi_refuses_bad_arguments_with_a_status():
    """Every refusal is a status and a message, decided before anything touches a GPU (the pointers here are made-up addresses)."""
    from r2dm_amd import _lib

    L = _lib.lib()
    base = dict(a=4096, a_offsets=8192, a_clouds=2, a_total=100, b=12288, b_offsets=16384, b_clouds=2, b_total=100, pairs=20480, P=2, max_points=64,
                tau=0.2, d2_ab=None, idx_ab=None, out_ab=None, d2_ba=None, idx_ba=None, out_ba=None, scratch=24576, sums=28672, status=32768)

    def nn(**kw):
        return L.r2dm_nn_pairs(*{**base, **kw}.values(), None), L.r2dm_last_error().decode()

    for null in ("a_offsets", "b_offsets", "pairs", "scratch", "sums", "status"):
        rc, msg = nn(**{null: None})
        assert rc == 1 and "null argument" in msg, null
    for kw in (dict(a=None), dict(b=None), dict(a_clouds=0), dict(b_clouds=-1), dict(a_total=-1)):
        rc, msg = nn(**kw)
        assert rc == 1 and "at least one cloud" in msg, kw
    rc, msg = nn(max_points=(1 << 21) + 1)
    assert rc == 1 and "2^21" in msg
    for kw in (dict(P=0), dict(P=-3), dict(max_points=0), dict(P=1 << 30, max_points=1024), dict(P=1 << 20, max_points=1 << 21)):
        rc, msg = nn(**kw)
        assert rc == 1 and "2^31 - 1 blocks" in msg, kw
    for tau in (-1.0, math.nan):
        rc, msg = nn(tau=tau)
        assert rc == 1 and "tau must be >= 0" in msg
    for kw in (dict(idx_ab=4096), dict(idx_ba=4096), dict(d2_ab=4096), dict(d2_ba=4096)):
        rc, msg = nn(**kw)
        assert rc == 1 and "an index output needs" in msg, kw
    for name in ("a", "b"):
        rc, msg = nn(**{name: 4096 + 8})
        assert rc == 1 and "16-byte aligned" in msg, name
    for name in ("a_offsets", "b_offsets", "pairs", "scratch", "sums", "status"):
        rc, msg = nn(**{name: 8192 + 4})
        assert rc == 1 and "8-byte aligned" in msg, name
    rc, msg = nn(d2_ab=4096 + 2, out_ab=8192)
    assert rc == 1 and "4-byte aligned" in msg

    f = L.r2dm_nn_pairs_scratch_bytes
    for empty in ((0, 64), (-1, 64), (2, 0), (2, (1 << 21) + 1), (1 << 30, 1024), (1 << 20, 1 << 21)):
        assert f(*empty) == 0, empty
    # per pair, direction and chunk of 1024 query points one partial of four doubles
    assert f(1, 1) == f(1, 1024) == 2 * 32 and f(1, 1025) == 2 * 2 * 32 and f(5, 2048) == 5 * f(1, 2048) and f(1, 1 << 21) == 2 * 2048 * 32
    assert f(((1 << 31) - 1) // 2, 1024) > 0


def test_command_line_flags():
    import completion_eval
    import geometry_eval
    from r2dm_amd.completion import evaluate_completion

    # completion_eval.py: off by default, and then the document is what it was (no geometry entry, no new info)
    a = completion_eval.build_parser().parse_args(["--ckpt", "m.pth", "--real_scans", "d"])
    assert a.chamfer is False and a.fscore_threshold == 0.2
    a = completion_eval.build_parser().parse_args(["--ckpt", "m.pth", "--real_scans", "d", "--chamfer", "--fscore_threshold", "0.5"])
    assert a.chamfer is True and a.fscore_threshold == 0.5
    sig = inspect.signature(evaluate_completion).parameters
    assert sig["chamfer"].default is False and sig["fscore_threshold"].default == 0.2
    src = inspect.getsource(completion_eval.main)
    assert 'if args.chamfer:\n        info["fscore_threshold"]' in src  # (the only new key of the document's info, and only when asked for)

    p = geometry_eval.build_parser()
    a = p.parse_args(["--sample_dir", "s", "--real_dir", "r"])
    assert (a.points, a.limit, a.seed, a.out, a.real_scans, a.ckpt) == (2048, 2000, 0, "geometry.json", None, None)
    a = p.parse_args(["--sample_dir", "s", "--real_scans", "r", "--ckpt", "m.pth", "--points", "512", "--limit", "10", "--seed", "4", "--out", "o.json"])
    assert (a.points, a.limit, a.seed, a.out, a.real_scans, str(a.ckpt)) == (512, 10, 4, "o.json", "r", "m.pth")
    assert (geometry_eval.MIN_DEPTH, geometry_eval.MAX_DEPTH) == (0.5, 63.0)  # LiDARGen's window, evaluate.py's
    with pytest.raises(SystemExit):
        p.parse_args(["--real_dir", "r"])
    with pytest.raises(SystemExit, match="one of --real_scans"):
        geometry_eval.main(["--sample_dir", "s"])
    with pytest.raises(SystemExit, match="one of --real_scans"):
        geometry_eval.main(["--sample_dir", "s", "--real_dir", "r", "--real_scans", "q"])
    with pytest.raises(SystemExit, match="must be >= 1"):
        geometry_eval.main(["--sample_dir", "s", "--real_dir", "r", "--points", "0"])
