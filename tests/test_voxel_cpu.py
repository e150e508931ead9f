"""No GPU: the voxel oracles against each other, what r2dm_amd.geometry derives from voxel counts (plain torch on integers), the refusals of the
C entry r2dm_voxel_occupancy (decided before anything touches a GPU) and the new options' defaults.

Everything derived is a ratio of two integers below 2^53 evaluated once in float64: the comparisons are exact equality with the same ratio
written out here."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import voxel_oracle as VO
from r2dm_amd import geometry as G


# ---- the oracles -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_the_two_oracles_agree(seed):
    g = np.random.Generator(np.random.PCG64(seed))
    K, size = int(g.integers(1, 5)), [0.1, 0.25, 0.5, 1.0, 0.3, 0.07][seed]
    # few voxels, many repeats, both signs, points on cell faces (multiples of the size) and empty clouds
    cloud = lambda n: (g.integers(-6, 6, (n, 4)) * np.float32(size) + g.choice([0.0, 0.0, 0.03], (n, 4))).astype(np.float32)
    clouds = [cloud(int(g.integers(0, 40))) for _ in range(K)]
    target = cloud(int(g.integers(0, 40)))
    member, hist = VO.occupancy(clouds, target, size)
    wm, wh = VO.occupancy_sets(clouds, target, size)
    assert np.array_equal(member, wm) and np.array_equal(hist, wh)
    assert hist[0, 0] == 0 and hist.sum() == len(set().union(VO.voxel_set(target, size), *[VO.voxel_set(c, size) for c in clouds]))
    i, na, nb = VO.iou_counts(clouds[0], target, size)
    assert (na, i) == tuple(member[0]) and nb == hist[1].sum()


def test_oracle_floor_and_faces():
    """floor, not truncation, and the float32 division decides at a face: on the points fl32(k * 0.1) it differs both from the division in
    float64 and from a multiplication by the reciprocal"""
    v = VO.voxels(np.array([[-0.05, 0.0, 0.05], [-0.0, -1.0, 1.0], [-1e-45, 1e-45, 0.25]], np.float32), 0.1)
    assert v.tolist() == [[-1, 0, 0], [0, -10, 10], [-1, 0, 2]]
    assert VO.keys(np.zeros((1, 3), np.float32), 1.0)[0] == (1 << 62) | (1 << 41) | (1 << 20)
    s, x = np.float32(0.1), (np.arange(-50, 51) * 0.1).astype(np.float32)
    want = VO.voxels(np.stack([x, x, x], axis=1), 0.1)[:, 0]
    assert (want != np.floor(x.astype(np.float64) / np.float64(s))).any() and (want != np.floor(x * (np.float32(1) / s))).any()
    assert np.array_equal(want, [int(np.floor(np.float32(np.float32(xi) / s))) for xi in x])


# ---- derived values --------------------------------------------------------------------------------------------------------------------------
def test_voxel_from_counts():
    d = G.voxel_from_counts(torch.tensor([[7, 7, 7], [0, 5, 9], [0, 0, 0], [3, 4, 6], [0, 0, 5], [0, 5, 0]]))
    assert all(v.dtype == torch.float64 for v in d.values()) and set(d) == set(G.VOXEL_NAMES)
    assert [d[k][0].item() for k in G.VOXEL_NAMES] == [1.0, 1.0, 1.0, 1.0]          # identical clouds
    assert [d[k][1].item() for k in G.VOXEL_NAMES] == [0.0, 0.0, 0.0, 0.0]          # disjoint clouds
    assert all(math.isnan(d[k][2].item()) for k in G.VOXEL_NAMES)                   # an empty union
    assert [d[k][3].item() for k in G.VOXEL_NAMES] == [3 / 7, 3 / 4, 3 / 6, 6 / 10]
    p, r = d["precision"][3].item(), d["recall"][3].item()
    assert abs(d["f1"][3].item() - 2 * p * r / (p + r)) < 1e-15
    assert math.isnan(d["precision"][4].item()) and d["recall"][4].item() == 0.0 and d["iou"][4].item() == 0.0  # an empty prediction
    assert math.isnan(d["recall"][5].item()) and d["precision"][5].item() == 0.0
    for bad in (torch.zeros(3, 2, dtype=torch.int64), torch.zeros(3, 3)):
        with pytest.raises(ValueError):
            G.voxel_from_counts(bad)


def hist_heads(hist, K):
    """the head values written out from a (2,K+1) histogram, python integers and one division each"""
    h = [[int(v) for v in row] for row in hist]
    div = lambda n, d: n / d if d else math.nan
    tgt, union = sum(h[1]), sum(h[0]) + sum(h[1])
    out = {"union": union, "voxels_target": tgt}
    for head, keep in (("any", lambda c: c >= 1), ("consensus", lambda c: 2 * c >= K)):
        inter = sum(h[1][c] for c in range(K + 1) if keep(c))
        pred = sum(h[0][c] + h[1][c] for c in range(K + 1) if keep(c))
        out.update({f"{head}_iou": div(inter, pred + tgt - inter), f"{head}_precision": div(inter, pred), f"{head}_recall": div(inter, tgt),
                    f"{head}_f1": div(2 * inter, pred + tgt)})
    out["brier"] = div(sum(h[0][c] * c * c + h[1][c] * (K - c) * (K - c) for c in range(K + 1)), K * K * union)
    out["reliability"] = [div(h[1][c], h[0][c] + h[1][c]) for c in range(K + 1)]
    return out


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


@pytest.mark.parametrize("K", [1, 2, 3, 4, 16, 63])
def test_occupancy_from_counts_equals_the_sums_over_hist(K):
    g = np.random.Generator(np.random.PCG64(K))
    hist = g.integers(0, 50, (3, 2, 2, K + 1))
    hist[..., 0, 0] = 0
    hist[1] = 0                      # an empty union: everything NaN
    hist[2, 0, :, K // 2:] = 0       # empty bins: a NaN in the reliability curve
    member = g.integers(0, 50, (3, 2, K, 2))
    member[..., 1] = np.minimum(member[..., 1], member[..., 0])
    d = G.occupancy_from_counts(torch.from_numpy(member), torch.from_numpy(hist))
    for i in range(3):
        for j in range(2):
            want = hist_heads(hist[i, j], K)
            for name, w in want.items():
                got = d[name][i, j].tolist()
                assert all(same(x, y) for x, y in zip(got, w)) if isinstance(w, list) else same(got, w), (name, got, w)
            tgt = want["voxels_target"]
            for k in range(K):
                a, i_k = int(member[i, j, k, 0]), int(member[i, j, k, 1])
                assert same(d["member_iou"][i, j, k].item(), (i_k / (a + tgt - i_k)) if a + tgt - i_k else math.nan)
                assert same(d["member_precision"][i, j, k].item(), i_k / a if a else math.nan)
                assert same(d["member_recall"][i, j, k].item(), i_k / tgt if tgt else math.nan)
                assert same(d["member_f1"][i, j, k].item(), 2 * i_k / (a + tgt) if a + tgt else math.nan)
    assert d["brier"][1].isnan().all() and d["any_iou"][1].isnan().all()


def test_one_member_is_the_pair():
    """K = 1: hist[1][1] is the intersection, and the Brier score is 1 - IoU; "any", "consensus" and the member are the same set"""
    for inter, only_a, only_b in ((5, 3, 2), (4, 0, 0), (0, 3, 6), (0, 0, 0)):
        hist = torch.tensor([[0, only_a], [only_b, inter]])
        member = torch.tensor([[inter + only_a, inter]])
        d = G.occupancy_from_counts(member, hist)
        pair = G.voxel_from_counts(torch.tensor([inter, inter + only_a, inter + only_b]))
        for name in G.VOXEL_NAMES:
            assert same(d[f"any_{name}"].item(), pair[name].item()) and same(d[f"consensus_{name}"].item(), pair[name].item())
            assert same(d[f"member_{name}"][0].item(), pair[name].item())
        union = inter + only_a + only_b
        assert same(d["brier"].item(), (only_a + only_b) / union if union else math.nan)
        if union:
            assert d["brier"].item() == 1 - pair["iou"].item() or abs(d["brier"].item() - (1 - pair["iou"].item())) < 2 ** -52
    with pytest.raises(ValueError):
        G.occupancy_from_counts(torch.zeros(2, 2, dtype=torch.int64), torch.zeros(2, 2, dtype=torch.int64))
    with pytest.raises(ValueError):
        G.occupancy_from_counts(torch.zeros(1, 2), torch.zeros(2, 2))


def test_aggregates():
    counts = torch.tensor([[[3, 4, 6], [2, 2, 4]], [[0, 0, 0], [0, 0, 0]], [[1, 5, 2], [1, 1, 1]]])
    agg = G.aggregate_voxel(counts, (0.1, 0.5))
    assert (agg["scans"], agg["empty"]) == (3, 1) and agg["sizes"] == [float(np.float32(0.1)), 0.5]
    assert agg["micro"]["iou"] == [4 / (9 + 8 - 4), 3 / (3 + 5 - 3)] and agg["micro"]["precision"] == [4 / 9, 3 / 3]
    assert agg["macro"]["iou"] == [(3 / 7 + 1 / 6) / 2, (2 / 4 + 1 / 1) / 2]
    none = G.aggregate_voxel(torch.zeros(0, 2, 3, dtype=torch.int64), (0.1, 0.5))
    assert none["scans"] == 0 and all(math.isnan(v) for v in none["micro"]["iou"] + none["macro"]["f1"])

    hist = torch.tensor([[[[0, 2, 1], [1, 1, 3]]], [[[0, 4, 0], [0, 0, 0]]], [[[0, 0, 1], [2, 0, 1]]]])      # (3,1,2,3): K = 2, scan 1 has no target voxels
    member = torch.tensor([[[[5, 3], [4, 4]]], [[[2, 0], [2, 0]]], [[[2, 1], [2, 1]]]])
    agg = G.aggregate_occupancy(member, hist, [0.2])
    assert (agg["scans"], agg["empty"], agg["members"]) == (3, 1, 2) and agg["hist"] == [[[0, 2, 2], [3, 1, 4]]]
    total = hist_heads(np.array(agg["hist"][0]), 2)
    assert agg["micro"]["brier"] == [total["brier"]] and agg["micro"]["consensus_iou"] == [total["consensus_iou"]]
    assert agg["micro"]["reliability"] == [total["reliability"]]
    per = [hist_heads(hist[i, 0].numpy(), 2) for i in (0, 2)]
    assert agg["macro"]["brier"] == [(per[0]["brier"] + per[1]["brier"]) / 2]
    assert agg["macro"]["reliability"][0][1] == per[0]["reliability"][1]  # (scan 2 has no voxel with c = 1: the mean of the defined ones)
    assert agg["micro"]["member_iou"] == [[4 / (7 + 8 - 4), 5 / (6 + 8 - 5)]]


def test_python_refusals():
    for bad in ((), [0.0], [-0.1], [math.nan], [math.inf], [1e-50], [0.1] * 9, "x", [[0.1]]):
        with pytest.raises(ValueError, match="voxel sizes"):
            G._voxel_sizes(bad)
    assert G._voxel_sizes(0.1).tolist() == [np.float32(0.1)] and G._voxel_sizes((0.1, 0.2)).dtype == np.float32
    for K in (0, 64):
        with pytest.raises(ValueError, match="63"):
            G._check_members(K)
    for bad in (lambda: G._group_indices([0, 1], [0, 1]), lambda: G._group_indices([[0.5]], [0]), lambda: G._group_indices([[0], [1]], [0]),
                lambda: G._group_indices([[0]], [[0]]), lambda: G._group_indices(np.zeros((2, 0), np.int64), [0, 0])):
        with pytest.raises(ValueError, match="members|targets"):
            bad()
    with pytest.raises(ValueError, match="63"):
        G._group_indices(np.zeros((1, 64), np.int64), [0])
    assert [G._voxel_capacity(n) for n in (1, 2, 3, 4, 5, 4096, 4097)] == [2, 4, 8, 8, 16, 8192, 16384]


# ---- the C entry -----------------------------------------------------------------------------------------------------------------------------
def test_c_abi_refuses_bad_arguments_with_a_status():
    """Every refusal is a status and a message, decided before anything touches a GPU (the device pointers here are made-up addresses)."""
    from r2dm_amd import _lib

    L = _lib.lib()
    sizes = (ctypes.c_float * 9)(0.1, 0.2, 0.5, 1, 1, 1, 1, 1, 1)
    base = dict(a=4096, a_offsets=8192, a_clouds=2, a_total=100, b=12288, b_offsets=16384, b_clouds=2, b_total=100, members=20480, targets=24576, G=2, K=1,
                sizes=sizes, S=3, max_group_points=200, scratch=28672, member_out=32768, hist_out=36864, status=40960)

    def vox(**kw):
        return L.r2dm_voxel_occupancy(*{**base, **kw}.values(), None), L.r2dm_last_error().decode()

    for null in ("a_offsets", "b_offsets", "members", "targets", "sizes", "scratch", "member_out", "hist_out", "status"):
        rc, msg = vox(**{null: None})
        assert rc == 1 and "null argument" in msg, null
    for kw in (dict(a=None), dict(b=None), dict(a_clouds=0), dict(b_clouds=-1), dict(a_total=-1)):
        rc, msg = vox(**kw)
        assert rc == 1 and "at least one cloud" in msg, kw
    for kw in (dict(G=0), dict(K=0), dict(S=0), dict(G=-1)):
        rc, msg = vox(**kw)
        assert rc == 1 and "must be >= 1" in msg, kw
    rc, msg = vox(K=64)
    assert rc == 1 and "at most 63 members" in msg and "bit 63" in msg
    rc, msg = vox(S=9)
    assert rc == 1 and "at most 8 voxel sizes" in msg
    for value in (0.0, -0.1, math.nan, math.inf):
        rc, msg = vox(sizes=(ctypes.c_float * 3)(0.1, value, 0.5))
        assert rc == 1 and "finite and > 0" in msg, value
    for kw in (dict(max_group_points=0), dict(max_group_points=(1 << 27) + 1), dict(G=65536), dict(G=1 << 10, S=8, max_group_points=1 << 27)):
        rc, msg = vox(**kw)
        assert rc == 1 and "2^36 slots" in msg, kw
    for name in ("a", "b", "scratch"):
        rc, msg = vox(**{name: 4096 + 8})
        assert rc == 1 and "16-byte aligned" in msg, name
    for name in ("a_offsets", "b_offsets", "members", "targets", "member_out", "hist_out", "status"):
        rc, msg = vox(**{name: 8192 + 4})
        assert rc == 1 and "8-byte aligned" in msg, name

    f = L.r2dm_voxel_occupancy_scratch_bytes
    for empty in ((0, 1, 64), (-1, 1, 64), (1, 0, 64), (1, 9, 64), (1, 1, 0), (1, 1, (1 << 27) + 1), (65536, 1, 1), (1 << 10, 8, 1 << 27)):
        assert f(*empty) == 0, empty
    # per group and size 16 bytes per slot of a table of the power of two >= 2 * max_group_points slots, and one 8-byte flag per group (rounded to 16)
    assert f(1, 1, 1) == 16 + 2 * 16 and f(1, 1, 4096) == 16 + 8192 * 16 and f(1, 1, 4097) == 16 + 16384 * 16
    assert f(3, 2, 100) == 32 + 3 * 2 * 256 * 16 and f(1, 8, 1 << 27) == 16 + 8 * (1 << 28) * 16 and f(65535, 8, 1) > 0
    for n in (1, 3, 100, 5000):
        assert f(1, 1, n) == 16 + 16 * G._voxel_capacity(n)


# ---- the options ---------------------------------------------------------------------------------------------------------------------------
def test_voxel_sizes_are_off_by_default_and_checked_before_the_gpu():
    import completion_eval
    from r2dm_amd.completion import evaluate_completion

    assert inspect.signature(evaluate_completion).parameters["voxel_sizes"].default is None
    assert inspect.signature(G.voxel_iou).parameters["sizes"].default == (0.1,)
    a = completion_eval.build_parser().parse_args(["--ckpt", "m.pth", "--real_scans", "d"])
    assert not hasattr(a, "voxel_iou")
    a = completion_eval.build_parser().parse_args(["--ckpt", "m.pth", "--real_scans", "d", "--voxel_iou", "0.1", "0.2", "--ensemble", "4"])
    assert a.voxel_iou == [0.1, 0.2] and a.ensemble == 4
    src = inspect.getsource(completion_eval.main)
    assert 'if hasattr(args, "voxel_iou"):\n        info["voxel_sizes"]' in src  # (the only new key of the document's info, and only when asked for)

    planes = torch.zeros(1, 6, 4, 8)  # on the CPU: reaching the GPU check would raise R2DMError instead
    with pytest.raises(ValueError, match="63"):
        evaluate_completion(None, None, planes, ["beams:4"], methods=("target",), voxel_sizes=(0.2, 0.5), ensemble=64)
    with pytest.raises(ValueError, match="voxel sizes"):
        evaluate_completion(None, None, planes, ["beams:4"], methods=("target",), voxel_sizes=(0.2, -0.5))
    from r2dm_amd._lib import R2DMError
    with pytest.raises(R2DMError):  # 63 members pass the check and stop at the next one
        evaluate_completion(None, None, planes, ["beams:4"], methods=("target",), voxel_sizes=(0.2, 0.5), ensemble=63)
    with pytest.raises(R2DMError, match="no CPU fallback"):
        G.voxel_iou(torch.zeros(4, 4), [0, 4], torch.zeros(4, 4), [0, 4])
