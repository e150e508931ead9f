"""The completion metrics' host side, without a GPU: corruption masks, IoU from a confusion matrix, the aggregation over scans, the
JSON document, the command line's flags, the refusal of CPU tensors and the C ABI's argument checks.

Tolerances: the masks, counts and the IoU of hand-written integer tables are exact.  The aggregation is compared with the same float64
expressions written out by hand (one division, one square root): equal to 1e-15 relative, two roundings of 2^-53."""
import json
import math

import numpy as np
import pytest
import torch

import completion_oracle as O


def test_mask_kinds():
    from r2dm_amd.completion import corruption_mask, parse_kind

    H, W = 16, 128
    want = torch.zeros(1, H, W)
    want[:, ::4] = 1
    m = corruption_mask("beams:4", H, W)
    assert m.shape == (1, H, W) and m.dtype == torch.float32 and m.device.type == "cpu" and torch.equal(m, want)
    assert torch.equal(corruption_mask("full", H, W), torch.ones(1, H, W))
    assert torch.equal(corruption_mask("beams:1", H, W), torch.ones(1, H, W))
    assert corruption_mask("beams:5", 7, 3)[0, :, 0].tolist() == [1, 0, 0, 0, 0, 1, 0]
    for kind, shape in (("random_beams:0.5", (H, 1)), ("random_points:0.1", (H, W))):
        a = corruption_mask(kind, H, W, torch.Generator().manual_seed(11))
        b = corruption_mask(kind, H, W, torch.Generator().manual_seed(11))
        c = corruption_mask(kind, H, W, torch.Generator().manual_seed(12))
        assert torch.equal(a, b) and not torch.equal(a, c) and set(a.unique().tolist()) <= {0.0, 1.0}
        # the demo's draw in the demo's shape
        assert torch.equal(a[0], torch.empty(*shape).bernoulli_(float(kind.split(":")[1]), generator=torch.Generator().manual_seed(11)).expand(H, W))
    rb = corruption_mask("random_beams:0.5", H, W, torch.Generator().manual_seed(3))
    assert ((rb[0] == rb[0, :, :1]).all())  # whole rows
    assert torch.equal(corruption_mask("random_points:0", H, W), torch.zeros(1, H, W))
    assert torch.equal(corruption_mask("random_beams:1", H, W), torch.ones(1, H, W))
    assert parse_kind("beams:4") == ("beams", 4) and parse_kind("full") == ("full", None) and parse_kind("random_points:0.25") == ("random_points", 0.25)
    for bad in ("", "beams", "beams:", "beams:0", "beams:-2", "beams:x", "beams:2.5", "full:1", "random_beams", "random_beams:1.5", "random_points:-0.1",
                "random_points:p", "points:0.1", "Beams:4", None):
        with pytest.raises(ValueError, match="malformed corruption"):
            corruption_mask(bad, H, W)
    with pytest.raises(ValueError):
        corruption_mask("full", 0, 4)


def test_the_demo_masks_are_unchanged():
    import completion_demo
    from r2dm_amd.completion import corruption_mask

    H, W = 16, 128
    for seed in (0, 3):
        got = completion_demo.corruption_masks(torch.zeros(1, 2, H, W), seed)
        torch.manual_seed(seed)
        want = torch.zeros(4, 2, H, W)
        want[0, ...] = 1
        want[1, :, ::4] = 1
        want[2, :] = torch.empty(H, 1).bernoulli_(0.5)
        want[3, :] = torch.empty(H, W).bernoulli_(0.1)
        assert torch.equal(got, want)
        assert torch.equal(got[1, :1], corruption_mask("beams:4", H, W))


def test_scan_seeds_are_distinct_and_checked():
    from r2dm_amd.completion import scan_seed

    assert scan_seed(0, 0) == 0 and scan_seed(0, 5) == 5 and scan_seed(2, 5) == 2 * 2 ** 32 + 5
    assert len({scan_seed(s, i) for s in range(4) for i in range(100)}) == 400
    for bad in ((-1, 0), (0, -1), (2 ** 31, 0), (0, 2 ** 32)):
        with pytest.raises(ValueError):
            scan_seed(*bad)


def test_iou_from_a_hand_written_table():
    from r2dm_amd.completion import iou_from_confusion

    #            pred: 0  1  2  3
    conf = torch.tensor([[5, 7, 0, 0],    # target 0 (ignored: the whole row leaves)
                         [1, 6, 2, 0],    # target 1
                         [2, 2, 4, 0],    # target 2
                         [0, 0, 0, 0]])   # target 3: absent, and never predicted
    iou, miou = iou_from_confusion(conf)
    # class 1: tp 6, fn 1 + 2, fp 2 (the 7 predicted on an ignored target do not count) -> 6 / 11; class 2: tp 4, fn 4, fp 2 -> 4 / 10
    assert iou.dtype == torch.float64 and math.isnan(iou[0]) and math.isnan(iou[3])
    assert iou[1].item() == 6 / 11 and iou[2].item() == 4 / 10 and abs(miou - (6 / 11 + 4 / 10) / 2) < 1e-15
    per, m = O.iou(conf.numpy())
    assert np.array_equal(per, iou.numpy(), equal_nan=True) and abs(m - miou) < 1e-15
    # nothing ignored: class 0 counts, tp 5, fn 7, fp 3
    iou, miou = iou_from_confusion(conf, ignore=())
    assert iou[0].item() == 5 / 15 and iou[1].item() == 6 / 18 and math.isnan(iou[3]) and abs(miou - (5 / 15 + 6 / 18 + 4 / 10) / 3) < 1e-15
    # all correct: exactly 1
    iou, miou = iou_from_confusion(torch.diag(torch.tensor([9, 3, 0, 12])))
    assert iou[1].item() == 1.0 and iou[3].item() == 1.0 and math.isnan(iou[2]) and math.isnan(iou[0]) and miou == 1.0
    # a batch of tables is summed; a class only ever predicted has IoU 0
    iou, miou = iou_from_confusion(torch.stack([conf, conf.flip(1)]), ignore=(0,))
    total = (conf + conf.flip(1)).numpy()
    assert np.array_equal(iou.numpy(), O.iou(total)[0], equal_nan=True) and iou[3].item() == 0.0
    # nothing left: NaN, not an error
    iou, miou = iou_from_confusion(torch.zeros(4, 4, dtype=torch.int64))
    assert iou.isnan().all() and math.isnan(miou)
    with pytest.raises(ValueError):
        iou_from_confusion(torch.zeros(3, 4))
    with pytest.raises(ValueError):
        iou_from_confusion(conf, ignore=(4,))


def test_aggregation_micro_against_macro():
    from r2dm_amd.completion import aggregate_errors, derived_errors

    #                    |U|  |E| |Bo| fr   abs    sq   absB   sqB   absR   sqR
    raw = torch.tensor([[100, 50, 40, 5, 25.0, 100.0, 8.0, 10.0, 5.0, 1.0],
                        [300, 10, 10, 0, 30.0, 250.0, 30.0, 250.0, 2.0, 0.5],
                        [0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]], dtype=torch.float64)  # (a scan with nothing to fill in)
    a = aggregate_errors(raw)
    assert a["counts"] == {"scans": 3, "unknown": 400, "evaluated": 60, "both": 50, "false_returns": 5, "unknown_without_return": 340}
    assert a["sums"]["abs_depth"] == 55.0 and a["sums"]["sq_reflectance"] == 1.5
    close = lambda x, y: abs(x - y) <= 1e-15 * abs(y)
    assert close(a["micro"]["mae_depth"], 55 / 60) and close(a["micro"]["rmse_depth"], math.sqrt(350 / 60))
    assert close(a["micro"]["mae_depth_both"], 38 / 50) and close(a["micro"]["rmse_depth_both"], math.sqrt(260 / 50))
    assert close(a["micro"]["mae_reflectance"], 7 / 60) and close(a["micro"]["return_recall"], 50 / 60)
    assert close(a["micro"]["false_return_rate"], 5 / 340)
    # macro: the mean over the scans that define the value (the third has none)
    assert close(a["macro"]["mae_depth"], (25 / 50 + 30 / 10) / 2) and close(a["macro"]["rmse_depth"], (math.sqrt(2) + 5) / 2)
    assert close(a["macro"]["return_recall"], (0.8 + 1.0) / 2) and close(a["macro"]["false_return_rate"], (5 / 50 + 0 / 290) / 2)
    assert a["macro"]["mae_depth"] != a["micro"]["mae_depth"]
    d = derived_errors(raw)
    assert all(v.shape == (3,) and v.dtype == torch.float64 and math.isnan(v[2]) for v in d.values())
    want = O.derived(raw.numpy())
    assert set(want) == set(d) and all(np.allclose(want[k], d[k].numpy(), rtol=1e-15, atol=0, equal_nan=True) for k in d)


def test_a_zero_denominator_is_null_in_the_json():
    from r2dm_amd.completion import DERIVED_NAMES, aggregate_errors, jsonable

    a = aggregate_errors(torch.zeros(2, 10, dtype=torch.float64))  # the "full" corruption: nothing unknown
    assert a["counts"]["evaluated"] == 0 and all(math.isnan(a[g][n]) for g in ("micro", "macro") for n in DERIVED_NAMES)
    doc = {"results": {"full": {"repaint": dict(a, iou={"per_class": torch.tensor([math.nan, 0.5]), "miou": math.nan})}}, "n": (1, math.inf)}
    text = json.dumps(jsonable(doc), allow_nan=False)
    assert "NaN" not in text and "Infinity" not in text
    back = json.loads(text)
    entry = back["results"]["full"]["repaint"]
    assert all(entry[g][n] is None for g in ("micro", "macro") for n in DERIVED_NAMES)
    assert entry["iou"] == {"per_class": [None, 0.5], "miou": None} and back["n"] == [1, None] and entry["counts"]["scans"] == 2
    # no scan at all
    assert aggregate_errors(torch.zeros(0, 10))["counts"]["scans"] == 0


def test_parser_flags():
    import completion_eval

    p = completion_eval.build_parser()
    a = p.parse_args(["--ckpt", "m.pth", "--real_scans", "d"])
    assert (a.corruption, a.methods, a.num_steps, a.num_resample_steps, a.jump_length) == (None, ["repaint"], 32, 10, 1)
    assert (a.limit, a.seed, a.rangenet_weights, a.semseg_postprocess, a.save_dir, a.real_dir) == (None, 0, None, "none", None, None)
    a = p.parse_args(["--ckpt", "m.pth", "--real_dir", "d", "--limit", "5", "--corruption", "beams:4", "--corruption", "random_points:0.1",
                      "--methods", "repaint", "nearest", "linear", "--num_steps", "8", "--num_resample_steps", "2", "--jump_length", "3",
                      "--batch_size", "4", "--seed", "7", "--rangenet_weights", "w.tar.gz", "--semseg_postprocess", "crf_knn", "--save_dir", "s",
                      "--out", "o.json"])
    assert a.corruption == ["beams:4", "random_points:0.1"] and a.methods == ["repaint", "nearest", "linear"] and str(a.save_dir) == "s"
    assert (a.limit, a.num_steps, a.num_resample_steps, a.jump_length, a.batch_size, a.seed, a.out) == (5, 8, 2, 3, 4, 7, "o.json")
    for bad in (["--ckpt", "m.pth", "--methods", "cubic"], ["--ckpt", "m.pth", "--semseg_postprocess", "median"], ["--real_dir", "d"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(SystemExit, match="one of --real_scans"):
        completion_eval.main(["--ckpt", "m.pth"])
    with pytest.raises(ValueError, match="malformed corruption"):
        completion_eval.main(["--ckpt", "m.pth", "--real_dir", "d", "--corruption", "beams"])


def test_cpu_tensors_raise():
    import r2dm_amd
    from r2dm_amd._lib import R2DMError

    img, known = torch.zeros(1, 5, 4, 8), torch.zeros(1, 1, 4, 8)
    lab = torch.zeros(1, 32, dtype=torch.int64)
    for call in (lambda: r2dm_amd.completion_errors(img, img, known, 1.0, 80.0),
                 lambda: r2dm_amd.confusion_matrix(lab, lab, 4),
                 lambda: r2dm_amd.fill_beams(torch.zeros(1, 2, 4, 8), torch.ones(1, 4), "linear"),
                 lambda: r2dm_amd.evaluate_completion(None, None, torch.zeros(1, 6, 4, 8), ["full"])):
        with pytest.raises(R2DMError, match="no CPU fallback"):
            call()
    # what is wrong with the arguments themselves is said first
    with pytest.raises(ValueError):
        r2dm_amd.fill_beams(torch.zeros(1, 2, 4, 8), torch.ones(1, 4), "cubic")
    with pytest.raises(ValueError):
        r2dm_amd.evaluate_completion(None, None, torch.zeros(1, 5, 4, 8), ["full"])


def _abi():
    from r2dm_amd import _lib

    return _lib.lib()


def test_c_abi_refuses_bad_arguments_with_a_status():
    """Every refusal is a status and a message, decided before anything touches a GPU (the pointers here are made-up addresses)."""
    L = _abi()

    def err(pred=4096, target=8192, known=12288, B=2, plane=64, scratch=16384, out=20480):
        return L.r2dm_completion_error(pred, target, known, 1.0, 80.0, B, plane, scratch, out, None), L.r2dm_last_error().decode()

    for null in ("pred", "target", "known", "scratch", "out"):
        rc, msg = err(**{null: None})
        assert rc == 1 and "null argument" in msg, null
    for name in ("pred", "target", "known"):
        rc, msg = err(**{name: 4096 + 4})
        assert rc == 1 and "16-byte aligned" in msg, name
        rc, msg = err(**{name: 4096 + 2}, plane=63)
        assert rc == 1 and "4-byte aligned" in msg, name
    for name in ("scratch", "out"):
        rc, msg = err(**{name: 16384 + 4})
        assert rc == 1 and "8-byte aligned" in msg, name
    for geometry in (dict(B=0), dict(B=-1), dict(B=65536), dict(plane=0), dict(plane=-4), dict(plane=1 << 41)):
        rc, msg = err(**geometry)
        assert rc == 1 and "batch must be in" in msg, geometry

    def conf(pred=4096, target=8192, mask=None, B=2, pixels=64, classes=20, counts=16384, bad=20480):
        return L.r2dm_confusion_matrix(pred, target, mask, B, pixels, classes, counts, bad, None), L.r2dm_last_error().decode()

    for null in ("pred", "target", "counts", "bad"):
        rc, msg = conf(**{null: None})
        assert rc == 1 and "null argument" in msg, null
    for classes in (0, -1, 65):
        rc, msg = conf(classes=classes)
        assert rc == 1 and "classes must be in [1, 64]" in msg
    for geometry in (dict(B=0), dict(B=65536), dict(pixels=0), dict(pixels=1 << 41)):
        rc, msg = conf(**geometry)
        assert rc == 1 and "batch must be in" in msg, geometry
    for name in ("pred", "target", "counts", "bad"):
        rc, msg = conf(**{name: 4096 + 4})
        assert rc == 1 and "8-byte aligned" in msg, name
    rc, msg = conf(mask=4096 + 2)
    assert rc == 1 and "mask 4-byte aligned" in msg

    def fill(x=4096, rows=8192, out=12288, B=2, C=2, H=16, W=128, mode=0):
        return L.r2dm_fill_beams(x, rows, out, B, C, H, W, -1.0, mode, None), L.r2dm_last_error().decode()

    for null in ("x", "rows", "out"):
        rc, msg = fill(**{null: None})
        assert rc == 1 and "null argument" in msg, null
    for mode in (-1, 2):
        rc, msg = fill(mode=mode)
        assert rc == 1 and "mode must be 0 (nearest) or 1 (linear)" in msg
    for geometry in (dict(B=0), dict(B=65536), dict(H=0), dict(H=65536), dict(C=0), dict(W=0), dict(C=1 << 20, W=1 << 20)):
        rc, msg = fill(**geometry)
        assert rc == 1 and "batch and height must be in" in msg, geometry
    rc, msg = fill(x=4096 + 2)
    assert rc == 1 and "4-byte aligned" in msg
    rc, msg = fill(out=4096)
    assert rc == 1 and "must not alias" in msg


def test_error_scratch_bytes():
    f = _abi().r2dm_completion_error_scratch_bytes
    for empty in ((0, 2048), (-1, 2048), (2, 0), (2, -5), (65536, 64), (2, 1 << 41)):
        assert f(*empty) == 0, empty
    assert f(1, 1) == 80  # one block of ten doubles
    planes = [1, 3, 4, 35, 1023, 1024, 1025, 2048, 16 * 1024, 16 * 1024 + 1, 65536, 1 << 24]
    for B in (1, 2, 7):
        sizes = [f(B, p) for p in planes]
        assert all(s > 0 and s % 80 == 0 for s in sizes) and sizes == sorted(sizes)
        assert all(f(B, p) == B * f(1, p) for p in planes)  # the blocks of a sample depend on the plane alone
    assert f(8, 65536) == f(8, 1 << 24)  # the grid is capped


def test_the_oracle_on_hand_worked_cases():
    """The specification itself, on cases small enough to work out by hand."""
    x = np.array([[1.0, -1.0, 2.0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [4.0, -1.0, 8.0]], np.float32)  # (H,W) = (5,3)
    x = np.stack([x, 10 * x])[None]  # (1,2,5,3)
    rows = np.array([[1, 0, 0, 0, 1]])
    lin, near = O.fill(x, rows, "linear"), O.fill(x, rows, "nearest")
    assert lin[0, 0, :, 0].tolist() == [1.0, 1.75, 2.5, 3.25, 4.0] and lin[0, 1, 2, 2] == 50.0
    assert lin[0, :, 1:4, 1].tolist() == [[-1.0] * 3] * 2  # both endpoints carry nodata in channel 0
    assert near[0, 0, :, 0].tolist() == [1.0, 1.0, 1.0, 4.0, 4.0]  # row 2 is a tie: the upper one
    one = O.fill(x, np.array([[0, 0, 1, 0, 0]]), "linear")
    assert (one[0, :, :, 0] == x[0, :, 2:3, 0]).all() and (O.fill(x, np.zeros((1, 5)), "nearest") == -1).all()
    pred = np.zeros((1, 5, 1, 4), np.float32)
    target = np.zeros((1, 5, 1, 4), np.float32)
    target[0, 0, 0], pred[0, 0, 0] = [10, 20, 0, np.nan], [12, 0, 5, 7]
    target[0, 4, 0], pred[0, 4, 0] = [0.5, 0.25, 0, 0], [0.25, 0.75, 1, 1]
    raw = O.error_sums(pred, target, np.zeros((1, 1, 1, 4), np.float32), 1.0, 80.0)[0]
    assert raw.tolist() == [4, 2, 1, 2, 2 + 20, 4 + 400, 2, 4, 0.25 + 0.5, 0.0625 + 0.25]
    assert (O.error_sums(pred, target, np.ones((1, 1, 1, 4), np.float32), 1.0, 80.0) == 0).all()
    c = O.confusion(np.array([[0, 1, 1, 5]]), np.array([[0, 1, 0, -3]]), 2, np.array([[1, 1, 2, 0]]))
    assert c.tolist() == [[[1, 1], [0, 1]]]
