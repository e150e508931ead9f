"""-m gpu: the completion metrics (r2dm_amd/csrc/completion.hip, r2dm_amd/completion.py, completion_eval.py) against the plain
numpy / float64 specifications of tests/completion_oracle.py.

Tolerances (stated, derived from the number formats, not from the code under test):
  * error kernel, the four counts: exact (integers below 2^53 in float64).
  * error kernel, the six sums: relative 1e-10 of the oracle.  Kernel and oracle widen the same float32 values to float64, so every
    difference is exact in both; what remains is one rounding per square and one per addition, in whatever order: at most n * 2^-53
    relative for sums of non-negative terms, with n <= 2^16 pixels here about 7e-12.  1e-10 leaves a margin above 10.
  * a sum that is zero in the oracle (no pixel in its set, or identical prediction and target) is an exact zero.
  * confusion matrix: exact equality with ``np.bincount`` (integer atomics, no order dependence).
  * fill_beams: bit for bit in both modes -- the linear mode is three float32 operations (subtract, multiply by t = float(h - up) /
    float(dn - up), add) with one IEEE rounding each and no contraction, which ``np.float32`` arithmetic reproduces exactly.
  * end to end: every reported number is recomputed by the oracle from the tensors the script saved and held to the same bars; a derived
    value is a ratio of an exact count and a sum within 1e-10 (and a square root, which halves a relative error), a macro average a
    mean of at most two such values: 1e-10 again.  This does not depend on what RePaint produces.
"""
import json
import math
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, GOLDEN_RES, ROOT, synthetic_ckpt

sys.path.insert(0, GOLDEN)
import make_golden_projection as G  # noqa: E402  (read-only: the integer-only generator of the free cloud)

import completion_oracle as O  # noqa: E402
import r2dm_amd  # noqa: E402
from r2dm_amd import completion, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
LO, HI = 1.45, 80.0
SUM_BAR = 1e-10
ERROR_SHAPES = ((1, 1, 1), (3, 5, 7), (2, 16, 128), (1, 64, 1024))


# ---- 1. the error kernel -----------------------------------------------------------------------------------------------------------------
def error_inputs(B, H, W):
    """pred, target (B,5,H,W) and known (B,1,H,W) as numpy float32, built to reach every set: sample 0 of a batch all known, sample 1 all
    unknown, the others a random half; target depths equal to lo, to hi, 0 and NaN; predictions outside the window and NaN on measured
    pixels; a NaN reflectance where the target has no return (it must stay outside every sum)."""
    g = np.random.Generator(np.random.PCG64(1000 * B + 10 * H + W))
    n = H * W
    target = g.uniform(0.0, 1.0, (B, 5, n)).astype(np.float32)
    target[:, 0] = g.uniform(0.5, 90.0, (B, n)).astype(np.float32)
    pred = target + g.normal(0, 0.3, (B, 5, n)).astype(np.float32)
    known = (g.uniform(size=(B, 1, n)) < 0.5).astype(np.float32)
    known[-1, 0, 0] = 0
    if B > 1:
        known[0], known[1] = 1, 0
    if n >= 32:
        for b in range(B):
            where = g.permutation(n)
            t_special, p_special = where[:8], where[8:16]
            target[b, 0, t_special] = np.array([LO, HI, 0, np.nan] * 2, np.float32)
            target[b, 4, t_special[3::4]] = np.nan
            pred[b, 4, t_special[3::4]] = np.nan
            pred[b, 0, t_special] = np.array([5.0, 6.0, 7.0, 8.0, LO, 0.0, np.nan, 100.0], np.float32)  # four returns where the scan has none
            pred[b, 0, p_special] = np.array([0.0, 100.0, np.nan, -3.0, LO, HI, np.inf, 1.0], np.float32)
            target[b, 0, p_special] = g.uniform(2.0, 70.0, 8).astype(np.float32)  # measured pixels
            known[b, 0, p_special[:6]] = 0 if b != 0 or B == 1 else 1
            known[b, 0, t_special[:6]] = 0 if b != 0 or B == 1 else 1
    shape = lambda a, c: np.ascontiguousarray(a.reshape(B, c, H, W))
    return shape(pred, 5), shape(target, 5), shape(known, 1)


def run_errors(pred, target, known):
    dev = lambda a: torch.from_numpy(a).to(DEV)
    return completion.completion_error_sums(dev(pred), dev(target), dev(known), LO, HI).cpu().numpy()


def check_against_oracle(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float64
    print(what, "got", got.tolist(), "want", want.tolist())
    assert np.isfinite(want).all() and np.array_equal(got[..., :4], want[..., :4]), what
    zero = want == 0
    assert (got[zero] == 0).all(), what
    rel = np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero])
    assert (rel <= SUM_BAR).all(), (what, rel.max())


@pytest.mark.parametrize("shape", ERROR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_error_kernel_against_the_float64_oracle(shape):
    pred, target, known = error_inputs(*shape)
    got, want = run_errors(pred, target, known), O.error_sums(pred, target, known, LO, HI)
    check_against_oracle(got, want, shape)
    assert np.array_equal(run_errors(pred, target, known), got)  # two calls, the same bits
    if shape[1] * shape[2] >= 32:  # every set is reached
        assert (want[-1, :4] > 0).all() and want[-1, 1] > want[-1, 2] and (want[-1, 4:] > 0).all()
    # identical prediction and target (NaNs included): every error sum is exactly 0, the counts stay
    same = run_errors(target, target, known)
    check_against_oracle(same, O.error_sums(target, target, known, LO, HI), (shape, "identical"))
    assert (same[:, 4:] == 0).all() and np.array_equal(same[:, 2], same[:, 1]) and (same[:, 3] == 0).all()


def test_error_kernel_all_known_all_unknown_and_batch_independence():
    B, H, W = ERROR_SHAPES[1]
    pred, target, known = error_inputs(B, H, W)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    out = completion.completion_errors(dev(pred), dev(target), dev(known), LO, HI)
    assert set(out) == set(completion.RAW_NAMES) | set(completion.DERIVED_NAMES)
    assert all(v.shape == (B,) and v.dtype == torch.float64 for v in out.values())
    raw = torch.stack([out[k] for k in completion.RAW_NAMES], 1).cpu().numpy()
    # sample 0: everything known -> ten exact zeros, every derived value NaN (and no exception)
    assert (raw[0] == 0).all() and all(math.isnan(out[k][0].item()) for k in completion.DERIVED_NAMES)
    # sample 1: everything unknown
    assert raw[1, 0] == H * W and raw[1, 1] > 0 and all(math.isfinite(out[k][1].item()) for k in completion.DERIVED_NAMES)
    want = O.derived(O.error_sums(pred, target, known, LO, HI))
    for k in completion.DERIVED_NAMES:
        assert np.allclose(out[k].cpu().numpy(), want[k], rtol=SUM_BAR, atol=0, equal_nan=True), k
    # every sample alone returns the bits it has in the batch; so does it in the larger shapes (several blocks per sample)
    for shape in (ERROR_SHAPES[1], ERROR_SHAPES[2]):
        pred, target, known = error_inputs(*shape)
        whole = run_errors(pred, target, known)
        for b in range(shape[0]):
            assert np.array_equal(run_errors(pred[b:b + 1], target[b:b + 1], known[b:b + 1])[0], whole[b]), (shape, b)


# ---- 2. the confusion matrix -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", (1, 7, 2048, 65536))
@pytest.mark.parametrize("C", (1, 20, 33, 64))
def test_confusion_matrix_equals_bincount(C, P):
    B = 3
    g = np.random.Generator(np.random.PCG64(100 * C + P % 97))
    pred, target = g.integers(0, C, (B, P)), g.integers(0, C, (B, P))
    pred[1], target[1] = C - 1, C - 1  # one cell takes every pixel of sample 1: contention on one LDS counter, labels at C - 1
    if P > 1:
        pred[1, 0] = 0
    mask = (g.uniform(size=(B, P)) < 0.7).astype(np.float32) * g.choice(np.array([1.0, 0.5, 3.0], np.float32), (B, P))
    mask[2] = 0  # a sample with nothing to count
    mask[0, 0] = 1
    dev = lambda a: torch.from_numpy(a).to(DEV)
    got = completion.confusion_matrix(dev(pred), dev(target), C)
    assert got.shape == (B, C, C) and got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), O.confusion(pred, target, C))
    assert got.sum().item() == B * P
    # labels outside [0, C) behind mask 0 are ignored
    bad_p, bad_t = pred.copy(), target.copy()
    bad_p[2, 0], bad_t[2, P - 1] = C, -1
    n_bad = 1 if P == 1 else 2
    hidden = np.where(mask != 0, 1, 0)
    if P > 1:
        off = np.argwhere(mask[0] == 0).ravel()[:2]
        bad_p[0, off[:1]], bad_t[0, off[1:]] = 2 ** 40, -2 ** 40
        n_bad += len(off)
    got_m = completion.confusion_matrix(dev(bad_p), dev(bad_t), C, dev(mask))
    want_m = O.confusion(pred, target, C, mask)
    assert np.array_equal(got_m.cpu().numpy(), want_m) and (want_m[2] == 0).all() and want_m.sum() == hidden.sum()
    # the same labels unmasked: an error that says how many, and the next call is clean
    with pytest.raises(ValueError, match=rf"^confusion_matrix: {n_bad} unmasked pixels carry a label outside \[0, {C}\)"):
        completion.confusion_matrix(dev(bad_p), dev(bad_t), C)
    again = completion.confusion_matrix(dev(pred).reshape(B, 1, P), dev(target).reshape(B, 1, P), C, dev(mask).reshape(B, 1, P))
    assert np.array_equal(again.cpu().numpy(), want_m)


# ---- 3. the interpolation baselines ------------------------------------------------------------------------------------------------------
def fill_case(name):
    """x (B,C,H,W) float32 and rows (B,H): random values, channel 0 away from the nodata code except where a case plants it"""
    g = np.random.Generator(np.random.PCG64(sum(map(ord, name))))

    def values(B, C, H, W):
        x = g.normal(0, 1, (B, C, H, W)).astype(np.float32)
        x[:, 0] = np.abs(x[:, 0])  # never -1 by accident
        return x

    rows_of = lambda H, *sets: np.array([[1 if h in s else 0 for h in range(H)] for s in sets], np.uint8)
    if name == "h1_known":
        return values(1, 2, 1, 7), rows_of(1, {0})
    if name == "h1_unknown":
        return values(1, 2, 1, 7), rows_of(1, set())
    if name in ("ends_c1", "ends_c2"):  # rows {0,4}: two-sided, row 2 a nearest-mode tie; columns with one / both endpoints nodata
        x = values(1, int(name[-1]), 5, 7)
        x[0, 0, 0, 1], x[0, 0, 4, 2], x[0, 0, 0, 3], x[0, 0, 4, 3] = -1, -1, -1, -1
        x[0, 0, 2, 5] = -1  # (an unknown row's own value plays no part)
        return x, rows_of(5, {0, 4})
    if name == "middle_only":  # one-sided in both directions, one column without any usable endpoint
        x = values(1, 2, 5, 7)
        x[0, 0, 2, 6] = -1
        return x, rows_of(5, {2})
    if name == "none_known":
        return values(1, 2, 5, 7), rows_of(5, set())
    if name == "batch_of_3":  # a different row set per sample
        x = values(3, 2, 5, 7)
        x[0, 0, 0, 0], x[1, 0, 2, 4], x[2, 0, 1, 1] = -1, -1, -1
        return x, rows_of(5, {0, 4}, {2}, {1, 2, 4})
    if name == "beams4_16x128":  # rows 0, 4, 8, 12 known: 13-15 are one-sided; nodata sprinkled over the known rows
        x = values(2, 2, 16, 128)
        x[:, 0][g.uniform(size=(2, 16, 128)) < 0.2] = -1
        return x, np.repeat(completion.rows_of_mask(completion.corruption_mask("beams:4", 16, 128)[None]).numpy(), 2, 0)
    if name == "odd_gaps_9x300":  # gaps of 1, 2 and 4 rows (t = 1/3, 1/5, ... are inexact in float32), more than one block per row
        x = values(1, 1, 9, 300)
        x[:, 0][g.uniform(size=(1, 9, 300)) < 0.1] = -1
        return x, rows_of(9, {1, 3, 6})
    raise KeyError(name)


FILL_CASES = ("h1_known", "h1_unknown", "ends_c1", "ends_c2", "middle_only", "none_known", "batch_of_3", "beams4_16x128", "odd_gaps_9x300")


@pytest.mark.parametrize("mode", ("nearest", "linear"))
@pytest.mark.parametrize("name", FILL_CASES)
def test_fill_beams_bit_for_bit(name, mode):
    x, rows = fill_case(name)
    got = completion.fill_beams(torch.from_numpy(x).to(DEV), torch.from_numpy(rows), mode).cpu().numpy()
    want = O.fill(x, rows, mode)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} values differ, first at {tuple(np.argwhere(bad)[0])}"
    if name == "ends_c2":
        near = got if mode == "nearest" else None
        if near is not None:
            assert (near[0, :, 2, 0] == x[0, :, 0, 0]).all() and (near[0, :, 3, 0] == x[0, :, 4, 0]).all()  # the tie goes up
            assert (near[0, :, 1:4, 1] == x[0, :, 4:5, 1]).all() and (near[0, :, 1:4, 3] == -1).all()
    if name == "none_known":
        assert (got == -1).all()
    if name == "h1_known":
        assert (got == x).all()
    if name == "beams4_16x128":
        usable = x[:, :1, 12] != -1
        assert (np.where(usable, got[:, :, 15] == x[:, :, 12], got[:, :, 15] == -1)).all()  # one-sided: a copy, or nodata


def test_fill_beams_takes_bool_rows_and_another_nodata():
    x, rows = fill_case("batch_of_3")
    x[x == -1] = 0.0
    got = completion.fill_beams(torch.from_numpy(x).to(DEV), torch.from_numpy(rows).bool().to(DEV), "linear", nodata=0.0).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), O.fill(x, rows, "linear", nodata=0.0).view(np.uint32))
    with pytest.raises(ValueError):
        completion.fill_beams(torch.from_numpy(x).to(DEV), torch.from_numpy(rows[:, :4]), "linear")
    with pytest.raises(ValueError):
        completion.fill_beams(torch.from_numpy(x).to(DEV), torch.from_numpy(rows), "linear", nodata=math.nan)


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------------------
KINDS = ("full", "beams:4", "random_points:0.1")
E2E_METHODS = ("repaint", "nearest", "linear")
SEED = 5


def small_scans():
    pts = G.make_cloud("free_64x1024")
    return [np.ascontiguousarray(pts[0:25000]), np.ascontiguousarray(pts[30000:52000])]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """completion_eval.py once, on two small scans: (the JSON document, the saved tensors per kind, the files it read)"""
    tmp = tmp_path_factory.mktemp("completion")
    ckpt, weights = tmp / "synthetic.pth", tmp / "rangenet.pth"
    torch.save(synthetic_ckpt(resolution=GOLDEN_RES), ckpt)
    torch.save(synthetic.synthetic_rangenet_state(), weights)
    for k, s in enumerate(small_scans()):
        d = tmp / "scans" / f"seq_{k}"
        d.mkdir(parents=True)
        s.tofile(d / f"{k:010d}.bin")
    cmd = [sys.executable, f"{ROOT}/completion_eval.py", "--ckpt", str(ckpt), "--real_scans", str(tmp / "scans"), "--methods", *E2E_METHODS,
           "--num_steps", "2", "--num_resample_steps", "1", "--batch_size", "2", "--seed", str(SEED), "--rangenet_weights", str(weights),
           "--save_dir", str(tmp / "kept"), "--out", str(tmp / "out" / "completion.json")]
    for kind in KINDS:
        cmd += ["--corruption", kind]
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    text = (tmp / "out" / "completion.json").read_text()
    assert "NaN" not in text and "Infinity" not in text
    kept = {kind: torch.load(tmp / "kept" / (kind.replace(":", "_") + ".pt")) for kind in KINDS}
    return json.loads(text), kept, ckpt, weights


def close(got, want):
    """a reported number against the oracle's: None for NaN, else within SUM_BAR (an exact zero for a zero)"""
    if want is None or (isinstance(want, float) and math.isnan(want)):
        return got is None
    return got is not None and (got == want if want == 0 else abs(got - want) <= SUM_BAR * abs(want))


def test_completion_eval_document(run):
    doc, kept, ckpt, weights = run
    H, W = GOLDEN_RES
    info = doc["info"]
    assert set(info) >= {"ckpt", "source", "num_scans", "resolution", "corruptions", "methods", "num_steps", "num_resample_steps", "jump_length",
                         "batch_size", "seed", "lo", "hi", "rangenet_weights", "semseg_postprocess"}
    assert info["num_scans"] == 2 and info["corruptions"] == list(KINDS) and info["methods"] == list(E2E_METHODS) and info["seed"] == SEED
    assert info["resolution"] == [H, W] and (info["num_steps"], info["num_resample_steps"], info["jump_length"]) == (2, 1, 1)
    assert set(doc["results"]) == set(KINDS) and all(set(doc["results"][k]) == set(E2E_METHODS) for k in KINDS)
    for kind in KINDS:
        for method in E2E_METHODS:
            e = doc["results"][kind][method]
            if kind.startswith("random_points") and method != "repaint":
                assert set(e) == {"skipped"} and "whole rows" in e["skipped"]
                continue
            assert set(e) == {"counts", "sums", "micro", "macro", "iou"}
            assert set(e["micro"]) == set(e["macro"]) == set(completion.DERIVED_NAMES) and set(e["sums"]) == set(completion.RAW_NAMES[4:])
            assert set(e["counts"]) == {"scans", "unknown_without_return", *completion.RAW_NAMES[:4]} and e["counts"]["scans"] == 2
            assert set(e["iou"]) == {"per_class", "miou", "pixels"} and len(e["iou"]["per_class"]) == 20
    # "full": nothing to fill in -> zero evaluated pixels, null errors; the labels are still compared
    for method in E2E_METHODS:
        e = doc["results"]["full"][method]
        assert e["counts"]["unknown"] == e["counts"]["evaluated"] == 0 and all(v == 0 for v in e["sums"].values())
        assert all(e[g][n] is None for g in ("micro", "macro") for n in completion.DERIVED_NAMES) and e["iou"]["pixels"] > 0
    # the baselines copy a full scan's coding back: the same labels as the target's
    assert doc["results"]["beams:4"]["repaint"]["counts"]["evaluated"] > 100


def test_completion_eval_numbers_equal_the_oracle_on_the_saved_tensors(run):
    doc, kept, _, _ = run
    lo, hi = doc["info"]["lo"], doc["info"]["hi"]
    assert (lo, hi) == (1.45, 80.0)
    checked = 0
    for kind in KINDS:
        k = kept[kind]
        target, mask = k["target"].numpy(), k["mask"].numpy()
        assert target.shape == (2, 5, *GOLDEN_RES) and mask.shape == (2, 1, *GOLDEN_RES)
        measured = ((target[:, 0] > np.float32(lo)) & (target[:, 0] < np.float32(hi))).reshape(2, -1)
        for method in E2E_METHODS:
            e = doc["results"][kind][method]
            if "skipped" in e:
                assert method not in k["pred"]
                continue
            raw = O.error_sums(k["pred"][method].numpy(), target, mask, lo, hi)
            print(kind, method, raw.tolist(), e)
            total = raw.sum(0)
            for j, name in enumerate(completion.RAW_NAMES):
                got = e["counts"][name] if j < 4 else e["sums"][name]
                assert got == total[j] if j < 4 else close(got, float(total[j])), (kind, method, name)
            assert e["counts"]["unknown_without_return"] == total[0] - total[1]
            micro, per_scan = O.derived(total), O.derived(raw)
            for name in completion.DERIVED_NAMES:
                assert close(e["micro"][name], float(micro[name])), (kind, method, name)
                v = per_scan[name][~np.isnan(per_scan[name])]
                assert close(e["macro"][name], float(v.mean()) if v.size else None), (kind, method, name)
            conf = O.confusion(k["labels"][method].numpy().reshape(2, -1), k["target_labels"].numpy().reshape(2, -1), 20, measured).sum(0)
            per, miou = O.iou(conf)
            assert e["iou"]["pixels"] == conf.sum() == measured.sum()
            assert all(close(a, float(b)) for a, b in zip(e["iou"]["per_class"], per)) and close(e["iou"]["miou"], float(miou))
            checked += 1
    assert checked == 7


def test_completion_eval_inputs_follow_the_documented_seeding(run):
    doc, kept, ckpt, _ = run
    H, W = GOLDEN_RES
    ddpm, lidar, cfg = r2dm_amd.setup_model(str(ckpt), device=DEV, show_info=False, max_batch=2)
    files = sorted((ckpt.parent / "scans").rglob("*.bin"))
    unfolding, width = r2dm_amd.parse_projection(cfg.data.projection)
    pts, off = r2dm_amd.load_scans(files)
    planes = torch.nn.functional.interpolate(
        r2dm_amd.project_scans(pts, off, H=64, W=width, scan_unfolding=unfolding, min_depth=lidar.min_depth, max_depth=lidar.max_depth), size=(H, W),
        mode="nearest-exact")
    known = r2dm_amd.known_from_scan(planes, lidar, (H, W)).cpu()
    for kind in KINDS:
        want = torch.stack([completion.corruption_mask(kind, H, W, torch.Generator().manual_seed(completion.scan_seed(SEED, i))) for i in range(2)])
        assert torch.equal(kept[kind]["mask"], want), kind
        assert torch.equal(kept[kind]["x_in"], want * known + (1 - want) * -1)
        # the target is the scan's own measured planes
        assert torch.equal(kept[kind]["target"], planes[:, [4, 0, 1, 2, 3]].cpu())
    assert torch.equal(kept["beams:4"]["mask"][0, 0, :, 0], (torch.arange(H) % 4 == 0).float())
    assert not torch.equal(kept["random_points:0.1"]["mask"][0], kept["random_points:0.1"]["mask"][1])
    # a prediction is the decoded, clamped output
    for method in E2E_METHODS:
        x_out = kept["beams:4"]["x_out"][method].to(DEV)
        assert torch.equal(lidar.postprocess(x_out.clamp(-1, 1)).cpu(), kept["beams:4"]["pred"][method])
    # the known beams pass through every method unchanged
    m = kept["beams:4"]["mask"].bool().expand(-1, 2, -1, -1)
    for method in ("nearest", "linear"):
        assert torch.equal(kept["beams:4"]["x_out"][method][m], kept["beams:4"]["x_in"][m])

    # the target's own planes as the prediction: errors exactly 0, mIoU exactly 1; and a scan's inputs and numbers do not depend on the batch size
    semseg = r2dm_amd.pretrained_rangenet(synthetic.synthetic_rangenet_state(), device=DEV)
    res, k2 = completion.evaluate_completion(ddpm, lidar, planes, ["beams:4", "random_points:0.1"], methods=("target", "linear"), seed=SEED,
                                             batch_size=2, semseg=semseg, keep=True)
    for kind in ("beams:4", "random_points:0.1"):
        e = res[kind]["target"]
        assert e["counts"]["evaluated"] > 0 and e["counts"]["both"] == e["counts"]["evaluated"] and e["counts"]["false_returns"] == 0
        assert all(v == 0.0 for v in e["sums"].values())
        assert all(e[g][n] == 0.0 for g in ("micro", "macro") for n in completion.DERIVED_NAMES[:6])
        assert e["micro"]["return_recall"] == 1.0 and e["iou"]["miou"] == 1.0
        assert all(v == 1.0 or math.isnan(v) for v in e["iou"]["per_class"])
    assert "skipped" in res["random_points:0.1"]["linear"]
    res1, k1 = completion.evaluate_completion(ddpm, lidar, planes, ["beams:4"], methods=("linear",), seed=SEED, batch_size=1, semseg=semseg, keep=True)
    assert torch.equal(k1["beams:4"]["mask"], k2["beams:4"]["mask"]) and torch.equal(k1["beams:4"]["x_in"], kept["beams:4"]["x_in"])
    assert torch.equal(k1["beams:4"]["raw"]["linear"], k2["beams:4"]["raw"]["linear"])
    for part in ("counts", "sums", "micro", "macro"):
        assert completion.jsonable(res1["beams:4"]["linear"][part]) == doc["results"]["beams:4"]["linear"][part], part
