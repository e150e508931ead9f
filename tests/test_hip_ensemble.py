"""-m gpu: the ensemble scores (``ensemble_score_kernel`` in r2dm_amd/csrc/completion.hip, ``r2dm_amd.completion.ensemble_scores``,
``evaluate_completion(ensemble=K)``, ``completion_eval.py --ensemble``, ``completion_demo.py --ensemble``) against the plain numpy / float64
specification of tests/ensemble_oracle.py.

Tolerances (stated, derived from the number formats, not from the code under test):
  * the two counts, the rank histogram: exact (integers; integer atomics, no order dependence).
  * the float64 sums (raw columns 2 .. 12, the per-member sums): relative 1e-10 of the oracle -- test_hip_completion.py's SUM_BAR with the
    same reasoning.  Kernel and oracle widen the same float32 values, so every difference is exact in both; the sums are of non-negative
    terms, in whatever order: at most n * 2^-53 relative for n additions.  The longest chain here is the oracle's double loop, 2016 pairs
    per pixel at K = 64, followed by the sum over at most 2080 pixels: about 4100 * 2^-53 = 5e-13; the kernel's gap form has 63 terms per
    pixel.  (The two forms were measured on the CPU to agree to 2e-15; tests/test_ensemble_cpu.py holds them to 1e-13.)  1e-10 leaves a
    margin above 100.  A sum that is zero in the oracle is an exact zero.
  * maps: return_probability, depth_median, depth_min and depth_max bit for bit (n / K is one division; the others are members' values or
    the fp64 mean of two of them, rounded once); the means and stds within 1 fp32 ulp (fp64 values rounded once: a different order of an
    fp64 sum can move a rounding boundary).
  * the properties (two calls, alone against in a batch, permuted members, with and without maps) are bitwise.
  * end to end: the document's numbers are recomputed by the oracle from the kept tensors and held to the same bars.

Measured on an MI355X (each test prints its figures before it asserts): over the 100 kernel cases the largest relative difference of a sum
was 4.2e-16 and every map value, means and stds included, agreed in every bit; the whole file takes 16 s."""
import functools
import json
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, GOLDEN_RES, ROOT, synthetic_ckpt

sys.path.insert(0, GOLDEN)
import make_golden_projection as G  # noqa: E402  (read-only: the integer-only generator of the free cloud)

import completion_oracle as CO  # noqa: E402
import ensemble_oracle as O  # noqa: E402
import r2dm_amd  # noqa: E402
from r2dm_amd import completion  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
LO, HI = 1.45, 80.0
SUM_BAR = 1e-10
BATCHES = (1, 3)
PLANES = (1, 3, 35, 1025, 16 * 130)  # below, at and beyond one block of 256 pixels; 16 * 130 is the one multiple of 4 (16-byte alignment)
MEMBERS = (1, 2, 3, 8, 9, 16, 17, 32, 33, 64)  # both sides of every bucket edge
CASES = [(B, K, P) for B in BATCHES for P in PLANES for K in MEMBERS]
ids = lambda c: "B{}-K{}-P{}".format(*c)


# ---- 1. the kernel -----------------------------------------------------------------------------------------------------------------------
def ensemble_inputs(B, K, P):
    """samples (B,K,5,1,P), target (B,5,1,P), known (B,1,1,P) as numpy float32.  20 % of the members are dropped (0); up to eight special
    pixels per scan (as many as the plane has), all unknown: no member returns (NaN, +-inf, exactly lo, exactly hi); all return; all members
    tied on the target's value; NaN member reflectances; a target without a return; members at lo and hi among valid ones; a NaN target; two
    values alternating, one the target's.  Scan 1 of a batch is fully known: E is empty there."""
    g = np.random.Generator(np.random.PCG64(100000 * B + 1000 * K + P))
    target = g.uniform(0.0, 1.0, (B, 5, P)).astype(np.float32)
    target[:, 0] = g.uniform(0.5, 90.0, (B, P)).astype(np.float32)
    samples = (target[:, None] + g.normal(0, 0.5, (B, K, 5, P))).astype(np.float32)
    samples[:, :, 0][g.uniform(size=(B, K, P)) < 0.2] = 0
    known = (g.uniform(size=(B, 1, P)) < 0.5).astype(np.float32)
    none = np.array([np.nan, np.inf, -np.inf, LO, HI, 0.0, 100.0, -3.0], np.float32)
    for b in range(B):
        where = g.permutation(P)[:8]
        for j, p in enumerate(where):
            known[b, 0, p] = 0
            if j == 0:
                samples[b, :, 0, p] = none[np.arange(K) % 8]
                target[b, 0, p] = 20.0
            elif j == 1:
                samples[b, :, 0, p] = g.uniform(2.0, 70.0, K).astype(np.float32)
                target[b, 0, p] = 30.0
            elif j == 2:
                samples[b, :, 0, p], samples[b, :, 4, p] = 10.0, 0.25
                target[b, 0, p], target[b, 4, p] = 10.0, 0.25
            elif j == 3:
                samples[b, ::2, 4, p] = np.nan
                target[b, 0, p] = 40.0
            elif j == 4:
                target[b, 0, p] = 0.0
                samples[b, :, 0, p] = g.uniform(2.0, 70.0, K).astype(np.float32)
            elif j == 5:
                samples[b, :, 0, p] = g.uniform(2.0, 70.0, K).astype(np.float32)
                samples[b, 0, 0, p], samples[b, K // 2, 0, p] = LO, HI
                target[b, 0, p] = 50.0
            elif j == 6:
                target[b, 0, p] = np.nan
            else:
                samples[b, :, 0, p] = np.where(np.arange(K) % 2 == 0, np.float32(12.5), np.float32(13.5))
                target[b, 0, p] = 13.5
    if B > 1:
        known[1] = 1
    return samples.reshape(B, K, 5, 1, P), target.reshape(B, 5, 1, P), known.reshape(B, 1, 1, P)


def run_kernel(samples, target, known, maps=True):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    out = completion.ensemble_score_sums(dev(samples), dev(target), dev(known), LO, HI, maps=maps)
    return tuple(None if o is None else o.cpu().numpy() for o in out)


@functools.lru_cache(maxsize=None)
def case(B, K, P):
    """the inputs, the kernel's outputs and the oracle's, computed once per case and shared by the tests below (never modified)"""
    inputs = ensemble_inputs(B, K, P)
    return inputs, run_kernel(*inputs), O.scores(*inputs, LO, HI)


def check_sums(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float64, what
    assert np.isfinite(want).all(), what
    zero = want == 0
    assert (got[zero] == 0).all(), what
    rel = np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero])
    print(what, "largest relative difference", rel.max() if rel.size else 0.0)
    assert (rel <= SUM_BAR).all(), (what, rel.max())


def ulps(got, want):
    """the distance of two float32 arrays in units in the last place (their bit patterns on a line that is monotonic through zero)"""
    assert got.dtype == want.dtype == np.float32 and np.isfinite(want).all() and np.isfinite(got).all()
    line = lambda a: (lambda k: np.where(k < 0, -(k & 0x7fffffff), k))(np.ascontiguousarray(a).view(np.int32).astype(np.int64))
    return np.abs(line(got) - line(want))


@pytest.mark.parametrize("c", CASES, ids=ids)
def test_kernel_against_the_float64_oracle(c):
    B, K, P = c
    (samples, target, known), (raw, member, rank, maps), (wraw, wmember, wrank, wmaps) = case(*c)
    assert raw.shape == (B, 13) and member.shape == (B, 2, K) and rank.shape == (B, K + 1) and maps.shape == (B, 8, 1, P)
    assert rank.dtype == np.int64 and maps.dtype == np.float32
    assert np.array_equal(raw[:, :2], wraw[:, :2]) and np.array_equal(rank, wrank), c
    assert np.array_equal(rank.sum(1), raw[:, 1].astype(np.int64))
    check_sums(raw[:, 2:], wraw[:, 2:], (c, "raw"))
    check_sums(member, wmember, (c, "member"))
    for plane in (0, 3, 4, 5):
        assert np.array_equal(maps[:, plane].view(np.int32), wmaps[:, plane].view(np.int32)), (c, O.MAPS[plane])
    for plane in (1, 2, 6, 7):
        u = ulps(maps[:, plane], wmaps[:, plane])
        print(c, O.MAPS[plane], "largest difference in ulps", u.max())
        assert u.max() <= 1, (c, O.MAPS[plane], u.max())
    # the derived values: NaN exactly where the oracle's are (the fully known scan), else ratios of the above
    got = completion.derived_ensemble(torch.from_numpy(raw), torch.from_numpy(member))
    want = O.derived(wraw, wmember)
    for name in completion.ENSEMBLE_DERIVED_NAMES:
        assert np.allclose(got[name].numpy(), want[name], rtol=SUM_BAR, atol=0, equal_nan=True), (c, name)
    if B > 1:
        assert raw[1, 1] == 0 and (raw[1, 2:] == 0).all() and all(np.isnan(got[n][1]) for n in completion.ENSEMBLE_DERIVED_NAMES)
    if P >= 35:  # every set is reached
        assert wraw[0, 0] > wraw[0, 1] > 0 and (wraw[0, [2, 4, 6, 8, 10, 11, 12]] > 0).all() and (maps[0, 0] == 0).any() and (maps[0, 0] == 1).any()


@pytest.mark.parametrize("c", CASES, ids=ids)
def test_kernel_properties_are_bitwise(c):
    B, K, P = c
    (samples, target, known), got, _ = case(*c)
    same = lambda a, b: all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert same(run_kernel(samples, target, known), got), "two calls"
    raw, member, rank, none = run_kernel(samples, target, known, maps=False)
    assert none is None and same((raw, member, rank), got[:3]), "without maps"
    b = B - 1  # a scan alone against the same scan inside the batch
    alone = run_kernel(samples[b:b + 1], target[b:b + 1], known[b:b + 1])
    assert same(alone, tuple(o[b:b + 1] for o in got)), "alone"
    perm = np.random.Generator(np.random.PCG64(K)).permutation(K)
    raw, member, rank, maps = run_kernel(samples[:, perm], target, known)
    assert same((raw, rank, maps), (got[0], got[2], got[3])) and member.tobytes() == np.ascontiguousarray(got[1][:, :, perm]).tobytes(), "permuted"


@pytest.mark.parametrize("c", [(B, 1, P) for B in BATCHES for P in PLANES], ids=ids)
def test_one_member_is_the_error_kernel(c):
    (samples, target, known), (raw, member, rank, _), _ = case(*c)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    err = completion.completion_error_sums(dev(samples[:, 0]), dev(target), dev(known), LO, HI).cpu().numpy()
    # |U|, |E|; with one member the expected returns are the counted ones
    assert np.array_equal(raw[:, :2], err[:, :2]) and np.array_equal(raw[:, 11], err[:, 2]) and np.array_equal(raw[:, 12], err[:, 3])
    # (the reflectance sums differ by definition: a NaN member reflectance counts as 0 here)
    check_sums(raw[:, [2, 4]], err[:, [4, 5]], (c, "against completion_error"))
    check_sums(member[:, :, 0], raw[:, [2, 6]], (c, "the one member"))
    assert (raw[:, [3, 5, 7, 9]] == 0).all()


def test_the_public_entry_and_the_consensus():
    (samples, target, known), (raw, member, rank, maps), _ = case(3, 9, 35)
    H, W = 5, 7
    dev = lambda a, *s: torch.from_numpy(np.ascontiguousarray(a)).reshape(*s).to(DEV)
    out = r2dm_amd.ensemble_scores(dev(samples, 3, 9, 5, H, W), dev(target, 3, 5, H, W), dev(known, 3, 1, H, W), LO, HI)
    assert set(out) == {*completion.ENSEMBLE_RAW_NAMES, *completion.ENSEMBLE_DERIVED_NAMES, "member_abs_depth", "member_abs_reflectance",
                        "rank_histogram", "maps"}
    assert all(np.array_equal(out[n].cpu().numpy(), raw[:, k]) for k, n in enumerate(completion.ENSEMBLE_RAW_NAMES))
    assert np.array_equal(out["member_abs_depth"].cpu().numpy(), member[:, 0]) and np.array_equal(out["rank_histogram"].cpu().numpy(), rank)
    assert out["maps"].shape == (3, 8, H, W) and np.array_equal(out["maps"].cpu().numpy().reshape(3, 8, 1, 35), maps)
    assert r2dm_amd.ensemble_scores(dev(samples, 3, 9, 5, H, W), dev(target, 3, 5, H, W), dev(known, 3, 1, H, W), LO, HI, maps=False)["maps"] is None
    with pytest.raises(ValueError):
        r2dm_amd.ensemble_scores(torch.zeros(1, 65, 5, H, W, device=DEV), torch.zeros(1, 5, H, W, device=DEV), torch.zeros(1, 1, H, W, device=DEV), LO, HI)
    with pytest.raises(ValueError):
        r2dm_amd.ensemble_scores(torch.zeros(1, 2, 5, H, W, device=DEV), torch.zeros(1, 5, H, W + 1, device=DEV), torch.zeros(1, 1, H, W, device=DEV), LO, HI)
    lidar = r2dm_amd.LiDARUtility(resolution=(H, W), depth_format="log_depth", min_depth=LO, max_depth=HI).to(DEV)
    cons = r2dm_amd.ensemble_consensus(out["maps"], lidar)
    m = out["maps"]
    depth = torch.where(m[:, [0]] >= 0.5, m[:, [3]], torch.zeros_like(m[:, [3]]))
    assert cons.shape == (3, 5, H, W) and torch.equal(cons[:, [0]], depth) and torch.equal(cons[:, [4]], m[:, [6]])
    assert torch.equal(cons[:, 1:4], lidar.to_xyz(depth)) and (depth == 0).any() and (depth > 0).any()


# ---- 2. end to end -----------------------------------------------------------------------------------------------------------------------
SEED = 5
KIND = "beams:4"
E2E_METHODS = ("dpmpp", "linear")
H, W = GOLDEN_RES


def small_scans():
    pts = G.make_cloud("free_64x1024")
    return [np.ascontiguousarray(pts[0:25000]), np.ascontiguousarray(pts[30000:52000])]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ensemble")
    ckpt = tmp / "synthetic.pth"
    torch.save(synthetic_ckpt(resolution=GOLDEN_RES), ckpt)
    for k, s in enumerate(small_scans()):
        d = tmp / "scans" / f"seq_{k}"
        d.mkdir(parents=True)
        s.tofile(d / f"{k:010d}.bin")
    return tmp, ckpt


@pytest.fixture(scope="module")
def runs(files):
    """evaluate_completion on the two scans: with ensemble = 3 (twice) and without"""
    import completion_eval

    tmp, ckpt = files
    ddpm, lidar, cfg = r2dm_amd.setup_model(str(ckpt), device=DEV, show_info=False, max_batch=2)
    scans = sorted((tmp / "scans").rglob("*.bin"))  # (evaluate.scan_files' order)
    planes = completion_eval.planes_of_scans(scans, cfg, lidar, 2, torch.device(DEV))
    go = lambda **kw: completion.evaluate_completion(ddpm, lidar, planes, [KIND], methods=E2E_METHODS, num_steps=2, seed=SEED, batch_size=2,
                                                     keep=True, **kw)
    return go(ensemble=3), go(ensemble=3), go(), lidar


def test_member_zero_is_the_single_draw(runs):
    (res, kept), _, (res1, kept1), _ = runs
    assert "ensemble" not in res1[KIND]["dpmpp"] and "ensemble" not in kept1[KIND]
    for method in E2E_METHODS:
        assert torch.equal(kept[KIND]["x_out"][method], kept1[KIND]["x_out"][method])
        assert torch.equal(kept[KIND]["raw"][method], kept1[KIND]["raw"][method])
        entry = {k: v for k, v in res[KIND][method].items() if k != "ensemble"}
        assert completion.jsonable(entry) == completion.jsonable(res1[KIND][method]) and set(entry) == {"counts", "sums", "micro", "macro"}
    members = kept[KIND]["ensemble"]["dpmpp"]["x_out"]
    assert members.shape == (2, 3, 2, H, W) and torch.equal(members[:, 0], kept1[KIND]["x_out"]["dpmpp"])
    unknown = (kept[KIND]["mask"] == 0).expand(2, 2, H, W)
    for i in range(2):
        for a, b in ((0, 1), (0, 2), (1, 2)):
            assert not torch.equal(members[i, a][unknown[i]], members[i, b][unknown[i]])
            assert torch.equal(members[i, a][~unknown[i]], members[i, b][~unknown[i]])  # one mask, the known pixels kept
    assert kept[KIND]["ensemble"]["linear"]["x_out"] is None


def test_a_deterministic_method_is_an_ensemble_of_one(runs):
    (res, kept), _, _, _ = runs
    e = res[KIND]["linear"]
    assert e["ensemble"]["members"] == 1 and e["ensemble"]["counts"]["members"] == 1 and res[KIND]["dpmpp"]["ensemble"]["members"] == 3
    for group in ("micro", "macro"):
        crps, mae = e["ensemble"][group]["crps_depth"], e[group]["mae_depth"]
        print(group, "crps_depth", crps, "mae_depth", mae)
        assert mae > 0 and abs(crps - mae) <= SUM_BAR * mae
    assert e["ensemble"]["counts"]["evaluated"] == e["counts"]["evaluated"] > 100
    assert kept[KIND]["ensemble"]["linear"]["rank"].shape == (2, 2)


def test_the_ensemble_numbers_equal_the_oracle_on_the_kept_tensors(runs):
    (res, kept), _, _, lidar = runs
    k = kept[KIND]
    target, mask = k["target"].numpy(), k["mask"].numpy()
    close = lambda got, want: (np.isnan(got) and np.isnan(want)) or (got == want if want == 0 else abs(got - want) <= SUM_BAR * abs(want))
    for method, K in (("dpmpp", 3), ("linear", 1)):
        e, t = res[KIND][method]["ensemble"], k["ensemble"][method]
        x = t["x_out"] if K > 1 else k["x_out"][method][:, None]
        samples = lidar.postprocess(x.flatten(0, 1).to(DEV).clamp(-1, 1)).reshape(2, K, 5, H, W).cpu().numpy()
        wraw, wmember, wrank, wmaps = O.scores(samples, target, mask, LO, HI)
        raw, member, rank, maps = (t[n].numpy() for n in ("raw", "member", "rank", "maps"))
        assert np.array_equal(raw[:, :2], wraw[:, :2]) and np.array_equal(rank, wrank) and wraw[:, 1].min() > 100
        check_sums(raw[:, 2:], wraw[:, 2:], (method, "raw"))
        check_sums(member, wmember, (method, "member"))
        assert all(np.array_equal(maps[:, p].view(np.int32), wmaps[:, p].view(np.int32)) for p in (0, 3, 4, 5))
        assert all(ulps(maps[:, p], wmaps[:, p]).max() <= 1 for p in (1, 2, 6, 7))
        assert e["rank_histogram"] == wrank.sum(0).tolist() and sum(e["rank_histogram"]) == e["counts"]["evaluated"] == int(wraw[:, 1].sum())
        micro, per_scan = O.derived(wraw.sum(0), wmember.sum(0)), O.derived(wraw, wmember)
        for name in completion.ENSEMBLE_DERIVED_NAMES:
            assert close(e["micro"][name], float(micro[name])), (method, name, e["micro"][name], micro[name])
            ok = ~np.isnan(per_scan[name])
            assert close(e["macro"][name], float(per_scan[name][ok].mean()) if ok.any() else np.nan), (method, name)
        assert all(close(e["sums"][n], float(wraw[:, j].sum())) for j, n in enumerate(O.RAW) if j >= 2)
        # the consensus scan: the median depth where at least half of the members return, the mean reflectance
        cons = np.zeros_like(target)
        cons[:, 0] = np.where(wmaps[:, 0] >= 0.5, wmaps[:, 3], np.float32(0))
        cons[:, 4] = maps[:, 6]
        want = CO.error_sums(cons, target, mask, LO, HI)
        got = t["consensus_raw"].numpy()
        assert np.array_equal(got[:, :4], want[:, :4])
        check_sums(got[:, 4:], want[:, 4:], (method, "consensus"))
        derived = CO.derived(want.sum(0))
        assert all(close(e["consensus"]["micro"][n], float(derived[n])) for n in completion.DERIVED_NAMES)
    # one member: the consensus is the member
    assert completion.jsonable(res[KIND]["linear"]["ensemble"]["consensus"]["counts"]) == completion.jsonable(res[KIND]["linear"]["counts"])


def test_a_second_run_reproduces_the_document(runs):
    (res, kept), (res2, kept2), _, _ = runs
    assert json.dumps(completion.jsonable(res), sort_keys=True) == json.dumps(completion.jsonable(res2), sort_keys=True)
    for method in E2E_METHODS:
        a, b = kept[KIND]["ensemble"][method], kept2[KIND]["ensemble"][method]
        assert all(torch.equal(a[n], b[n]) for n in ("raw", "member", "rank", "maps", "consensus_raw"))


def png_size(path):
    with open(path, "rb") as f:
        head = f.read(24)
    assert head[:8] == b"\x89PNG\r\n\x1a\n" and head[12:16] == b"IHDR"
    return struct.unpack(">II", head[16:24])


def test_completion_eval_with_an_ensemble(files, runs):
    tmp, ckpt = files
    out = tmp / "eval" / "completion.json"
    r = subprocess.run([sys.executable, f"{ROOT}/completion_eval.py", "--ckpt", str(ckpt), "--real_scans", str(tmp / "scans"), "--methods", *E2E_METHODS,
                        "--num_steps", "2", "--batch_size", "2", "--seed", str(SEED), "--corruption", KIND, "--ensemble", "3",
                        "--save_dir", str(tmp / "eval"), "--out", str(out)], cwd=tmp, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert any("3 members: CRPS depth" in line for line in r.stdout.splitlines()), r.stdout
    text = out.read_text()
    assert "NaN" not in text and "Infinity" not in text
    doc = json.loads(text)
    assert doc["info"]["ensemble"] == 3
    # the script's document is the function's
    assert doc["results"] == json.loads(json.dumps(completion.jsonable(runs[0][0])))
    k = torch.load(tmp / "eval" / "beams_4.pt")
    assert k["ensemble"]["dpmpp"]["maps"].shape == (2, 8, H, W) and torch.equal(k["ensemble"]["dpmpp"]["maps"], runs[0][1][KIND]["ensemble"]["dpmpp"]["maps"])
    p = k["ensemble"]["dpmpp"]["maps"][:, 0]
    assert set(p.unique().tolist()) <= {0.0, np.float32(1 / 3).item(), np.float32(2 / 3).item(), 1.0}


def test_completion_demo_with_an_ensemble(files):
    tmp, ckpt = files
    (tmp / "demo").mkdir()
    scan_file = next((tmp / "scans").rglob("*.bin"))
    base = [sys.executable, f"{ROOT}/completion_demo.py", "--ckpt", str(ckpt), "--scan", str(scan_file), "--method", "dpmpp", "--num_steps", "2", "--seed", "3"]
    r = subprocess.run(base + ["--ensemble", "2", "--out", str(tmp / "demo" / "ensemble.png")], cwd=tmp / "demo", capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    # the four rows of the plain run (2H + W + 2H + W) and the two new ones of H each
    assert png_size(tmp / "demo" / "ensemble.png") == (4 * (W + 2) + 2, 4 * H + 2 * W + 2 * H + 4)
    state = torch.load(tmp / "demo" / "completion.pt")
    assert set(state) == {"x_in", "mask", "x_out", "maps"} and state["maps"].shape == (4, 8, H, W) and state["maps"].dtype == torch.float32
    assert set(state["maps"][:, 0].unique().tolist()) <= {0.0, 0.5, 1.0}
    # the full input (column 0) leaves nothing to draw: both members are the scan, the depth std is 0
    assert (state["maps"][0, 2] == 0).all() and (state["maps"][1, 2] > 0).any()
