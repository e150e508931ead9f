"""-m gpu: the ensemble coherence sums (``coherence_dist_kernel`` / ``coherence_vario_kernel`` in r2dm_amd/csrc/completion.hip,
``r2dm_amd.completion.ensemble_coherence``, ``evaluate_completion(ensemble_coherence=True)``, ``completion_eval.py --ensemble_coherence``)
against the plain numpy / float64 specification of tests/coherence_oracle.py.

Bars (stated, derived from the number formats, not from the code under test):
  * ``counts`` and the pair counts of ``vario``: exact (integers below 2^53 counted in float64).
  * ``dist``: relative 1e-10 of the oracle.  Kernel and oracle widen the same float32 values, so every difference is exact in float64;
    each square is rounded at most once (the kernel fuses it into the addition); at most 2080 non-negative terms are added, in whatever order: at most about 2100 * 2^-53 = 2.3e-13
    relative.  A margin above 100.  A sum that is zero in the oracle is an exact zero; the diagonal is 0; [i][j] and [j][i] have equal bits.
  * ``vario``, sum a^2: relative 1e-10, by the same reasoning (a^2 = sqrt(x)^2 adds two roundings per term).
  * ``vario``, sum m^2 and sum (a - m)^2: absolute 1e-10 * (sum a^2 + sum m^2) of the oracle: a - m can cancel, so the error of a term is
    bounded not by the term but by about 4 K * 2^-53 * (a^2 + m^2) (K roots and K additions behind m), 2.8e-14 at K = 64, and the
    summation adds about 2.3e-13.  A margin above 100.
  * the properties (two calls, alone against in a batch, a part left out, permuted members) are bitwise.
  * at K = 1 the squared distance to the target is ``completion_error_sums``' squared error, to 1e-10 relative (two float64 sums of the same
    terms in different orders).  The error kernel takes a member's reflectance as stored, this one reads its NaN as 0 (the convention of
    ``r2dm_ensemble_score``), so the comparison hands the error kernel the member with that convention applied.
  * end to end: the kept tensors are held to the oracle by the bars above, the document's numbers to the oracle's formulas on the kept
    tensors by 1e-12 (host arithmetic on equal float64 sums, tests/test_coherence_cpu.py).

Measured on an MI355X (each test prints its figures before it asserts): over the 140 kernel cases, the shuffle input and the end-to-end run
the largest relative difference of a ``dist`` entry was 7.5e-16 and of a sum a^2 2.2e-16, the largest difference of a sum m^2 or
sum (a - m)^2 3.1e-16 of (sum a^2 + sum m^2); at K = 1 the squared distances were within 1.8e-16 of ``completion_error_sums``; on the shuffle
input the GPU gives 1.157 x on the energy score and 28.04 x on the variogram score, as the oracle; the whole file takes 11 s."""
import functools
import json
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, GOLDEN_RES, ROOT, synthetic_ckpt

sys.path.insert(0, GOLDEN)
import make_golden_projection as G  # noqa: E402  (read-only: the integer-only generator of the free cloud)

import coherence_oracle as O  # noqa: E402
import r2dm_amd  # noqa: E402
from r2dm_amd import _lib, completion  # noqa: E402
from test_coherence_cpu import ENERGY_FACTOR, OFFSETS, VARIOGRAM_FACTOR, separation, shuffle_case  # noqa: E402
from test_hip_ensemble import ensemble_inputs  # noqa: E402  (the recipe: 20 % dropped members, eight special pixels, scan 1 fully known)

pytestmark = pytest.mark.gpu
DEV = "cuda"
LO, HI = 1.45, 80.0
BAR = 1e-10
BATCHES = (1, 3)
# a single pixel; a wrap distance of 1; rows crossing a wave; more than one slab of 1024 pixels (8 x 260, 16 x 130); 16 x 130 is the one plane
# that is a multiple of 4 (16-byte alignment)
SHAPES = ((1, 1), (1, 3), (2, 5), (5, 7), (3, 70), (8, 260), (16, 130))
MEMBERS = (1, 2, 3, 7, 8, 9, 16, 17, 33, 64)  # K + 1 rows in tiles of 8: both sides of every tile edge
CASES = [(B, K, H, W) for B in BATCHES for (H, W) in SHAPES for K in MEMBERS]
ids = lambda c: "B{}-K{}-{}x{}".format(*c)


def offsets_of(H, W):
    return tuple(o for o in ((0, 1), (1, 0), (1, -1), (0, W - 1), (H - 1, 0)) if o != (0, 0) and abs(o[0]) < H and abs(o[1]) < W)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_kernel(samples, target, known, offsets):
    out = completion.ensemble_coherence_sums(dev(samples), dev(target), dev(known), LO, HI, offsets)
    assert out[3] == tuple(offsets)
    return tuple(o.cpu().numpy() for o in out[:3])


def run_abi(samples, target, known, offsets, dist=True, vario=True):
    """the C entry itself, with ``dist`` or ``vario`` left out (NULL); what is left out comes back as None"""
    import ctypes

    s, t, k = dev(samples), dev(target), dev(known)
    B, K, _, H, W = s.shape
    L = _lib.lib()
    scratch = torch.empty(L.r2dm_ensemble_coherence_scratch_bytes(B, K, H, W, len(offsets)) // 8, dtype=torch.float64, device=DEV)
    counts = torch.empty(B, 2, dtype=torch.float64, device=DEV)
    d = torch.empty(B, 2, K + 1, K + 1, dtype=torch.float64, device=DEV) if dist else None
    v = torch.empty(B, 2, len(offsets), 4, dtype=torch.float64, device=DEV) if vario else None
    host = (ctypes.c_int32 * max(2 * len(offsets), 1))(*[x for o in offsets for x in o])
    _lib.check(L.r2dm_ensemble_coherence(_lib.ptr(s), _lib.ptr(t), _lib.ptr(k), LO, HI, B, K, H, W, ctypes.cast(host, ctypes.c_void_p), len(offsets),
                                         _lib.ptr(scratch), _lib.ptr(counts), _lib.ptr(d), _lib.ptr(v), _lib.stream_ptr(torch.device(DEV))))
    return tuple(None if o is None else o.cpu().numpy() for o in (counts, d, v))


@functools.lru_cache(maxsize=None)
def case(B, K, H, W):
    """the inputs, the kernel's outputs and the oracle's, computed once per case and shared by the tests below (never modified)"""
    samples, target, known = ensemble_inputs(B, K, H * W)
    inputs = (samples.reshape(B, K, 5, H, W), target.reshape(B, 5, H, W), known.reshape(B, 1, H, W))
    offsets = offsets_of(H, W)
    return inputs, offsets, run_kernel(*inputs, offsets), O.scores(*inputs, LO, HI, offsets)


def check_dist(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float64 and np.isfinite(want).all(), what
    zero = want == 0
    rel = np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero])
    print(what, "dist: largest relative difference", rel.max() if rel.size else 0.0)
    assert (got[zero] == 0).all(), what
    assert (rel <= BAR).all(), (what, rel.max())
    R = got.shape[-1]
    assert (got[..., np.arange(R), np.arange(R)] == 0).all(), what
    assert got.tobytes() == np.ascontiguousarray(np.swapaxes(got, -1, -2)).tobytes(), (what, "symmetry")


def check_vario(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float64 and np.isfinite(want).all(), what
    assert np.array_equal(got[..., 0], want[..., 0]), (what, "pairs")
    a2, m2 = want[..., 2], want[..., 3]
    zero = a2 == 0
    rel = np.abs(got[..., 2][~zero] - a2[~zero]) / a2[~zero]
    scale = a2 + m2
    some = scale > 0
    cancel = np.maximum(np.abs(got[..., 1] - want[..., 1]), np.abs(got[..., 3] - want[..., 3]))
    print(what, "vario: largest relative difference of sum a^2", rel.max() if rel.size else 0.0, "largest difference of sum m^2 and sum (a - m)^2 over "
          "(sum a^2 + sum m^2)", (cancel[some] / scale[some]).max() if some.any() else 0.0)
    assert (got[..., 2][zero] == 0).all() and (rel <= BAR).all(), (what, "sum a^2")
    assert (cancel <= BAR * scale).all(), (what, "sum m^2, sum (a - m)^2")


# ---- 1. the kernels against the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=ids)
def test_kernel_against_the_float64_oracle(c):
    B, K, H, W = c
    _, offsets, (counts, dist, vario), (wcounts, wdist, wvario) = case(*c)
    assert counts.shape == (B, 2) and dist.shape == (B, 2, K + 1, K + 1) and vario.shape == (B, 2, len(offsets), 4)
    assert np.array_equal(counts, wcounts), c
    check_dist(dist, wdist, c)
    check_vario(vario, wvario, c)
    got = completion.derived_coherence(torch.from_numpy(counts), torch.from_numpy(dist), torch.from_numpy(vario))
    want = O.derived(wcounts, wdist, wvario)
    for name in ("member_rmse_depth", "member_rmse_reflectance", "best_rmse_depth"):  # a root of one sum held to 1e-10
        assert np.allclose(got[name].numpy(), want[name], rtol=BAR, atol=0, equal_nan=True), (c, name)
    for name in completion.COHERENCE_DERIVED_NAMES:  # NaN exactly where the oracle's are (tests/test_coherence_cpu.py holds the formulas)
        assert np.array_equal(np.isnan(got[name].numpy()), np.isnan(want[name])), (c, name)
    if B > 1:  # scan 1 is fully known: E is empty
        assert counts[1].tolist() == [0, 0] and (dist[1] == 0).all() and (vario[1] == 0).all() and got["energy_depth"][1].isnan()
    if H * W >= 35:  # every set is reached
        assert wcounts[0, 0] > wcounts[0, 1] > 0 and (wdist[0, :, 0, K] > 0).all() and wvario[0, 0, 0, 0] > 0 and len(offsets) == 5


@pytest.mark.parametrize("c", CASES, ids=ids)
def test_kernel_properties_are_bitwise(c):
    B, K, H, W = c
    (samples, target, known), offsets, got, _ = case(*c)
    same = lambda a, b: all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert same(run_kernel(samples, target, known, offsets), got), "two calls"
    b = B - 1  # a scan alone against the same scan inside the batch
    assert same(run_kernel(samples[b:b + 1], target[b:b + 1], known[b:b + 1], offsets), tuple(o[b:b + 1] for o in got)), "alone"
    perm = np.random.Generator(np.random.PCG64(K)).permutation(K)
    rows = np.concatenate([perm, [K]])
    counts, dist, vario = run_kernel(samples[:, perm], target, known, offsets)
    assert counts.tobytes() == got[0].tobytes()
    assert dist.tobytes() == np.ascontiguousarray(got[1][:, :, rows][:, :, :, rows]).tobytes(), "permuted members permute rows and columns"
    a = completion.derived_coherence(*(torch.from_numpy(x) for x in got))
    p = completion.derived_coherence(torch.from_numpy(counts), torch.from_numpy(dist), torch.from_numpy(vario))
    for name in ("energy_depth", "energy_fair_depth", "energy_reflectance", "energy_fair_reflectance"):
        assert a[name].numpy().tobytes() == p[name].numpy().tobytes(), name


@pytest.mark.parametrize("c", [(3, 9, 5, 7), (1, 16, 8, 260), (3, 1, 1, 3)], ids=ids)
def test_a_part_left_out_leaves_the_other_unchanged(c):
    (samples, target, known), offsets, got, _ = case(*c)
    counts, dist, vario = run_abi(samples, target, known, offsets)
    assert all(x.tobytes() == y.tobytes() for x, y in zip((counts, dist, vario), got))
    counts, dist, vario = run_abi(samples, target, known, offsets, dist=False)
    assert dist is None and counts.tobytes() == got[0].tobytes() and vario.tobytes() == got[2].tobytes()
    counts, dist, vario = run_abi(samples, target, known, offsets, vario=False)
    assert vario is None and counts.tobytes() == got[0].tobytes() and dist.tobytes() == got[1].tobytes()
    counts, dist, vario = run_abi(samples, target, known, (), vario=False)
    assert counts.tobytes() == got[0].tobytes() and dist.tobytes() == got[1].tobytes()


# ---- 2. consistency with what exists ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [(B, 1, H, W) for B in BATCHES for (H, W) in SHAPES], ids=ids)
def test_one_member_is_the_error_kernel(c):
    (samples, target, known), _, (counts, dist, _), _ = case(*c)
    member = samples[:, 0].copy()
    member[:, 4] = np.where(np.isnan(member[:, 4]), np.float32(0), member[:, 4])  # (the convention here; see the docstring)
    err = completion.completion_error_sums(dev(member), dev(target), dev(known), LO, HI).cpu().numpy()
    assert np.array_equal(counts, err[:, :2])
    for ch, col in ((0, 5), (1, 9)):
        got, want = dist[:, ch, 0, 1], err[:, col]
        rel = np.abs(got - want)[want != 0] / want[want != 0]
        print(c, completion.RAW_NAMES[col], "largest relative difference", rel.max() if rel.size else 0.0)
        assert (got[want == 0] == 0).all() and (rel <= BAR).all(), (c, ch)


@pytest.mark.parametrize("c", [(3, 9, 5, 7), (1, 16, 16, 130), (3, 64, 3, 70)], ids=ids)
def test_the_counts_are_the_ensemble_kernel_s(c):
    (samples, target, known), _, (counts, _, _), _ = case(*c)
    raw = completion.ensemble_score_sums(dev(samples), dev(target), dev(known), LO, HI, maps=False)[0].cpu().numpy()
    assert np.array_equal(counts, raw[:, :2])


def test_the_public_entry():
    (samples, target, known), offsets, (counts, dist, vario), _ = case(3, 9, 5, 7)
    out = r2dm_amd.ensemble_coherence(dev(samples), dev(target), dev(known), LO, HI, offsets)
    assert set(out) == {"counts", "dist", "vario", "offsets", *completion.COHERENCE_DERIVED_NAMES} and out["offsets"] == offsets
    assert all(np.array_equal(out[n].cpu().numpy(), w) for n, w in (("counts", counts), ("dist", dist), ("vario", vario)))
    assert out["member_rmse_depth"].shape == (3, 9) and out["variogram_depth"].shape == (3, 5) and out["energy_depth"].is_cuda
    # the default offsets: those of DEFAULT_OFFSETS that fit 5 x 7 (all but (0, 8)); on a single row the four along the beam; on one pixel none
    fit = tuple(o for o in completion.DEFAULT_OFFSETS if o != (0, 8))
    assert r2dm_amd.ensemble_coherence(dev(samples), dev(target), dev(known), LO, HI)["offsets"] == fit and len(fit) == 7
    row = [dev(a.reshape(*a.shape[:-2], 1, 35)) for a in (samples, target, known)]
    assert completion.ensemble_coherence_sums(*row, LO, HI)[3] == ((0, 1), (0, 2), (0, 4), (0, 8))
    (s1, t1, k1), _, got1, _ = case(1, 2, 1, 1)
    one = completion.ensemble_coherence_sums(dev(s1), dev(t1), dev(k1), LO, HI)
    assert one[3] == () and one[2].shape == (1, 2, 0, 4) and np.array_equal(one[1].cpu().numpy(), got1[1])
    for bad in (((0, 0),), ((5, 0),), ((0, -7),), tuple((0, 1) for _ in range(17))):
        with pytest.raises(ValueError):
            completion.ensemble_coherence_sums(dev(samples), dev(target), dev(known), LO, HI, bad)
    with pytest.raises(ValueError):
        completion.ensemble_coherence_sums(torch.zeros(1, 65, 5, 5, 7, device=DEV), torch.zeros(1, 5, 5, 7, device=DEV), torch.zeros(1, 1, 5, 7, device=DEV), LO, HI)
    with pytest.raises(ValueError):
        completion.ensemble_coherence_sums(torch.zeros(1, 2, 5, 5, 7, device=DEV), torch.zeros(1, 5, 5, 8, device=DEV), torch.zeros(1, 1, 5, 7, device=DEV), LO, HI)


# ---- 3. the point of the feature ----------------------------------------------------------------------------------------------------------
def test_the_shuffled_ensemble_is_told_from_the_coherent_one():
    (coherent, shuffled, target, known), want_coherent, want_shuffled = shuffle_case()
    a = completion.ensemble_score_sums(dev(coherent), dev(target), dev(known), LO, HI, maps=False)
    b = completion.ensemble_score_sums(dev(shuffled), dev(target), dev(known), LO, HI, maps=False)
    # the per-pixel scores see the same K values at every pixel: the same bits
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes()
    assert (a[0][:, 2] > 0).all()
    derived = []
    for name, samples, want in (("coherent", coherent, want_coherent), ("shuffled", shuffled, want_shuffled)):
        counts, dist, vario = run_kernel(samples, target, known, OFFSETS)
        assert np.array_equal(counts, want[0])
        check_dist(dist, want[1], name)
        check_vario(vario, want[2], name)
        derived.append({n: v.numpy() for n, v in completion.derived_coherence(*(torch.from_numpy(x) for x in (counts, dist, vario))).items()})
    energy, variogram = separation(*derived)
    print("shuffled / coherent on the GPU: energy_depth", energy, "variogram_total_depth", variogram)
    assert energy >= ENERGY_FACTOR and variogram >= VARIOGRAM_FACTOR


# ---- 4. end to end ------------------------------------------------------------------------------------------------------------------------
SEED = 5
KIND = "beams:4"
E2E_METHODS = ("dpmpp", "linear")
H, W = GOLDEN_RES


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("coherence")
    ckpt = tmp / "synthetic.pth"
    torch.save(synthetic_ckpt(resolution=GOLDEN_RES), ckpt)
    pts = G.make_cloud("free_64x1024")
    for k, s in enumerate((np.ascontiguousarray(pts[0:25000]), np.ascontiguousarray(pts[30000:52000]))):
        d = tmp / "scans" / f"seq_{k}"
        d.mkdir(parents=True)
        s.tofile(d / f"{k:010d}.bin")
    return tmp, ckpt


@pytest.fixture(scope="module")
def runs(files):
    """evaluate_completion on the two scans: with ensemble = 3 and the coherence scores, and with ensemble = 3 alone"""
    import completion_eval

    tmp, ckpt = files
    ddpm, lidar, cfg = r2dm_amd.setup_model(str(ckpt), device=DEV, show_info=False, max_batch=2)
    scans = sorted((tmp / "scans").rglob("*.bin"))
    planes = completion_eval.planes_of_scans(scans, cfg, lidar, 2, torch.device(DEV))
    go = lambda **kw: completion.evaluate_completion(ddpm, lidar, planes, [KIND], methods=E2E_METHODS, num_steps=4, seed=SEED, batch_size=2,
                                                     ensemble=3, keep=True, **kw)
    with pytest.raises(ValueError):
        completion.evaluate_completion(ddpm, lidar, planes, [KIND], methods=("linear",), ensemble=3, ensemble_coherence=True, coherence_offsets=((0, W),))
    return go(ensemble_coherence=True), go(), lidar


def test_without_the_option_the_document_is_what_it_was(runs):
    (res, kept), (res0, kept0), _ = runs
    for method in E2E_METHODS:
        e, e0 = res[KIND][method]["ensemble"], res0[KIND][method]["ensemble"]
        assert set(e0) == {"members", "counts", "sums", "micro", "macro", "rank_histogram", "consensus"} and set(e) == set(e0) | {"coherence"}
        assert set(res[KIND][method]) == set(res0[KIND][method]) == {"counts", "sums", "micro", "macro", "ensemble"}
        assert completion.jsonable({k: v for k, v in e.items() if k != "coherence"}) == completion.jsonable(e0)
        k, k0 = kept[KIND]["ensemble"][method], kept0[KIND]["ensemble"][method]
        assert set(k0) == {"raw", "member", "rank", "consensus_raw", "maps", "x_out"} and set(k) == set(k0) | {"counts", "dist", "vario", "offsets"}
        assert all(torch.equal(k[n], k0[n]) for n in ("raw", "member", "rank", "consensus_raw", "maps"))
    assert set(kept[KIND]) == set(kept0[KIND])


def test_the_coherence_numbers_equal_the_oracle_on_the_kept_tensors(runs):
    (res, kept), _, lidar = runs
    k = kept[KIND]
    target, mask = k["target"].numpy(), k["mask"].numpy()
    close = lambda got, want: np.allclose(np.asarray(got, np.float64), np.asarray(want, np.float64), rtol=1e-12, atol=0, equal_nan=True)
    for method, K in (("dpmpp", 3), ("linear", 1)):
        e, t = res[KIND][method]["ensemble"]["coherence"], k["ensemble"][method]
        assert t["offsets"] == completion.DEFAULT_OFFSETS and e["offsets"] == [list(o) for o in completion.DEFAULT_OFFSETS]
        x = t["x_out"] if K > 1 else k["x_out"][method][:, None]
        samples = lidar.postprocess(x.flatten(0, 1).to(DEV).clamp(-1, 1)).reshape(2, K, 5, H, W).cpu().numpy()
        wcounts, wdist, wvario = O.scores(samples, target, mask, LO, HI, completion.DEFAULT_OFFSETS)
        counts, dist, vario = (t[n].numpy() for n in ("counts", "dist", "vario"))
        assert np.array_equal(counts, wcounts) and wcounts[:, 1].min() > 100 and np.array_equal(counts, t["raw"].numpy()[:, :2])
        check_dist(dist, wdist, method)
        check_vario(vario, wvario, method)
        assert (wvario[:, 0, :, 0] > 0).all()
        # the document: the oracle's formulas on the kept tensors
        per_scan, micro = O.derived(counts, dist, vario), O.derived(counts.sum(0), np.zeros_like(dist[0]), vario.sum(0))
        assert e["counts"] == {"scans": 2, "members": K, "unknown": int(counts[:, 0].sum()), "evaluated": int(counts[:, 1].sum()),
                               "pairs": vario[:, 0, :, 0].sum(0).astype(int).tolist()}
        for name in completion.COHERENCE_DERIVED_NAMES:
            with np.errstate(invalid="ignore"):
                every = np.isnan(per_scan[name]).all(0)
                mean = np.where(every, np.nan, np.nanmean(np.where(every, 0.0, per_scan[name]), axis=0))
            assert close(e["macro"][name], mean), (method, name, e["macro"][name], mean)
            if name.startswith("variogram"):
                assert close(e["micro"][name], micro[name]), (method, name)
            else:
                assert name not in e["micro"]
        print(method, "energy_depth", e["macro"]["energy_depth"], "diversity_depth", e["macro"]["diversity_depth"], "variogram_total_depth",
              e["micro"]["variogram_total_depth"])


def test_a_deterministic_method_is_an_ensemble_of_one(runs):
    (res, kept), _, _ = runs
    e = res[KIND]["linear"]
    c = e["ensemble"]["coherence"]
    assert c["counts"]["members"] == 1 and res[KIND]["dpmpp"]["ensemble"]["coherence"]["counts"]["members"] == 3
    energy, rmse = c["macro"]["energy_depth"], e["macro"]["rmse_depth"]
    print("linear: energy_depth", energy, "rmse_depth", rmse)
    assert rmse > 0 and abs(energy - rmse) <= BAR * rmse
    assert c["macro"]["energy_fair_depth"] is None or np.isnan(c["macro"]["energy_fair_depth"])
    assert kept[KIND]["ensemble"]["linear"]["dist"].shape == (2, 2, 2, 2) and kept[KIND]["ensemble"]["dpmpp"]["dist"].shape == (2, 2, 4, 4)
    assert res[KIND]["dpmpp"]["ensemble"]["coherence"]["macro"]["diversity_depth"] > 0


def test_completion_eval_with_the_coherence_scores(files):
    tmp, ckpt = files
    out = tmp / "eval" / "completion.json"
    r = subprocess.run([sys.executable, f"{ROOT}/completion_eval.py", "--ckpt", str(ckpt), "--real_scans", str(tmp / "scans"), "--methods", *E2E_METHODS,
                        "--num_steps", "2", "--batch_size", "2", "--seed", str(SEED), "--corruption", KIND, "--ensemble", "2", "--ensemble_coherence",
                        "--coherence_offsets", "0,1 1,-1", "--out", str(out)], cwd=tmp, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert any("2 members: CRPS depth" in line and "energy depth" in line and "variogram depth" in line for line in r.stdout.splitlines()), r.stdout
    text = out.read_text()
    assert "NaN" not in text and "Infinity" not in text
    doc = json.loads(text)
    assert doc["info"]["ensemble"] == 2 and doc["info"]["ensemble_coherence"] is True
    for method, K in (("dpmpp", 2), ("linear", 1)):
        c = doc["results"][KIND][method]["ensemble"]["coherence"]
        assert c["offsets"] == [[0, 1], [1, -1]] and c["counts"]["members"] == K and c["counts"]["scans"] == 2 and min(c["counts"]["pairs"]) > 100
        assert c["macro"]["energy_depth"] > 0 and len(c["macro"]["variogram_depth"]) == 2 and c["micro"]["variogram_total_depth"] > 0
        assert (c["macro"]["energy_fair_depth"] is None) == (K == 1)
