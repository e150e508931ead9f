"""CPU tests of the projection's specification and host side: the numpy closed form (tests/golden/make_golden_projection.py) against
the reference's recorded results (tests/golden/projection.npz), file loading, option parsing, argument validation."""
import ctypes
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
import make_golden_projection as G  # noqa: E402

from r2dm_amd import _lib, projection  # noqa: E402


@pytest.fixture(scope="module")
def golden_file():
    with np.load(f"{GOLDEN}/projection.npz") as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(G.CASES))
def test_numpy_closed_form_reproduces_the_reference(name, golden_file):
    """The specification the kernels implement -- the reference's expressions, the closed form of its scan-unfolding loop, nearest
    point per cell -- gives the reference's winner in every cell and its depth plane bit for bit."""
    H, W, unfolding, rings = G.CASES[name][:4]
    pts = G.make_cloud(name)
    idx, planes = G.project_numpy(pts, H, W, unfolding)
    want_idx, want_depth = golden_file[f"idx_{name}"], golden_file[f"depth_{name}"]
    keep = np.ones((H, W), bool)
    if rings == "free":
        keep = ~np.unpackbits(golden_file[f"skip_{name}"]).astype(bool).reshape(H, W)
        occupied = want_idx >= 0
        assert (~keep & occupied).sum() <= G.SKIP_CAP * occupied.sum()
        assert np.array_equal(keep, ~G.edge_cells(pts, H, W)[0])
    assert np.array_equal(idx[keep], want_idx[keep])
    assert np.array_equal(planes[4].view(np.uint32)[keep], want_depth.view(np.uint32)[keep])
    assert (want_idx >= 0).sum() > 0.5 * H * W and (want_idx < 0).any()


def test_centred_clouds_cover_the_cases_of_the_issue(golden_file):
    """Both ends of the depth window on the value and one ulp either side; ring counts H - 3, H, H + 1, H + 3; a scan starting mid-ring."""
    for name in ("sph_8x32", "sph_64x1024", "unf_8x32_r8"):
        d = golden_file[f"depth_{name}"]
        for t in G.SPECIAL:
            assert (d == t).any(), (name, t)
    assert {G.CASES[n][3] - G.CASES[n][0] for n in G.CASES if G.CASES[n][2]} >= {-3, 0, 1, 3}
    mid = G.make_cloud("unf_8x32_r8_mid")
    assert not (mid[-1, 0] >= 0 and mid[-1, 1] < 0 and mid[0, 0] >= 0 and mid[0, 1] >= 0), "the file does not start on a delimiter"
    assert (G.unfolding_rows(G.make_cloud("unf_8x32_r9"), 8) == 7).sum() > 0


def test_unfolding_closed_form_against_the_loop():
    """kitti_360.py:52-74 written out as its loop, on quadrant sequences with fewer, as many and more delimiters than rows."""
    g = np.random.Generator(np.random.PCG64(0))
    for H in (4, 8):
        for rings in range(0, H + 5):
            quad = np.concatenate([np.repeat([0, 1, 2, 3], g.integers(1, 4, size=4)) for _ in range(rings)] + [np.zeros(0, np.int64)])
            quad = np.roll(quad, int(g.integers(0, 5))) if len(quad) else np.array([2, 2, 1])
            pts = np.array([[1, 1], [-1, 1], [-1, -1], [1, -1]], np.float32)[quad]
            pts = np.concatenate([pts, np.ones((len(pts), 2), np.float32)], 1)
            delim = np.where((np.roll(quad, 1) - quad) == 3)[0]
            inds = list(delim) + [len(pts)]
            want = np.zeros(len(pts), np.int64)
            cur = H - 1
            for i in reversed(range(len(delim))):
                want[inds[i]:inds[i + 1]] = cur
                if cur >= 0:
                    cur -= 1
                else:
                    break
            want[want < 0] += H  # (the scatter's negative index wraps)
            assert np.array_equal(G.unfolding_rows(pts, H), want), (H, rings)


def test_parse_projection():
    assert projection.parse_projection("unfolding-2048") == (True, 2048)
    assert projection.parse_projection("spherical-1024") == (False, 1024)
    for bad in ("cylindrical-1024", "unfolding", "unfolding-", "unfolding-wide", "spherical-0", "spherical-1024-2", ""):
        with pytest.raises(ValueError, match="unknown projection"):
            projection.parse_projection(bad)


def test_load_scans(tmp_path):
    a, b = G.make_cloud("sph_8x32"), G.make_cloud("unf_8x32_r5")
    a.tofile(tmp_path / "a.bin")
    b.tofile(tmp_path / "b.bin")
    (tmp_path / "empty.bin").write_bytes(b"")
    pts, off = projection.load_scans([tmp_path / "a.bin", tmp_path / "empty.bin", tmp_path / "b.bin"])
    assert pts.dtype == np.float32 and off.dtype == np.int64
    assert off.tolist() == [0, len(a), len(a), len(a) + len(b)]
    assert np.array_equal(pts.view(np.uint32), np.concatenate([a, b]).view(np.uint32))
    pts, off = projection.load_scans([])
    assert pts.shape == (0, 4) and off.tolist() == [0]
    (tmp_path / "torn.bin").write_bytes(a.tobytes()[:-6])
    with pytest.raises(ValueError, match="torn.bin"):
        projection.load_scans([tmp_path / "a.bin", tmp_path / "torn.bin"])
    with pytest.raises(FileNotFoundError):
        projection.load_scans([tmp_path / "missing.bin"])


def test_project_scans_refuses_bad_arguments_before_touching_the_gpu():
    pts = G.make_cloud("sph_8x32")
    off = np.array([0, len(pts)], np.int64)
    with pytest.raises(ValueError, match="layout"):
        projection.project_scans(pts, off, layout="xyz")
    with pytest.raises(ValueError, match=r"\(total,4\)"):
        projection.project_scans(pts[:, :3], off)
    with pytest.raises(ValueError, match="out_width"):
        projection.project_scans(pts, off, W=32, out_width=33)
    with pytest.raises(ValueError, match="out_width"):
        projection.project_scans(pts, off, W=32, out_width=0)
    for bad in ([0, len(pts) - 1], [1, len(pts)], [0, 900, 800, len(pts)], [[0, len(pts)]], []):
        with pytest.raises(ValueError, match="offsets"):
            projection.project_scans(pts, np.array(bad, np.int64))
    with pytest.raises(ValueError, match=r"\(B,6,H,W\)"):
        projection.known_from_scan(torch.zeros(1, 5, 8, 32), None, (8, 32))
    # no CPU fallback: a CPU tensor is refused, and so is a numpy cloud where there is no device
    with pytest.raises(_lib.R2DMError, match="no CPU fallback"):
        projection.project_scans(torch.from_numpy(pts), off)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.R2DMError, match="no CPU fallback"):
            projection.project_scans(pts, off)


def test_c_abi_refuses_bad_arguments_with_a_status():
    """Argument errors come back as a status and a message (no launch, no fault): checked before any device call."""
    L = _lib.lib()
    I64 = ctypes.POINTER(ctypes.c_int64)
    off = (ctypes.c_int64 * 3)(0, 10, 20)
    fake = 1 << 20  # stands for device memory: never dereferenced by a refused call

    def call(points=fake, offsets=off, out=fake, batch=2, H=8, W=32, out_width=32, unfolding=1, apply_mask=1, layout=0, scratch=fake,
             scratch_bytes=1 << 30):
        rc = L.r2dm_project_scans(points, ctypes.cast(offsets, I64) if offsets is not None else None, out, batch, H, W, out_width, unfolding, 1.45,
                                  80.0, apply_mask, layout, scratch, scratch_bytes, None)
        return rc, L.r2dm_last_error().decode()

    for kw, msg in [(dict(out=None), "null"), (dict(offsets=None), "null"), (dict(scratch=None), "null"), (dict(points=None), "null"),
                    (dict(batch=0), "batch"), (dict(batch=70000), "batch"), (dict(H=0), "cells"), (dict(W=-1), "cells"),
                    (dict(H=1 << 15, W=1 << 15), "cells"), (dict(out_width=33), "out_width"), (dict(out_width=0), "out_width"),
                    (dict(layout=2), "layout"), (dict(unfolding=2), "0 or 1"), (dict(apply_mask=-1), "0 or 1"),
                    (dict(points=fake + 4), "aligned"), (dict(scratch=fake + 64), "aligned"), (dict(scratch_bytes=100), "scratch too small"),
                    (dict(offsets=(ctypes.c_int64 * 3)(1, 10, 20)), "offsets"), (dict(offsets=(ctypes.c_int64 * 3)(0, 10, 5)), "offsets"),
                    (dict(offsets=(ctypes.c_int64 * 3)(0, 10, 1 << 31)), "points")]:
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
    assert L.r2dm_project_scratch_bytes(1000, 2, 64, 2048, 0) >= 2 * 64 * 2048 * 8
    assert L.r2dm_project_scratch_bytes(1000, 2, 64, 2048, 1) > L.r2dm_project_scratch_bytes(1000, 2, 64, 2048, 0)
    for bad in [(-1, 2, 64, 2048, 1), (1 << 31, 2, 64, 2048, 1), (10, 0, 64, 2048, 1), (10, 2, 0, 2048, 1), (10, 2, 1 << 15, 1 << 15, 0)]:
        assert L.r2dm_project_scratch_bytes(*bad) == 0, bad


@pytest.mark.parametrize("script, options", [
    ("evaluate.py", ["--ckpt", "--sample_dir", "--dataset", "--batch_size", "--num_workers", "--real_set", "--real_dir", "--real_scans"]),
    ("completion_demo.py", ["--ckpt", "--num_steps", "--num_resample_steps", "--jump_length", "--seed", "--scan", "--out"]),
])
def test_script_options(script, options):
    r = subprocess.run([sys.executable, f"{ROOT}/{script}", "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for o in options:
        assert o in r.stdout, (script, o)


def test_completion_demo_masks_are_the_references_draws():
    sys.path.insert(0, ROOT)
    import completion_demo

    H, W = 16, 128
    mask = completion_demo.corruption_masks(torch.zeros(1, 2, H, W), seed=7)
    torch.manual_seed(7)
    want = torch.zeros(4, 2, H, W)
    want[0, ...] = 1
    want[1, :, ::4] = 1
    want[2, :] = torch.empty(H, 1).bernoulli_(0.5)
    want[3, :] = torch.empty(H, W).bernoulli_(0.1)
    assert torch.equal(mask, want) and mask.device.type == "cpu"
    assert 0 < mask[2].mean() < 1 and 0.03 < mask[3].mean() < 0.2
