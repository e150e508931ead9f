"""-m gpu: raw scans -> range images (r2dm_amd/csrc/projection.hip) against the reference's load_points_as_images
(tests/golden/projection.npz, tests/golden/make_golden_projection.py), bit for bit, and the scripts built on it."""
import ctypes
import functools
import json
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, GOLDEN_RES, ROOT, synthetic_ckpt

sys.path.insert(0, GOLDEN)
import make_golden_projection as G  # noqa: E402  (the fixture's integer-only input generators and the numpy specification)

import r2dm_amd  # noqa: E402
from r2dm_amd import _lib, projection  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def golden_file():
    with np.load(f"{GOLDEN}/projection.npz") as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def case(name):
    """(points, unmasked planes (6,H,W) of the reference, cells to compare (H,W) bool)"""
    H, W = G.CASES[name][:2]
    z = golden_file()
    pts, idx, depth = G.make_cloud(name), z[f"idx_{name}"], z[f"depth_{name}"]
    planes = G.planes_of(pts, idx)
    planes[4] = depth  # the reference's own depth plane (tests/test_projection_cpu.py holds the rebuilt one to it)
    planes[5] = ((depth >= np.float32(G.MIN_DEPTH)) & (depth <= np.float32(G.MAX_DEPTH))) & (idx >= 0)
    skip = np.unpackbits(z[f"skip_{name}"]).astype(bool).reshape(H, W) if f"skip_{name}" in z else np.zeros((H, W), bool)
    for a in (pts, planes, skip):
        a.setflags(write=False)
    return pts, planes, ~skip


def batch_of(clouds):
    off = np.zeros(len(clouds) + 1, np.int64)
    np.cumsum([len(c) for c in clouds], out=off[1:])
    return np.concatenate(clouds), off


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want, keep=None):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (g.shape, w.shape)
    bad = g != w
    if keep is not None:
        bad &= keep
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} values differ, first at {tuple(np.argwhere(bad)[0])}"


def masked(planes):
    with np.errstate(invalid="ignore"):
        return planes * planes[[5]]


# name -> (H, W, scan_unfolding, scans of one batch; None: an empty scan)
GROUPS = {
    "sph_8x32": (8, 32, False, ["sph_8x32", None]),
    "unf_8x32": (8, 32, True, ["unf_8x32_r5", "unf_8x32_r8", None, "unf_8x32_r9", "unf_8x32_r11", "unf_8x32_r8_mid"]),
    "sph_64x1024": (64, 1024, False, [None, "sph_64x1024", "free_64x1024"]),
    # (the first scan, made for another grid and not compared, moves the second off a block boundary)
    "unf_64x1024": (64, 1024, True, ["unf_8x32_r8_mid", "unf_64x1024_r65", None]),
}


@functools.lru_cache(maxsize=None)
def group_output(group):
    """The unmasked planes of one batch (an empty scan among scans of unequal lengths), computed once."""
    H, W, unfolding, names = GROUPS[group]
    pts, off = batch_of([np.zeros((0, 4), np.float32) if n is None else case(n)[0] for n in names])
    out = projection.project_scans(pts, off, H=H, W=W, scan_unfolding=unfolding, apply_mask=False)
    assert out.shape == (len(names), 6, H, W) and out.dtype == torch.float32 and out.is_cuda
    return out


# ---- 1. the reference, bit for bit -------------------------------------------------------------------
@pytest.mark.parametrize("group", list(GROUPS))
def test_matches_the_reference_bit_for_bit(group):
    out = group_output(group)
    H, W = out.shape[-2:]
    compared = 0
    for b, name in enumerate(GROUPS[group][3]):
        if name is None:
            assert not out[b].any(), "an empty scan gives an empty image"
        elif G.CASES[name][:2] == (H, W):
            _, want, keep = case(name)
            same_bits(out[b], want, keep[None])
            compared += 1
    assert compared >= 1


def test_free_cloud_leaves_out_at_most_one_percent():
    _, want, keep = case("free_64x1024")
    occupied = want[4] > 0
    assert (~keep & occupied).sum() <= G.SKIP_CAP * occupied.sum()


@pytest.mark.parametrize("name", ["sph_8x32", "unf_8x32_r9"])
def test_load_points_as_images(name, tmp_path):
    pts, want, _ = case(name)
    H, W, unfolding = G.CASES[name][:3]
    path = tmp_path / "scan.bin"
    pts.tofile(path)
    img = projection.load_points_as_images(str(path), scan_unfolding=unfolding, H=H, W=W)
    assert isinstance(img, np.ndarray) and img.shape == (H, W, 6) and img.dtype == np.float32
    same_bits(np.moveaxis(img, -1, 0), want)  # unmasked: the reference's raw return value


# ---- 2. mask, layout, width --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sph_64x1024", "unf_8x32_r11"])
def test_mask_layout_and_width(name):
    pts, want, _ = case(name)
    H, W, unfolding = G.CASES[name][:3]
    off = np.array([0, len(pts)], np.int64)
    kw = dict(H=H, W=W, scan_unfolding=unfolding)
    m = masked(want)
    assert (want[5] == 0).any() and (want[4][want[5] == 0] > 0).any(), "the case has winners outside the depth window"
    same_bits(projection.project_scans(pts, off, **kw)[0], m)  # apply_mask is the default
    same_bits(projection.project_scans(pts, off, layout="sample", **kw)[0], m[[4, 0, 1, 2, 3]])
    same_bits(projection.project_scans(pts, off, out_width=W // 2, **kw)[0], m[:, :, 1::2])  # floor((j + 0.5) 2) = 2 j + 1
    same_bits(projection.project_scans(pts, off, out_width=W // 2, apply_mask=False, layout="sample", **kw)[0], want[[4, 0, 1, 2, 3]][:, :, 1::2])
    # another depth window
    other = want.copy()
    other[5] = (want[4] >= np.float32(10)) & (want[4] <= np.float32(50.5))
    same_bits(projection.project_scans(pts, off, min_depth=10.0, max_depth=50.5, **kw)[0], masked(other))


@pytest.mark.parametrize("out_width", [12, 16, 1])
def test_out_width_is_nearest_exact(out_width):
    pts, want, _ = case("sph_8x32")
    off = np.array([0, len(pts)], np.int64)
    got = projection.project_scans(pts, off, H=8, W=32, scan_unfolding=False, out_width=out_width)
    full = torch.from_numpy(masked(want))[None]
    same_bits(got, F.interpolate(full, size=(8, out_width), mode="nearest-exact"))


# ---- 3. a scan over many blocks ------------------------------------------------------------------------
def test_unfolding_prefix_count_across_many_blocks():
    H, W = 64, 2048
    scan = G.centred_unfolding(H, W, rings=64, mid=True, seed=21, sparse=True)  # ~118 k points: some 460 blocks of 256
    head = case("unf_8x32_r9")[0]                                               # 1601 points: the scan starts inside a block
    assert len(scan) > 100_000 and len(head) % 256
    # the closed form of the reference's loop, here in numpy
    x, y = scan[:, 0], scan[:, 1]
    quad = np.select([(x >= 0) & (y >= 0), (x < 0) & (y >= 0), (x < 0) & (y < 0), (x >= 0) & (y < 0)], [0, 1, 2, 3], 0)
    delim = np.roll(quad, 1) - quad == 3
    seg, D = np.cumsum(delim), int(delim.sum())
    assert D == 64 and not delim[0], "64 rings, starting mid-ring"
    r = H - 1 - (D - seg)
    rows = np.where(seg == 0, 0, np.where(r >= 0, r, np.where(r == -1, H - 1, 0)))
    _, w, depth, ok = G.grid_of(scan, H, W, True)
    assert np.array_equal(rows, G.unfolding_rows(scan, H))
    want = G.planes_of(scan, G.winners(rows, w, depth, ok, H, W))
    pts, off = batch_of([head, scan, head[:300]])
    out = projection.project_scans(pts, off, H=H, W=W, scan_unfolding=True, apply_mask=False)
    same_bits(out[1], want)
    # its neighbours in the batch (made for another grid: not held to numpy) are what they are alone
    for b, cloud in ((0, head), (2, head[:300])):
        same_bits(out[b], projection.project_scans(cloud, np.array([0, len(cloud)]), H=H, W=W, scan_unfolding=True, apply_mask=False)[0])


# ---- 4. ties -----------------------------------------------------------------------------------------
def test_lowest_index_wins_a_tie_on_every_call():
    pts, want, _ = case("sph_8x32")
    z = golden_file()
    win = z["idx_sph_8x32"][z["idx_sph_8x32"] >= 0][::3]
    first, last = pts[win].copy(), pts[win].copy()
    first[:, 3], last[:, 3] = 0.25, 0.75             # the same positions, told apart by the reflectance
    crowd = np.repeat(pts[win[:1]], 3000, axis=0)    # 3000 copies of one point: one cell, one depth
    crowd[:, 3] = np.arange(3000) / 4096.0
    cloud = np.concatenate([first, pts, last, crowd])
    off = np.array([0, len(cloud)], np.int64)
    a = projection.project_scans(cloud, off, H=8, W=32, scan_unfolding=False, apply_mask=False)
    b = projection.project_scans(cloud, off, H=8, W=32, scan_unfolding=False, apply_mask=False)
    same_bits(a, b)
    idx, planes = G.project_numpy(cloud, 8, 32, False)
    same_bits(a[0], planes)
    assert (np.sort(idx[idx >= 0])[:len(win)] == np.arange(len(win))).all(), "the first copies win their cells"
    expect = want.copy()
    cells = np.isin(z["idx_sph_8x32"], win)
    expect[3][cells] = 0.25
    same_bits(a[0], expect)


# ---- 5. order ----------------------------------------------------------------------------------------
def test_spherical_output_does_not_depend_on_the_order_of_the_points():
    pts, want, _ = case("sph_64x1024")
    perm = np.random.Generator(np.random.PCG64(5)).permutation(len(pts))
    off = np.array([0, len(pts)], np.int64)
    out = projection.project_scans(pts[perm], off, H=64, W=1024, scan_unfolding=False, apply_mask=False)
    same_bits(out[0], group_output("sph_64x1024")[1])
    same_bits(out[0], want)


# ---- 6. undefined inputs -----------------------------------------------------------------------------
def _with_undefined_rows(pts, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    bad = np.array([[np.nan, 1, 1, 0.5], [1, np.nan, 1, 0.5], [1, 1, np.nan, 0.5], [np.nan] * 4, [np.inf, 1, 1, 0.5], [1, -np.inf, 1, 0.5],
                    [1, 1, np.inf, 0.5], [np.inf, -np.inf, np.inf, 0.5], [0, 0, 0, 0.5], [-0.0, 0.0, -0.0, 0.5], [3e30, 1, 1, 0.5],
                    [1e-30, 0, 0, 0.5]], np.float32)
    bad = bad[g.integers(0, len(bad), size=200)]
    at = np.sort(g.integers(0, len(pts) + 1, size=len(bad)))
    return np.insert(pts, at, bad, axis=0)


@pytest.mark.parametrize("name", ["sph_8x32", "unf_8x32_r9"])
def test_undefined_inputs_stay_inside_the_output(name):
    pts, want, _ = case(name)
    H, W, unfolding = G.CASES[name][:3]
    cloud = _with_undefined_rows(pts, 6)
    assert not np.isfinite(cloud).all() and len(cloud) == len(pts) + 200
    # through the C ABI, with guard elements around the output and the scratch buffer
    L = _lib.lib()
    n, guard = 6 * H * W, 4096
    buf = torch.full((n + 2 * guard,), -7.0, device=DEV)
    dpts = torch.from_numpy(cloud).to(DEV)
    off = np.array([0, len(cloud)], np.int64)
    need = L.r2dm_project_scratch_bytes(len(cloud), 1, H, W, int(unfolding))
    scratch = torch.full((need // 4 + 2 * guard + 64,), -7.0, device=DEV)
    sptr = scratch.data_ptr() + 4 * guard
    sptr += (-sptr) % 256
    _lib.check(L.r2dm_project_scans(dpts.data_ptr(), off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), buf.data_ptr() + 4 * guard, 1, H, W, W,
                                    int(unfolding), 1.45, 80.0, 0, 0, sptr, need, _lib.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    assert (buf[:guard] == -7).all() and (buf[-guard:] == -7).all(), "written outside the output"
    lo, hi = (sptr - scratch.data_ptr()) // 4, (sptr - scratch.data_ptr() + need + 3) // 4
    assert (scratch[:lo] == -7).all() and (scratch[hi:] == -7).all(), "written outside the scratch buffer"
    out = buf[guard:guard + n].view(6, H, W)
    # the rule: a point whose depth is not a finite number > 0 wins no cell; it keeps its place in the sequence
    same_bits(out, G.project_numpy(cloud, H, W, unfolding)[1])
    assert np.isfinite(out.cpu().numpy()).all()
    if not unfolding:
        same_bits(out, want)  # the cells of the valid points are unchanged


# ---- 7. the scripts ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ckpt_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("ckpt") / "synthetic.pth"
    torch.save(synthetic_ckpt(resolution=GOLDEN_RES), p)
    return p


def _small_scans(n):
    """Scans of a few thousand points inside the BEV field (the free cloud's first points, rotated a little from scan to scan)."""
    pts = case("free_64x1024")[0]
    return [np.ascontiguousarray(pts[3000 * k:3000 * k + 2500 + 100 * k]) for k in range(n)]


def test_evaluate_real_scans_equals_real_dir_on_the_projected_scans(ckpt_file, tmp_path):
    from r2dm_amd.option import Config

    cfg = Config(**torch.load(ckpt_file)["cfg"])
    unfolding, width = projection.parse_projection(cfg.data.projection)
    H, W = GOLDEN_RES
    gen, scans_dir, real = tmp_path / "gen", tmp_path / "scans", tmp_path / "real"
    subprocess.run([sys.executable, "sample_and_save.py", "--ckpt", str(ckpt_file), "--output_dir", str(gen), "--batch_size", "2",
                    "--num_samples", "3", "--num_steps", "2"], cwd=ROOT, check=True, timeout=600)
    real.mkdir()
    scans = _small_scans(5)
    for k, s in enumerate(scans):  # nested, as KITTI-360 lays its sequences out
        d = scans_dir / f"seq_{k % 2}" / "velodyne_points" / "data"
        d.mkdir(parents=True, exist_ok=True)
        s.tofile(d / f"{k:010d}.bin")
    files = sorted(scans_dir.rglob("*.bin"))
    pts, off = projection.load_scans(files)
    imgs = projection.project_scans(pts, off, H=64, W=width, scan_unfolding=unfolding, layout="sample")
    imgs = F.interpolate(imgs, size=(H, W), mode="nearest-exact")
    assert (imgs[:, 0] > 0).any()
    for k, img in enumerate(imgs):
        torch.save(img.cpu(), real / f"{k:010d}.pth")

    def run(extra):
        before = set(tmp_path.glob("gen_*.json"))
        r = subprocess.run([sys.executable, f"{ROOT}/evaluate.py", "--ckpt", str(ckpt_file), "--sample_dir", str(gen), "--dataset", "test",
                            "--batch_size", "2", "--num_workers", "0"] + extra, cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        new = sorted(set(tmp_path.glob("gen_*.json")) - before)
        assert len(new) == 1
        return json.loads(new[0].read_text())

    a, b = run(["--real_scans", str(scans_dir)]), run(["--real_dir", str(real)])
    assert a["info"]["#real"] == b["info"]["#real"] == 5 and a["info"]["#fake"] == 3
    assert a["bev"] == b["bev"] and set(a["bev"]) == {"jsd", "mmd"}
    assert np.isfinite([a["bev"]["jsd"], a["bev"]["mmd"]]).all()


def test_completion_demo(ckpt_file, tmp_path):
    scan = tmp_path / "scan.bin"
    case("free_64x1024")[0].tofile(scan)
    out = tmp_path / "demo" / "completion.png"
    r = subprocess.run([sys.executable, f"{ROOT}/completion_demo.py", "--ckpt", str(ckpt_file), "--scan", str(scan), "--out", str(out),
                        "--num_steps", "2", "--num_resample_steps", "2", "--jump_length", "1", "--seed", "3"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    # a valid PNG of four columns: 2H + W + 2H + W rows of W pixels each, 2 pixels of padding around every cell
    import struct
    import zlib

    H, W = GOLDEN_RES
    data = out.read_bytes()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR"
    width, height, depth, colour = struct.unpack(">IIBB", data[16:26])
    assert (width, height, depth, colour) == (4 * (W + 2) + 2, 4 * H + 2 * W + 4, 8, 2)
    pos, idat = 8, b""
    while pos < len(data):
        (n,), tag = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        assert zlib.crc32(data[pos + 4:pos + 8 + n]) & 0xFFFFFFFF == struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]
        idat += data[pos + 8:pos + 8 + n] if tag == b"IDAT" else b""
        pos += 12 + n
    assert len(zlib.decompress(idat)) == height * (1 + 3 * width)

    state = torch.load(out.parent / "completion.pt")
    x_in, mask, x_out = state["x_in"], state["mask"], state["x_out"]
    assert x_in.shape == mask.shape == x_out.shape == (4, 2, H, W)
    # the masks are the reference's draws (completion_demo.py:81-87)
    torch.manual_seed(3)
    want_mask = torch.zeros(4, 2, H, W)
    want_mask[0, ...] = 1
    want_mask[1, :, ::4] = 1
    want_mask[2, :] = torch.empty(H, 1).bernoulli_(0.5)
    want_mask[3, :] = torch.empty(H, W).bernoulli_(0.1)
    assert torch.equal(mask, want_mask)

    # the same completion through the API
    ddpm, lidar, cfg = r2dm_amd.setup_model(str(ckpt_file), device=DEV, show_info=False, max_batch=4)
    unfolding, width = projection.parse_projection(cfg.data.projection)
    pts, off = projection.load_scans([scan])
    xyzrdm = projection.project_scans(pts, off, H=64, W=width, scan_unfolding=unfolding, min_depth=lidar.min_depth, max_depth=lidar.max_depth)
    known = projection.known_from_scan(xyzrdm, lidar, GOLDEN_RES)
    assert known.shape == (1, 2, H, W) and (known > -1).any() and known.min() >= -1 and known.max() <= 1
    m = mask.to(DEV)
    want_in = m * known + (1 - m) * -1
    assert torch.equal(x_in.to(DEV), want_in)
    want = ddpm.repaint(known=want_in, mask=m, num_steps=2, num_resample_steps=2, jump_length=1, progress=False,
                        rng=r2dm_amd.setup_rng(range(4), device=DEV)).clamp(-1, 1)
    assert torch.equal(x_out.to(DEV), want)
    # where the mask is 1 the output is the input, up to the last step's noise level: RePaint's final blend is
    # alpha_0 x_in + sigma_0 noise with log-SNR(0) = 15 (sigma_0 = sqrt(sigmoid(-15)) = 5.5e-4), |noise| < 6 over these 16 k draws
    sigma0 = float(torch.tensor(-15.0).sigmoid().sqrt())
    dev = ((x_out - x_in).abs() * mask).max().item()
    print(f"max |x_out - x_in| where mask == 1: {dev:.3e} (bound {6 * sigma0 + 1e-6:.3e})")
    assert dev <= 6 * sigma0 + 1e-6
    assert ((x_out - x_in).abs() * (1 - mask)).max() > 0.1, "the unknown region was completed"
