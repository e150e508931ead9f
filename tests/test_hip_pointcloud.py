"""-m gpu: range images -> point clouds (r2dm_amd/csrc/pointcloud.hip) against the contract's numpy restatement
(tests/pointcloud_oracle.py) applied to ``lidar_utils.postprocess(x)``, bit for bit; the round trip through the projection; the
scripts' new flags."""
import functools
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, GOLDEN_RES, ROOT, synthetic_ckpt

sys.path.insert(0, GOLDEN)
sys.path.insert(0, f"{ROOT}/tests")
import make_golden_pointcloud as G  # noqa: E402  (the golden's mask)
import pointcloud_oracle as PO  # noqa: E402

import r2dm_amd  # noqa: E402
from r2dm_amd import pointcloud, projection  # noqa: E402
from r2dm_amd.synthetic import hdl64e_ray_angles  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
MIN_DEPTH, MAX_DEPTH = 1.45, 80.0
FORMATS = ["log_depth", "inverse_depth", "depth"]
# (B,H,W) -> the scans of the batch.  (3,5,104): 520 positions a scan -- the third block of a scan is short, rows straddle blocks, W
# is no multiple of 64.  (2,64,1024): 256 blocks a scan, 513 block counts: a prefix sum of three rounds.
MIXES = {
    "3x5x104": ((5, 104), ["random", "empty", "inside"]),
    "2x64x1024": ((64, 1024), ["random", "empty"]),
    "2x64x1024_inside": ((64, 1024), ["inside", "random"]),
}


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def lidar_of(H, W, fmt, rays="edge"):
    if rays == "centred":
        ang = pointcloud.centred_ray_angles(H, W)
    else:
        # the project's default grid; on the small image every row's azimuths are turned by another few columns: row_start differs
        ang = hdl64e_ray_angles(H, W)
        if H == 5:
            ang = torch.stack([ang[0, 0], torch.stack([ang[0, 1, h].roll(7 * h) for h in range(H)])])[None]
    return r2dm_amd.LiDARUtility((H, W), fmt, MIN_DEPTH, MAX_DEPTH, ray_angles=ang).to(DEV)


@functools.lru_cache(maxsize=None)
def batch(mix, fmt):
    """(x (B,2,H,W) on the GPU, its post-processed planes (B,5,H,W) as numpy), computed once and left unchanged."""
    (H, W), kinds = MIXES[mix]
    g = np.random.Generator(np.random.PCG64(11 + len(mix) + FORMATS.index(fmt)))
    scans = []
    for kind in kinds:
        if kind == "empty":
            s = np.full((2, H, W), -1.0)
        elif kind == "inside":  # d in [0.25, 0.9]: log 2 .. 51 m, inverse 1.6 .. 5.8 m, linear 20 .. 72 m
            s = g.uniform(-0.5, 0.8, size=(2, H, W))
        else:
            s = g.uniform(-1.2, 1.2, size=(2, H, W))
            at = g.permutation(2 * H * W)[:max(12, H * W // 50)]
            s.reshape(-1)[at] = np.resize([np.nan, np.inf, -np.inf], len(at))
        scans.append(s)
    x = torch.from_numpy(np.stack(scans).astype(np.float32)).to(DEV)
    post = lidar_of(H, W, fmt).postprocess(x).cpu().numpy()
    post.setflags(write=False)
    return x, post


def check_against_oracle(got, post, row_start, order, keep):
    points, offsets, index = got
    want_p, want_o, want_i = PO.export(post, row_start, order, *keep)
    assert isinstance(offsets, np.ndarray) and offsets.dtype == np.int64 and np.array_equal(offsets, want_o), (offsets, want_o)
    assert points.is_cuda and points.dtype == torch.float32 and tuple(points.shape) == want_p.shape
    assert index.dtype == torch.int32 and np.array_equal(index.cpu().numpy(), want_i)
    bad = bits(points) != bits(want_p)
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} values differ, first at {tuple(np.argwhere(bad)[0])}"


# ---- 1. parity, bit for bit --------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("mix", list(MIXES))
def test_matches_the_oracle_bit_for_bit(mix, fmt):
    (H, W), kinds = MIXES[mix]
    x, post = batch(mix, fmt)
    lidar = lidar_of(H, W, fmt)
    row_start = pointcloud.scan_row_start(lidar.ray_angles)
    assert (len(set(row_start.tolist())) == H) if H == 5 else (row_start == W // 2).all()
    planes = torch.from_numpy(post).to(DEV)
    for order in ("scan", "image"):
        for layout, src in (("model", x), ("sample", planes)):
            got = pointcloud.images_to_points(src, lidar, layout=layout, order=order, return_index=True)
            check_against_oracle(got, post, row_start, order, (MIN_DEPTH, MAX_DEPTH))
            counts = np.diff(got[1])
            assert counts[kinds.index("empty")] == 0 if "empty" in kinds else True, "an empty scan repeats the offset"
            if "inside" in kinds:
                assert counts[kinds.index("inside")] == H * W
            assert 0 < counts[kinds.index("random")] < H * W
    # sample layout, image order: no lidar_utils needed (every pixel with a depth > 0)
    got = pointcloud.images_to_points(planes, layout="sample", order="image", return_index=True)
    check_against_oracle(got, post, None, "image", (0.0, np.inf))
    assert len(pointcloud.images_to_points(planes, layout="sample", order="image")) == 2


@pytest.mark.parametrize("mix", ["3x5x104", "2x64x1024"])
def test_a_narrower_keep_window(mix):
    """evaluate.py's window (0.5, 63) m inside the checkpoint's (1.45, 80) m."""
    (H, W), _ = MIXES[mix]
    x, post = batch(mix, "log_depth")
    lidar = lidar_of(H, W, "log_depth")
    row_start = pointcloud.scan_row_start(lidar.ray_angles)
    assert ((post[:, 0] >= 63) & (post[:, 0] < 80)).any()
    for layout, src in (("model", x), ("sample", torch.from_numpy(post).to(DEV))):
        got = pointcloud.images_to_points(src, lidar, layout=layout, keep_min=0.5, keep_max=63.0, return_index=True)
        check_against_oracle(got, post, row_start, "scan", (0.5, 63.0))


def test_ray_angles_override_sets_the_order_and_the_points():
    """``ray_angles=`` replaces the utility's angles: for the order (both layouts) and for the points (layout "model")."""
    H, W = 5, 104
    x, _ = batch("3x5x104", "log_depth")
    edge, centred = lidar_of(H, W, "log_depth"), lidar_of(H, W, "log_depth", "centred")
    post = centred.postprocess(x).cpu().numpy()
    got = pointcloud.images_to_points(x, edge, ray_angles=pointcloud.centred_ray_angles(H, W), return_index=True)
    check_against_oracle(got, post, np.full(H, W // 2 - 1), "scan", (MIN_DEPTH, MAX_DEPTH))
    got = pointcloud.images_to_points(torch.from_numpy(post).to(DEV), layout="sample", ray_angles=pointcloud.centred_ray_angles(H, W)[0].to(DEV),
                                      keep_min=MIN_DEPTH, keep_max=MAX_DEPTH, return_index=True)
    check_against_oracle(got, post, np.full(H, W // 2 - 1), "scan", (MIN_DEPTH, MAX_DEPTH))


# ---- 2. rows, index, offsets -------------------------------------------------------------------------
@pytest.mark.parametrize("mix", list(MIXES))
def test_rows_are_the_planes_at_their_index(mix):
    (H, W), _ = MIXES[mix]
    x, post = batch(mix, "log_depth")
    lidar = lidar_of(H, W, "log_depth")
    planes = torch.from_numpy(post).to(DEV)
    for layout, src in (("model", x), ("sample", planes)):
        points, offsets, index = pointcloud.images_to_points(src, lidar, layout=layout, return_index=True)
        assert offsets[0] == 0 and offsets[-1] == len(points) == len(index) and (np.diff(offsets) >= 0).all() and len(offsets) == len(x) + 1
        for b in range(len(x)):
            idx = index[offsets[b]:offsets[b + 1]].long()
            assert len(torch.unique(idx)) == len(idx) and (len(idx) == 0 or (0 <= idx.min() and idx.max() < H * W))
            want = planes[b].flatten(1)[1:5][:, idx].T
            assert torch.equal(points[offsets[b]:offsets[b + 1]].contiguous().view(torch.int32), want.contiguous().view(torch.int32))
            d = planes[b, 0].flatten()[idx]
            assert ((d > MIN_DEPTH) & (d < MAX_DEPTH)).all()


# ---- 3. the same bits on every call ------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["model", "sample"])
def test_two_calls_give_the_same_bits(layout):
    x, post = batch("2x64x1024", "log_depth")
    lidar = lidar_of(64, 1024, "log_depth")
    src = x if layout == "model" else torch.from_numpy(post).to(DEV)
    a = pointcloud.images_to_points(src, lidar, layout=layout, return_index=True)
    b = pointcloud.images_to_points(src, lidar, layout=layout, return_index=True)
    assert np.array_equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert torch.equal(a[0].contiguous().view(torch.int32), b[0].contiguous().view(torch.int32))


# ---- 4. round trip through the projection ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def round_trip_input(B, H, W, kind):
    g = np.random.Generator(np.random.PCG64(17 + B + H))
    x = np.stack([g.uniform(-0.5, 0.9, size=(B, H, W)), g.uniform(-1.0, 1.0, size=(B, H, W))], 1).astype(np.float32)
    valid = G.valid_mask(H, W, G.CASES[kind])
    x[:, :, ~valid] = -1.0
    x = torch.from_numpy(x).to(DEV)
    post = lidar_of(H, W, "log_depth", "centred").postprocess(x)
    assert torch.equal(post[:, 0] > 0, torch.from_numpy(valid).to(DEV).expand(B, H, W))
    return x, post, valid


@pytest.mark.parametrize("mode", ["unfolding", "spherical"])
@pytest.mark.parametrize("kind", list(G.CASES))
@pytest.mark.parametrize("B, H, W", [(2, 8, 64), (1, 64, 1024)])
def test_scan_order_export_projects_back_to_its_image(B, H, W, kind, mode):
    """images -> scans (scan order, rays at the cell centres) -> project_scans gives the post-processed image back where it has a
    point, and empty cells elsewhere: x, y, z, reflectance and the mask bit-exact, depth (recomputed by the projection as the fp32
    norm of the coordinates) within 1e-6 relative."""
    x, post, valid = round_trip_input(B, H, W, kind)
    lidar = lidar_of(H, W, "log_depth", "centred")
    unfolding = mode == "unfolding"

    def back(order):
        points, offsets = pointcloud.images_to_points(x, lidar, order=order, ray_angles=pointcloud.centred_ray_angles(H, W))
        assert offsets.tolist() == [int(valid.sum()) * b for b in range(B + 1)]
        return projection.project_scans(points, offsets, H=H, W=W, scan_unfolding=unfolding, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH)

    got = back("scan")
    v = torch.from_numpy(valid).to(DEV).expand(B, H, W)
    want = torch.where(v[:, None], post[:, [1, 2, 3, 4]], torch.zeros((), device=DEV))
    assert torch.equal(got[:, 5] == 1, v) and ((got[:, 5] == 0) | (got[:, 5] == 1)).all()
    bad = bits(got[:, :4]) != bits(want)
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} values differ, first at {tuple(np.argwhere(bad)[0])}"
    rel = ((got[:, 4].double() - post[:, 0].double()).abs() / post[:, 0].double())[v]
    print(f"{B}x{H}x{W} {kind} {mode}: depth off by at most {rel.max().item():.3e} relative")
    assert rel.max().item() <= 1e-6 and not got[:, 4][~v].any()
    if unfolding:  # the order matters: row-major rows get other rows
        other = back("image")
        assert (bits(other[:, :4]) != bits(want)).any()


# ---- 5. the scripts ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ckpt_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("ckpt") / "synthetic.pth"
    torch.save(synthetic_ckpt(resolution=GOLDEN_RES), p)
    return p


def _run(cmd, cwd):
    r = subprocess.run([sys.executable] + [str(c) for c in cmd], cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_sample_and_save_points_dir(ckpt_file, tmp_path):
    common = ["sample_and_save.py", "--ckpt", ckpt_file, "--batch_size", "2", "--num_samples", "3", "--num_steps", "2"]
    _run(common + ["--output_dir", tmp_path / "plain"], ROOT)
    _run(common + ["--output_dir", tmp_path / "with", "--points_dir", tmp_path / "scans"], ROOT)
    _, lidar, _ = r2dm_amd.setup_model(str(ckpt_file), device=DEV, show_info=False, max_batch=1)
    assert sorted(p.name for p in (tmp_path / "scans").iterdir()) == [f"samples_{s:010d}.bin" for s in range(3)]
    assert sorted(p.name for p in (tmp_path / "with").iterdir()) == sorted(p.name for p in (tmp_path / "plain").iterdir())
    for s in range(3):
        name = f"samples_{s:010d}"
        a, b = torch.load(tmp_path / "with" / f"{name}.pth"), torch.load(tmp_path / "plain" / f"{name}.pth")
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the flag changes nothing else"
        points, offsets = pointcloud.images_to_points(a[None].to(DEV), lidar, layout="sample", order="scan")
        got, got_off = projection.load_scans([tmp_path / "scans" / f"{name}.bin"])
        assert np.array_equal(got_off, offsets) and len(got) > 0
        assert np.array_equal(bits(got), bits(points))


def test_generate_points_dir_and_ply(ckpt_file, tmp_path):
    out = tmp_path / "samples.pt"
    _run([f"{ROOT}/generate.py", "--ckpt", ckpt_file, "--batch_size", "2", "--sampling_steps", "2", "--seed", "1", "--output", out,
          "--points_dir", tmp_path / "scans", "--points_ply"], tmp_path)
    files = sorted((tmp_path / "scans").iterdir())
    assert [p.name for p in files] == ["samples_0000.bin", "samples_0000.ply", "samples_0001.bin", "samples_0001.ply"]
    got, got_off = projection.load_scans(files[0::2])
    _, lidar, _ = r2dm_amd.setup_model(str(ckpt_file), device=DEV, show_info=False, max_batch=1)
    points, offsets = pointcloud.images_to_points(torch.load(out)["points"].to(DEV), lidar, layout="sample", order="scan")
    assert np.array_equal(got_off, offsets) and np.array_equal(bits(got), bits(points)) and len(got) > 0
    for k, ply in enumerate(files[1::2]):
        head, payload = ply.read_bytes().split(b"end_header\n", 1)
        n = int(got_off[k + 1] - got_off[k])
        assert f"element vertex {n}\n".encode() in head and b"property uchar blue" in head and len(payload) == 19 * n
        rows = np.frombuffer(payload, np.uint8).reshape(n, 19)
        assert np.array_equal(rows[:, :16].copy().view(np.uint32), bits(got[got_off[k]:got_off[k + 1]]))


def test_completion_demo_out_scan(ckpt_file, tmp_path):
    g = np.random.Generator(np.random.PCG64(9))
    k = g.integers(0, 2**24, size=(4, 20_000)) / 2.0**24
    phi, theta, depth = np.deg2rad(-24.0 + 26.0 * k[0]), (2.0 * k[1] - 1.0) * np.pi, 2.0 + 60.0 * k[2]
    scan = np.stack([depth * np.cos(phi) * np.cos(theta), depth * np.cos(phi) * np.sin(theta), depth * np.sin(phi), k[3]], 1).astype(np.float32)
    scan.tofile(tmp_path / "scan.bin")
    out = tmp_path / "demo" / "completion.png"
    _run([f"{ROOT}/completion_demo.py", "--ckpt", ckpt_file, "--scan", tmp_path / "scan.bin", "--out", out, "--num_steps", "2",
          "--num_resample_steps", "2", "--jump_length", "1", "--out_scan", tmp_path / "done" / "completed.bin"], tmp_path)
    _, lidar, _ = r2dm_amd.setup_model(str(ckpt_file), device=DEV, show_info=False, max_batch=1)
    x_out = torch.load(out.parent / "completion.pt")["x_out"]
    points, offsets = pointcloud.images_to_points(x_out[:1].to(DEV), lidar, layout="model", order="scan")
    got, got_off = projection.load_scans([tmp_path / "done" / "completed.bin"])
    assert np.array_equal(got_off, offsets) and np.array_equal(bits(got), bits(points)) and len(got) > 0
