"""CPU tests of the point-cloud export's contract and host side: the numpy restatement (tests/pointcloud_oracle.py) against what the
reference's load_points_as_images made of its export (tests/golden/pointcloud.npz, tests/golden/make_golden_pointcloud.py), the
scan-order helpers, the writers, argument validation."""
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
sys.path.insert(0, f"{ROOT}/tests")
import make_golden_pointcloud as G  # noqa: E402
import pointcloud_oracle as PO  # noqa: E402

import r2dm_amd  # noqa: E402
from r2dm_amd import _lib, pointcloud, projection  # noqa: E402
from r2dm_amd.synthetic import hdl64e_ray_angles  # noqa: E402


@pytest.fixture(scope="module")
def golden_file():
    with np.load(f"{GOLDEN}/pointcloud.npz") as z:
        return {k: z[k] for k in z.files}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the order, held to the reference ------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.CASES))
@pytest.mark.parametrize("mode", ["unfolding", "spherical"])
def test_scan_order_export_projects_back_through_the_reference(name, mode, golden_file):
    """The oracle's scan-order export of an 8 x 64 image along centred rays is what the reference read (bit for bit), and the
    reference's projection of it is the source image: x, y, z, reflectance bit-exact, the mask equal, depth within 1e-6 relative
    (the reference recomputes it as the fp32 norm of coordinates that carry a rounding each: about 8 ulp)."""
    src = golden_file[f"src_{name}"]
    assert np.array_equal(bits(src), bits(G.source_planes(G.H, G.W, G.CASES[name]))), "the generator's images are the stored ones"
    row_start = pointcloud.scan_row_start(pointcloud.centred_ray_angles(G.H, G.W))
    pts, off, idx = PO.export(src[None], row_start, "scan", G.MIN_DEPTH, G.MAX_DEPTH)
    assert np.array_equal(bits(pts), bits(golden_file[f"pts_{name}"])) and off.tolist() == [0, len(pts)]
    valid = G.valid_mask(G.H, G.W, G.CASES[name])
    assert len(pts) == valid.sum() and np.array_equal(np.sort(idx), np.flatnonzero(valid))
    ref = golden_file[f"{mode}_{name}"]  # (6,H,W) [x, y, z, reflectance, depth, mask]
    assert np.array_equal(bits(ref[:4]), bits(src[[1, 2, 3, 4]]))
    assert np.array_equal(ref[5] == 1, valid) and set(np.unique(ref[5])) <= {0.0, 1.0}
    rel = np.abs(ref[4].astype(np.float64) - src[0])[valid] / src[0][valid]
    print(f"{name} {mode}: depth off by at most {rel.max():.3e} relative")
    assert rel.max() <= 1e-6 and not ref[4][~valid].any()


def test_image_order_export_does_not_survive_scan_unfolding(golden_file):
    """The order matters: the same points written row-major get other rows from the closed form of the reference's loop."""
    sys.path.insert(0, GOLDEN)
    import make_golden_projection as GP

    src = golden_file["src_dense"]
    rs = pointcloud.scan_row_start(pointcloud.centred_ray_angles(G.H, G.W))
    scan, _, scan_idx = PO.export(src[None], rs, "scan", G.MIN_DEPTH, G.MAX_DEPTH)
    image, _, image_idx = PO.export(src[None], None, "image", G.MIN_DEPTH, G.MAX_DEPTH)
    assert np.array_equal(image_idx, np.arange(G.H * G.W)) and np.array_equal(np.sort(scan_idx), image_idx)
    assert np.array_equal(GP.unfolding_rows(scan, G.H), scan_idx // G.W)
    assert (GP.unfolding_rows(image, G.H) != image_idx // G.W).any()


def test_oracle_positions():
    assert PO.positions(2, 4, None, "image").tolist() == list(range(8))
    assert PO.positions(2, 4, [1, 3], "scan").tolist() == [1, 0, 3, 2, 7, 6, 5, 4]
    planes = np.zeros((2, 5, 2, 4), np.float32)
    planes[0, 0] = [[2, 0, 3, np.nan], [100, 5, 1.45, 80]]
    planes[0, 1:4] = 1
    planes[0, 2, 0, 2] = np.inf     # depth 3: y not finite
    planes[0, 4] = np.arange(8).reshape(2, 4)
    pts, off, idx = PO.export(planes, [1, 3], "scan")
    assert off.tolist() == [0, 2, 2] and idx.tolist() == [0, 5] and pts[:, 3].tolist() == [0, 5] and idx.dtype == np.int32
    pts, off, idx = PO.export(planes, None, "image", 0.0, np.inf)
    assert idx.tolist() == [0, 4, 5, 6, 7] and off.tolist() == [0, 5, 5]


# ---- host helpers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("H, W", [(8, 64), (5, 104), (64, 1024), (64, 2048)])
def test_scan_row_start_on_the_edge_and_centred_grids(H, W):
    edge, centred = pointcloud.scan_row_start(hdl64e_ray_angles(H, W)), pointcloud.scan_row_start(pointcloud.centred_ray_angles(H, W))
    assert edge.dtype == centred.dtype == np.int32 and edge.shape == centred.shape == (H,)
    assert (edge == W // 2).all() and (centred == W // 2 - 1).all()
    assert np.array_equal(pointcloud.scan_row_start(pointcloud.centred_ray_angles(H, W)[0]), centred)  # (2,H,W) too


def test_scan_row_start_rule():
    az = torch.tensor([[3.0, 2.0, 0.0, -1.0], [-1.0, -2.0, -3.0, -0.5], [1.0, -1.0, 2.0, -2.0], [0.5, 0.5, 0.5, 0.5]])
    ang = torch.stack([torch.zeros_like(az), az])
    assert pointcloud.scan_row_start(ang).tolist() == [2, 3, 2, 3]
    with pytest.raises(ValueError, match="ray_angles"):
        pointcloud.scan_row_start(torch.zeros(3, 4, 4))


def test_centred_ray_angles():
    a = pointcloud.centred_ray_angles(64, 1024)
    assert a.shape == (1, 2, 64, 1024) and a.dtype == torch.float32
    edge = hdl64e_ray_angles(64, 1024)
    # half a cell below / right of the edge grid
    assert torch.allclose(a[0, 0], edge[0, 0] - np.deg2rad(28.0 / 64 / 2), atol=1e-6)
    assert torch.allclose(a[0, 1], edge[0, 1] - np.deg2rad(360.0 / 1024 / 2), atol=1e-6)
    # symmetric in the azimuth: no ray on 0 or on +-180 degrees
    assert torch.allclose(a[0, 1], -a[0, 1].flip(-1), atol=1e-6) and a[0, 1].abs().min() > 1e-3


def test_save_scans_then_load_scans_is_the_identity(tmp_path):
    g = np.random.Generator(np.random.PCG64(3))
    pts = g.standard_normal((1000, 4)).astype(np.float32)
    pts[5, 3], pts[6, 0] = np.nan, -0.0
    off = np.array([0, 300, 300, 999, 1000], np.int64)
    paths = [tmp_path / f"{k}.bin" for k in range(4)]
    pointcloud.save_scans(pts, off, paths)
    got, got_off = projection.load_scans(paths)
    assert np.array_equal(bits(got), bits(pts)) and np.array_equal(got_off, off) and paths[1].stat().st_size == 0
    pointcloud.save_scans(torch.from_numpy(pts), torch.from_numpy(off), paths)  # tensors too
    assert np.array_equal(bits(projection.load_scans(paths)[0]), bits(pts))
    with pytest.raises(ValueError, match="paths"):
        pointcloud.save_scans(pts, off, paths[:3])
    with pytest.raises(ValueError, match="offsets"):
        pointcloud.save_scans(pts, off[:-1], paths[:3])
    with pytest.raises(ValueError, match=r"\(total,4\)"):
        pointcloud.save_scans(pts[:, :3], off, paths)


@pytest.mark.parametrize("coloured", [False, True])
def test_save_ply(tmp_path, coloured):
    g = np.random.Generator(np.random.PCG64(4))
    pts = g.standard_normal((37, 4)).astype(np.float32)
    colors = g.integers(0, 256, size=(37, 3)).astype(np.uint8) if coloured else None
    path = tmp_path / "cloud.ply"
    pointcloud.save_ply(torch.from_numpy(pts), path, colors)
    data = path.read_bytes()
    head, payload = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 37"]
    want = ["property float x", "property float y", "property float z", "property float intensity"]
    want += ["property uchar red", "property uchar green", "property uchar blue"] if coloured else []
    assert lines[3:] == want
    stride = 19 if coloured else 16
    assert len(payload) == 37 * stride
    rows = np.frombuffer(payload, np.uint8).reshape(37, stride)
    assert np.array_equal(rows[:, :16].copy().view("<f4"), pts)
    if coloured:
        assert np.array_equal(rows[:, 16:], colors)
        with pytest.raises(ValueError, match="colors"):
            pointcloud.save_ply(pts, path, colors[:-1])
        with pytest.raises(ValueError, match="colors"):
            pointcloud.save_ply(pts, path, colors.astype(np.float32))
    pointcloud.save_ply(np.zeros((0, 4), np.float32), path)
    assert path.read_bytes().endswith(b"element vertex 0\nproperty float x\nproperty float y\nproperty float z\nproperty float intensity\nend_header\n")


# ---- arguments ---------------------------------------------------------------------------------------
def test_images_to_points_refuses_bad_arguments_before_touching_the_gpu():
    lidar = r2dm_amd.LiDARUtility((8, 64), "log_depth", 1.45, 80.0)
    x, s = torch.zeros(2, 2, 8, 64), torch.zeros(2, 5, 8, 64)
    with pytest.raises(ValueError, match="layout"):
        pointcloud.images_to_points(x, lidar, layout="xyz")
    with pytest.raises(ValueError, match="order"):
        pointcloud.images_to_points(x, lidar, order="ring")
    with pytest.raises(ValueError, match=r"\(B,2,H,W\)"):
        pointcloud.images_to_points(s, lidar)
    with pytest.raises(ValueError, match=r"\(B,5,H,W\)"):
        pointcloud.images_to_points(x, lidar, layout="sample")
    with pytest.raises(ValueError, match=r"\(B,2,H,W\)"):
        pointcloud.images_to_points(x[0], lidar)
    with pytest.raises(ValueError, match="lidar_utils"):
        pointcloud.images_to_points(x)
    with pytest.raises(ValueError, match="azimuths"):
        pointcloud.images_to_points(s, layout="sample", order="scan")
    with pytest.raises(ValueError, match="ray_angles"):
        pointcloud.images_to_points(x, lidar, ray_angles=pointcloud.centred_ray_angles(8, 32))
    with pytest.raises(ValueError, match="ray_angles"):
        pointcloud.images_to_points(torch.zeros(2, 2, 16, 64), lidar)
    # no CPU fallback: a CPU tensor is refused, and so is a numpy batch where there is no device
    for kw in (dict(), dict(order="image"), dict(return_index=True)):
        with pytest.raises(_lib.R2DMError, match="no CPU fallback"):
            pointcloud.images_to_points(x, lidar, **kw)
    with pytest.raises(_lib.R2DMError, match="no CPU fallback"):
        pointcloud.images_to_points(s, layout="sample", order="image")
    if not torch.cuda.is_available():
        with pytest.raises(_lib.R2DMError, match="no CPU fallback"):
            pointcloud.images_to_points(x.numpy(), lidar)


def test_c_abi_refuses_bad_arguments_with_a_status():
    """Argument errors come back as a status and a message (no launch, no fault): checked before any device call."""
    L = _lib.lib()
    fake = 1 << 20  # stands for device memory: never dereferenced by a refused call

    def call(src=fake, layout=0, ang=fake, row_start=None, points=fake, index=None, offsets=fake, batch=2, H=8, W=64, fmt=0, scratch=fake,
             scratch_bytes=1 << 30):
        rc = L.r2dm_unproject(src, layout, ang, row_start, points, index, offsets, batch, H, W, 1.45, 80.0, fmt, 1.45, 80.0, scratch, scratch_bytes, None)
        return rc, L.r2dm_last_error().decode()

    for kw, msg in [(dict(src=None), "null"), (dict(points=None), "null"), (dict(offsets=None), "null"), (dict(scratch=None), "null"),
                    (dict(ang=None), "null"), (dict(layout=2), "layout"), (dict(layout=-1), "layout"), (dict(fmt=3), "depth_format"),
                    (dict(batch=0), "batch"), (dict(batch=65536), "batch"), (dict(H=0), "pixels"), (dict(W=-1), "pixels"),
                    (dict(H=1 << 15, W=1 << 15), "pixels"), (dict(batch=2, H=1 << 15, W=1 << 15), "pixels"),
                    (dict(points=fake + 4), "aligned"), (dict(offsets=fake + 4), "aligned"), (dict(scratch=fake + 64), "aligned"),
                    (dict(scratch_bytes=16), "scratch too small")]:
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
    assert L.r2dm_unproject_scratch_bytes(2, 64, 1024) >= (2 * 256 + 1) * 4
    assert L.r2dm_unproject_scratch_bytes(3, 5, 104) >= (3 * 3 + 1) * 4
    for bad in [(0, 64, 1024), (65536, 64, 1024), (2, 0, 1024), (2, 64, -3), (1, 1 << 15, 1 << 16), (65535, 1 << 8, 1 << 8)]:
        assert L.r2dm_unproject_scratch_bytes(*bad) == 0, bad
    assert L.r2dm_unproject_scratch_bytes(65535, 128, 255) > 0  # just inside 2^31 pixels


def test_package_exports():
    for name in ("images_to_points", "save_scans", "save_ply", "scan_row_start", "centred_ray_angles"):
        assert getattr(r2dm_amd, name) is getattr(pointcloud, name) and name in r2dm_amd.__all__


@pytest.mark.parametrize("script, options", [
    ("sample_and_save.py", ["--points_dir"]),
    ("generate.py", ["--points_dir", "--points_ply"]),
    ("completion_demo.py", ["--out_scan"]),
])
def test_script_options(script, options):
    r = subprocess.run([sys.executable, f"{ROOT}/{script}", "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for o in options:
        assert o in r.stdout, (script, o)
