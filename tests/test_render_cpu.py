"""CPU tests of the rendering's host side (r2dm_amd/render.py): the torch oracle against the reference's goldens, the view
matrices, the image grid, the PNG writer and the no-fallback rule."""
import math
import struct
import zlib

import numpy as np
import pytest
import torch

import render_oracle as O


def test_oracle_reproduces_the_reference_bit_for_bit(golden):
    """tests/render_oracle.py in fp32 on the CPU == utils/render.py (tests/golden/render.npz, make_golden_render.py)."""
    g = golden("render")
    for name in ("turbo", "viridis"):
        assert torch.equal(O.colorize(g["colorize_in"], g[f"lut_{name}"]), g[f"colorize_{name}"]), name
    assert torch.equal(O.colorize(g["colorize_in"][:, None], g["lut_turbo"]), g["colorize_turbo"])  # (B,1,H,W) as well
    shape = tuple(g["raster_out"].shape[2:])
    got = O.bilinear_rasterizer(g["raster_coords"], g["raster_values"], shape)
    assert torch.equal(got, g["raster_out"])
    # the fixture does what it is for: points outside add on border rows / columns, some weights fall under the threshold
    idx, terms = O.raster_terms(g["raster_coords"], g["raster_values"], shape)
    assert (got[..., 0, :] != 0).any() and (got[..., -1] != 0).any() and (terms == 0).all(-1).any() and (terms != 0).all(-1).any()
    for size in (64, 96):
        bev = O.render_point_clouds(g["cloud_points"], g["cloud_colors"], size, g["view_R"], g["view_t"])
        assert torch.equal(bev, g[f"cloud_bev{size}"]), size
    assert (g["cloud_points"] == 0).all(-1).float().mean() == 0.25


def test_make_Rt_against_the_closed_form(golden):
    from r2dm_amd.render import make_Rt

    for roll, pitch, yaw in ((0.0, math.pi / 3, math.pi / 4), (0.3, -1.1, 2.5), (-2.0, 0.0, 0.0), (0.0, 0.0, 0.0)):
        R, t = make_Rt(roll=roll, pitch=pitch, yaw=yaw, x=0.1, y=-0.2, z=0.8)
        assert R.shape == (1, 3, 3) and t.shape == (1, 3) and R.dtype == t.dtype == torch.float32
        assert np.abs(R[0].double().numpy() - O.rotation(roll, pitch, yaw)).max() < 1e-6
        assert torch.equal(t, torch.tensor([[0.1, -0.2, 0.8]]))
    R, t = make_Rt(pitch=math.pi / 3, yaw=math.pi / 4, z=0.8)  # generate.py's view: what the goldens were rendered through
    assert torch.equal(R, golden("render")["view_R"]) and torch.equal(t, golden("render")["view_t"])


def test_make_grid_geometry():
    from r2dm_amd.render import make_grid

    imgs = torch.arange(5, dtype=torch.float32)[:, None, None, None].expand(5, 3, 4, 6) + 1
    grid = make_grid(imgs, nrow=4)  # 2 rows of 4 cells, 2 pixels of border around every cell
    assert grid.shape == (3, 2 * (4 + 2) + 2, 4 * (6 + 2) + 2)
    for k in range(5):
        r, c = divmod(k, 4)
        assert (grid[:, 2 + r * 6:2 + r * 6 + 4, 2 + c * 8:2 + c * 8 + 6] == k + 1).all()
    assert grid.sum() == 3 * 4 * 6 * (1 + 2 + 3 + 4 + 5)  # everything else is pad_value 0
    col = make_grid(imgs, nrow=1, padding=1, pad_value=0.5)
    assert col.shape == (3, 5 * 5 + 1, 6 + 2) and (col[:, 0] == 0.5).all() and (col[:, :, 0] == 0.5).all() and (col[:, 1:5, 1:7] == 1).all()
    assert make_grid(imgs[:1], nrow=4).shape == (3, 4, 6)  # torchvision returns a single image without a border
    with pytest.raises(ValueError):
        make_grid(imgs[0], nrow=1)


def _decode_png(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        chunks.append((tag, body))
        pos += 12 + n
    assert [t for t, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    W, H, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT")), np.uint8).reshape(H, 1 + 3 * W)
    assert (raw[:, 0] == 0).all()  # filter type 0 on every row
    return raw[:, 1:].reshape(H, W, 3)


def test_save_png_round_trip(tmp_path):
    from r2dm_amd.render import save_png

    g = np.random.Generator(np.random.PCG64(5))
    u8 = torch.from_numpy(g.integers(0, 256, size=(3, 7, 13)).astype(np.uint8))
    save_png(u8, tmp_path / "u8.png")
    assert (_decode_png(tmp_path / "u8.png") == u8.permute(1, 2, 0).numpy()).all()
    f = torch.from_numpy(g.uniform(-0.1, 1.1, size=(3, 5, 9)).astype(np.float32))
    f[0, 0, :4] = torch.tensor([0.0, 1.0, 0.5 / 255, 127.5 / 255])
    save_png(f, tmp_path / "f.png")
    want = f.mul(255).add(0.5).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).numpy()
    got = _decode_png(tmp_path / "f.png")
    assert (got == want).all() and got[0, 0, 0] == 0 and got[0, 1, 0] == 255
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        assert (np.asarray(Image.open(tmp_path / "f.png").convert("RGB")) == want).all()
    with pytest.raises(ValueError):
        save_png(torch.zeros(1, 4, 4), tmp_path / "bad.png")


def test_render_refuses_cpu_tensors():
    from r2dm_amd import _lib, render
    from r2dm_amd.lidar import LiDARUtility

    lu = LiDARUtility((16, 128), "log_depth", 1.45, 80.0)
    lut = torch.zeros(256, 3)
    for call in (lambda: render.colorize(torch.zeros(1, 1, 4, 4), lut),
                 lambda: render.colorize(torch.zeros(1, 4, 4)),
                 lambda: render.bilinear_rasterizer(torch.zeros(1, 8, 2), torch.zeros(1, 8, 3), (4, 4)),
                 lambda: render.render_point_clouds(torch.zeros(1, 8, 3)),
                 lambda: render.render_point_clouds(torch.zeros(1, 8, 3), torch.zeros(1, 8, 3), size=16),
                 lambda: render.render_frames(torch.zeros(1, 2, 16, 128), lu, size=16)):
        with pytest.raises(_lib.R2DMError, match="no CPU fallback"):
            call()


def test_colormap_tables():
    from r2dm_amd import render

    t = torch.rand(256, 3)
    assert torch.equal(render.colormap_lut(t), t)
    ramp = lambda v: np.stack([v, v * 0, 1 - v, v * 0 + 1], 1)  # a callable, used the way the reference uses matplotlib's
    assert torch.equal(render.colormap_lut(ramp)[:, 0], torch.from_numpy(np.linspace(0, 1, 256)).float())
    with pytest.raises(ValueError):
        render.colormap_lut(torch.zeros(16, 3))
    with pytest.raises(TypeError):
        render.colormap_lut(3)


def test_named_colormaps_are_the_references(golden):
    pytest.importorskip("matplotlib")
    from r2dm_amd import render

    for name in ("turbo", "viridis"):
        assert torch.equal(render.colormap_lut(name), golden("render")[f"lut_{name}"]), name
    with pytest.raises(ValueError):
        render.colormap_lut("no_such_map")
