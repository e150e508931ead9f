"""-m gpu: the surface-normal kernels (r2dm_amd/csrc/render.hip) against the fp32 restatement of tests/normals_oracle.py, bit for bit on
every pixel, and the fused view of the training monitor against the fp64 evaluation of tests/render_oracle.py by the bars of
tests/test_hip_render.py; log_images; generate.py --render_normals end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import normals_oracle as O
from conftest import GOLDEN, GOLDEN_RES, ROOT, synthetic_ckpt
from test_hip_render import _check_bev, _png_size  # (the bars of render_point_clouds, and the PNG reader)

sys.path.insert(0, GOLDEN)
import make_golden_normals as G  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {c[0]: c for c in G.CASES}
SMALL = [c[0] for c in G.CASES if c[4]]
CONFIGS = [(name, mode, d) for name in CASES for mode in G.MODES for d in G.DS]


def bits(t):
    return t.contiguous().view(torch.int32)


def _lidar(res):
    from r2dm_amd.lidar import LiDARUtility

    return LiDARUtility(res, "log_depth", G.MIN_DEPTH, G.MAX_DEPTH)


@pytest.fixture(scope="module")
def inputs(golden):
    """name -> (depth (B,1,H,W), trig (4,H,W), xyz (B,3,H,W)) on the CPU; the 64 x 1024 case from the integer draws."""
    cache = {}

    def get(name):
        if name not in cache:
            _, seed, shape, kind, stored = CASES[name]
            g = golden("normals")
            if stored:
                cache[name] = tuple(g[f"{k}_{name}"] for k in ("depth", "trig", "xyz"))
            else:
                B, H, W = shape
                trig = torch.cat([g[f"trigrows_{name}"][:, :, None].expand(-1, -1, W), g[f"trigcols_{name}"][:, None, :].expand(-1, H, -1)]).contiguous()
                depth = torch.from_numpy(G.depth_scene(seed, shape, kind))
                cache[name] = (depth, trig, O.frame_xyz(depth, trig, G.MIN_DEPTH, G.MAX_DEPTH))
        return cache[name]

    return get


@pytest.fixture(scope="module")
def restated(inputs):
    """(name, mode, d) -> the fp32 restatement's normals on the CPU, computed once."""
    cache = {}

    def get(name, mode, d):
        if (name, mode, d) not in cache:
            cache[name, mode, d] = O.estimate_surface_normal(inputs(name)[2], d, mode)
        return cache[name, mode, d]

    return get


# ---- estimate_surface_normal ---------------------------------------------------------------------
@pytest.mark.parametrize("name,mode,d", CONFIGS, ids=["-".join(map(str, c)) for c in CONFIGS])
def test_normals_are_the_restatement_bit_for_bit(inputs, restated, name, mode, d):
    from r2dm_amd import render

    xyz = inputs(name)[2]
    got = render.estimate_surface_normal(xyz.cuda(), d, mode).cpu()
    want = restated(name, mode, d)
    differ = (bits(got) != bits(want)).any(1)
    print(f"{name} {mode} d {d}: {int(differ.sum())} of {differ.numel()} pixels differ in a bit")
    assert got.shape == want.shape and got.dtype == torch.float32
    assert not differ.any()
    if name == "zero":
        assert (got == 0).all()  # (exact zeros; their signs are the restatement's, whose masked points are +-0)


def test_ties_return_the_lowest_pairs_normal(inputs):
    """H = 1, W = 4, d = 2: the pairs 0, 2, 4 and 6 tie exactly; the pair 0's cross product 0 x V_2 and the pair 2's V_2 x 0 differ in the
    signs of their zeros."""
    from r2dm_amd import render

    xyz = inputs("tie")[2]
    V = O.neighbours(xyz, 2) - xyz
    n0, n2 = O.cross(V[0], V[2]) / 1e-8, O.cross(V[2], V[4]) / 1e-8
    assert not torch.equal(bits(n0), bits(n2)), "fixture: the tie cannot be told from the result"
    got = render.estimate_surface_normal(xyz.cuda(), 2, "closest").cpu()
    assert torch.equal(bits(got), bits(n0))


@pytest.mark.parametrize("name", ["flat", "full"])
def test_guard_elements_around_the_output_are_untouched(inputs, restated, name):
    from r2dm_amd import _lib

    xyz = inputs(name)[2].cuda()
    B, _, H, W = xyz.shape
    guard, n = 4096, xyz.numel()
    for mode, d in (("closest", 2), ("mean", 1)):
        buf = torch.full((n + 2 * guard,), -7.25, device="cuda")
        _lib.check(_lib.lib().r2dm_surface_normals(_lib.ptr(xyz), buf.data_ptr() + 4 * guard, B, H, W, d, G.MODES.index(mode), _lib.stream_ptr(xyz.device)))
        buf = buf.cpu()
        assert (buf[:guard] == -7.25).all() and (buf[-guard:] == -7.25).all()
        assert torch.equal(bits(buf[guard:-guard].view(B, 3, H, W)), bits(restated(name, mode, d)))


def test_batch_independence_and_determinism(inputs):
    from r2dm_amd import render

    small, other = inputs("small")[2].cuda(), inputs("zero")[2].cuda()
    for mode in G.MODES:
        a = render.estimate_surface_normal(small, 2, mode)
        assert torch.equal(bits(a), bits(render.estimate_surface_normal(small, 2, mode)))
        for k in range(small.shape[0]):
            assert torch.equal(bits(a[k:k + 1]), bits(render.estimate_surface_normal(small[k:k + 1], 2, mode)))
        mixed = torch.cat([small[1:], small[:1], small[1:]])  # (another batch size, another place in it)
        assert torch.equal(bits(render.estimate_surface_normal(mixed, 2, mode)[1:2]), bits(a[:1]))
    full = inputs("full")[2].cuda()
    assert torch.equal(bits(render.estimate_surface_normal(full)), bits(render.estimate_surface_normal(full)))
    assert other.shape[2:] != small.shape[2:]


@pytest.mark.parametrize("d", G.DS)
def test_non_finite_inputs_stay_inside_their_footprint(inputs, restated, d):
    """One +inf and one NaN (next to the azimuth seam and to the last rows): every pixel whose window holds neither keeps its bits."""
    from r2dm_amd import render

    xyz = inputs("full")[2].clone()
    _, _, H, W = xyz.shape
    planted = [(0, 10, 5, float("inf")), (2, H - 2, W - 1, float("nan"))]
    for c, h, w, v in planted:
        xyz[0, c, h, w] = v
    hh, ww = torch.arange(H)[:, None], torch.arange(W)[None, :]
    touched = torch.zeros(H, W, dtype=torch.bool)
    for _, h, w, _ in planted:
        dw = (ww - w).abs()
        touched |= ((hh - h).abs() <= d) & (torch.minimum(dw, W - dw) <= d)
    assert int(touched.sum()) == (2 * d + 1) ** 2 + (2 * d + 1) * (d + 2)
    for mode in G.MODES:
        got = render.estimate_surface_normal(xyz.cuda(), d, mode)
        torch.cuda.synchronize()
        same = (bits(got.cpu()) == bits(restated("full", mode, d))).all(1)[0]
        assert same[~touched].all(), (mode, int((~same & ~touched).sum()))


def test_bad_arguments_raise():
    from r2dm_amd import render

    x = torch.zeros(1, 3, 4, 6, device="cuda")
    for d in (0, 9, -1, 7):
        with pytest.raises(ValueError, match="neighbour distance"):
            render.estimate_surface_normal(x, d)
    with pytest.raises(NotImplementedError, match="median"):
        render.estimate_surface_normal(x, 2, "median")
    for bad in (torch.zeros(3, 4, 6), torch.zeros(1, 2, 4, 6), torch.zeros(1, 3, 0, 6), torch.zeros(1, 3, 4, 6, 1)):
        with pytest.raises(ValueError, match=r"\(B,3,H,W\)"):
            render.estimate_surface_normal(bad.cuda())
    assert render.estimate_surface_normal(x[:0]).shape == (0, 3, 4, 6)
    assert render.estimate_surface_normal(x, 6, "mean").shape == x.shape  # (d = W is the limit)
    lu = _lidar((4, 6))
    metric = torch.ones(1, 1, 4, 6, device="cuda")
    with pytest.raises(ValueError, match="neighbour distance"):
        render.render_normals(metric, lu, size=16, d=7)
    with pytest.raises(NotImplementedError, match="median"):
        render.render_normals(metric, lu, size=16, mode="median")
    with pytest.raises(ValueError, match="depths"):
        render.render_normals(metric[:, :, :3], lu, size=16)
    with pytest.raises(ValueError, match="trig"):
        render.render_normals(metric, lu, size=16, trig=torch.zeros(4, 4, 5, device="cuda"))
    with pytest.raises(ValueError, match="size"):
        render.render_normals(metric, lu, size=0)
    with pytest.raises(ValueError, match="channels"):
        render.log_images(torch.zeros(1, 2, 4, 6, device="cuda"), lu, channels=(1, 0))


# ---- render_normals ------------------------------------------------------------------------------
def _check_view(inputs, name, size, mode="closest", d=2):
    from r2dm_amd import render

    depth, trig, xyz = inputs(name)
    H, W = depth.shape[2:]
    lu = _lidar((H, W))
    colors, bev = render.render_normals(depth.cuda(), lu, size=size, d=d, mode=mode, trig=trig.cuda())
    c32 = O.normal_colors(O.estimate_surface_normal(xyz, d, mode))
    assert colors.shape == c32.shape and bev.shape == (depth.shape[0], 3, size, size)
    assert torch.equal(bits(colors.cpu()), bits(c32))
    # the truth: the fp64 projection and splat with the colours FIXED to the fp32 restatement's (a near-tie of the closest pair would
    # otherwise flip a colour between the precisions)
    _, o32 = O.render_normals(depth, trig, G.MIN_DEPTH, G.MAX_DEPTH, size, d, mode, colors=c32)
    _, o64, hit = O.render_normals(depth, trig, G.MIN_DEPTH, G.MAX_DEPTH, size, d, mode, dtype=torch.float64, colors=c32, return_hit=True)
    _check_bev(bev.cpu(), o32, o64, hit, f"render_normals {name} {mode} d {d}, size {size}")
    again = render.render_normals(depth.cuda(), lu, size=size, d=d, mode=mode, trig=trig.cuda())
    assert torch.equal(bits(bev), bits(again[1])) and torch.equal(bits(colors), bits(again[0]))
    none, only = render.render_normals(depth.cuda(), lu, size=size, d=d, mode=mode, trig=trig.cuda(), with_colors=False)
    assert none is None and torch.equal(bits(only), bits(bev))


@pytest.mark.parametrize("size", [64, 96])
@pytest.mark.parametrize("name", SMALL)
def test_render_normals_small(inputs, name, size):
    _check_view(inputs, name, size)
    if name == "small":
        _check_view(inputs, name, size, "mean", 1)


def test_render_normals_full_size(inputs):
    _check_view(inputs, "full", 800)


def test_render_normals_default_planes(inputs):
    """Without ``trig`` the planes are taken from the ray angles on the device: the same image up to the device's cos / sin."""
    from r2dm_amd import render

    depth, trig, _ = inputs("small")
    lu = _lidar(tuple(depth.shape[2:]))
    assert (render.ray_trig(lu, "cuda").cpu() - trig).abs().max() <= 2e-7
    c0, b0 = render.render_normals(depth.cuda(), lu, size=64)
    c1, b1 = render.render_normals(depth.cuda(), lu, size=64, trig=render.ray_trig(lu, "cuda"))
    assert torch.equal(bits(c0), bits(c1)) and torch.equal(bits(b0), bits(b1))


def test_render_normals_chunking():
    """Five frames through a scratch buffer of two == one frame at a time."""
    from r2dm_amd import render

    depth = torch.from_numpy(G.depth_scene(77, (5, *GOLDEN_RES))).cuda()
    lu = _lidar(GOLDEN_RES)
    colors, bev = render.render_normals(depth, lu, size=75, scratch_frames=2)
    for k in range(5):
        c1, b1 = render.render_normals(depth[k:k + 1], lu, size=75, scratch_frames=1)
        assert torch.equal(bits(colors[k:k + 1]), bits(c1)) and torch.equal(bits(bev[k:k + 1]), bits(b1)), k
    assert torch.equal(bits(bev), bits(render.render_normals(depth, lu, size=75)[1]))
    assert (bev != 0).any() and torch.isfinite(bev).all()


# ---- log_images ----------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [(1, 1), (1, 0), (0, 1)])
def test_log_images(channels):
    pytest.importorskip("matplotlib")
    from r2dm_amd import render

    H, W = GOLDEN_RES
    lu = _lidar(GOLDEN_RES)
    depth = lu.convert_depth(torch.from_numpy(G.depth_scene(78, (2, H, W))))
    refl = torch.from_numpy(np.random.Generator(np.random.PCG64(79)).integers(0, 256, size=(2, 1, H, W)) / 255).float()
    image = lu.normalize(torch.cat([depth, refl], 1)[:, [k for k in (0, 1) if channels[k]]]).cuda()
    out = render.log_images(image, lu, channels=channels, tag="sample", size=48)
    keys = (["sample/depth", "sample/depth/orig", "sample/bev"] if channels[0] else []) + (["sample/reflectance"] if channels[1] else []) \
        + (["sample/mask"] if channels[0] else [])
    assert list(out) == keys
    for k, v in out.items():
        assert v.dtype == torch.uint8 and v.is_cuda and v.shape == ((2, 3, 48, 48) if k.endswith("bev") else (2, 3, H, W)), k
    if channels[0]:
        d01 = lu.denormalize(image[:, :1])
        metric = lu.revert_depth(d01)
        _, bev = render.render_normals(metric, lu, size=48)
        assert torch.equal(out["sample/bev"], bev.mul(255).clamp(0, 255).byte()) and len(out["sample/bev"].unique()) > 8
        assert torch.equal(out["sample/depth"], render.colorize(d01)) and torch.equal(out["sample/depth/orig"], render.colorize(metric / G.MAX_DEPTH))
        mask = (metric > G.MIN_DEPTH) & (metric < G.MAX_DEPTH)
        assert torch.equal(out["sample/mask"], render.colorize(mask.float(), "binary_r")) and 0.05 < 1 - mask.float().mean().item() < 0.2
    if channels[1]:
        assert torch.equal(out["sample/reflectance"], render.colorize(lu.denormalize(image[:, -1:]), "plasma"))


# ---- generate.py ---------------------------------------------------------------------------------
def test_generate_renders_normal_pngs(tmp_path):
    pytest.importorskip("matplotlib")
    ckpt = tmp_path / "synthetic.pth"
    torch.save(synthetic_ckpt(resolution=GOLDEN_RES), ckpt)
    common = [sys.executable, "generate.py", "--ckpt", str(ckpt), "--batch_size", "2", "--sampling_steps", "3", "--seed", "0", "--bev_size", "64"]
    plain, normals = tmp_path / "plain", tmp_path / "normals"
    subprocess.run(common + ["--output", str(tmp_path / "plain.pt"), "--render_dir", str(plain)], cwd=ROOT, check=True, timeout=600)
    subprocess.run(common + ["--output", str(tmp_path / "normals.pt"), "--render_dir", str(normals), "--render_normals"], cwd=ROOT, check=True, timeout=600)
    today = ["samples_bev.png", "samples_img.png"]
    assert sorted(os.listdir(plain)) == today
    assert sorted(os.listdir(normals)) == sorted(today + ["samples_normal.png", "samples_bev_normal.png"])
    for name in today:
        assert (plain / name).read_bytes() == (normals / name).read_bytes(), name
    a, b = torch.load(tmp_path / "plain.pt"), torch.load(tmp_path / "normals.pt")
    assert torch.equal(a["frames"], b["frames"]) and torch.equal(a["points"], b["points"])
    H, W = GOLDEN_RES
    for name, shape in {"samples_normal.png": (2 * (H + 2) + 2, W + 4), "samples_bev_normal.png": (64 + 4, 2 * 66 + 2)}.items():
        got, raw = _png_size(normals / name)
        assert got == shape, (name, got)
        assert len(np.unique(raw)) > 8, name  # (not a constant image behind its border)
