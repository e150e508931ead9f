"""-m gpu: the FRD extractor and the segmentation on the GPU -- RangeNet-53 / -21 (r2dm_amd.rangenet, rangenet.hip) against the
reference's recorded fp64 outputs and the fp64 oracle (tests/golden/rangenet.npz, tests/golden/make_golden_rangenet.py,
tests/rangenet_oracle.py), determinism, batching, the mask, the error paths, evaluate.py and completion_demo.py."""
import json
import os
import struct
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN, GOLDEN_RES, ROOT, synthetic_ckpt

sys.path.insert(0, GOLDEN)
import make_golden_projection as GP  # noqa: E402  (a raw scan for the completion demo)
import make_golden_rangenet as G  # noqa: E402  (the fixture's integer-only input generators)
import rangenet_oracle as O  # noqa: E402

from r2dm_amd import metrics, rangenet, render, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

STORED = {c[0]: c for c in G.STORED_CASES}
REGEN = {c[0]: c for c in G.REGEN_CASES}


@pytest.fixture(scope="module")
def data():
    with np.load(os.path.join(GOLDEN, "rangenet.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def states():
    return {b: synthetic.synthetic_rangenet_state(G.STATE_SEED, b) for b in (53, 21)}


@pytest.fixture(scope="module")
def extractors(states):
    return {b: rangenet.RangeNetExtractor(sd, device="cuda") for b, sd in states.items()}


@pytest.fixture(scope="module")
def extractor(extractors):
    return extractors[53]


@pytest.fixture(scope="module")
def b2(data, extractor):
    """The (2,5,4,64) case on the device and its decoder map, computed once."""
    x = torch.from_numpy(data["x_b2"]).cuda()
    return x, extractor.extract(x, feature="decoder")


def _check(name, got, want64, err):
    """rms <= 2x and max <= 4x the reference's own error against fp64 on the same inputs (the ratios of tests/test_hip_configs.py)"""
    d = got.double().cpu() - want64.double().cpu()
    rms, mx = d.pow(2).mean().sqrt().item(), d.abs().max().item()
    print(f"{name}: |hip - fp64| rms {rms:.3e} max {mx:.3e}; reference's own rms {err[0]:.3e} max {err[1]:.3e} "
          f"(ratios {rms / err[0]:.2f}, {mx / err[1]:.2f})")
    assert got.dtype == torch.float32 and got.is_cuda and torch.isfinite(got).all()
    assert rms <= 2 * err[0] and mx <= 4 * err[1]


def _check_labels(name, labels, log64, err_log):
    """equal to the fp64 argmax wherever the fp64 top-two margin exceeds 8x the reference's max logit error; those are >= 99 %"""
    log64 = log64.double().cpu()
    top2 = log64.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > G.MARGIN * err_log[1]
    left_out = 1 - sure.double().mean().item()
    print(f"{name}: {left_out:.3%} of the pixels within the label margin")
    assert labels.dtype == torch.int64 and labels.shape == (log64.shape[0], 1, *log64.shape[2:])
    assert left_out <= G.MAX_EXCLUDED
    assert torch.equal(labels.cpu()[:, 0][sure], log64.argmax(1)[sure])


def _all_outputs(name, e, x, dec64, log64, data):
    dec, logits = e.extract(x, feature="decoder"), e.extract(x, feature=None)
    B, _, H, W = x.shape
    assert dec.shape == (B, 32, H, W) and logits.shape == (B, 20, H, W)
    _check(f"{name} decoder", dec, dec64, data[f"err_dec_{name}"])
    _check(f"{name} logits", logits, log64, data[f"err_log_{name}"])
    labels = e.segment(x)
    _check_labels(name, labels, log64, data[f"err_log_{name}"])
    assert torch.equal(labels[:, 0], logits.argmax(1))  # (the device argmax: the lowest index on a tie, as torch's)
    return dec


@pytest.mark.parametrize("name", list(STORED))
def test_outputs_against_the_references_fp64(data, extractor, name):
    x = torch.from_numpy(data[f"x_{name}"]).cuda()
    dec = _all_outputs(name, extractor, x, torch.from_numpy(data[f"dec64_{name}"]), torch.from_numpy(data[f"log64_{name}"]), data)
    H, W = x.shape[2:]
    if 32 * H * W >= 4096:  # "lidargen": the decoder map at the reference's indices, bit for bit
        import random

        random.seed(0)
        idx = torch.tensor(random.sample(range(32 * H * W), 4096), device="cuda")
        feats = extractor.extract(x, feature="lidargen")
        assert feats.shape == (x.shape[0], 4096) and torch.equal(feats, dec.flatten(1)[:, idx])
        assert torch.equal(extractor(x), feats)  # the callable is the same path; the same bits on a second call


def _oracle64(states, backbone, x):
    """the fp64 oracle, torch ops on the device"""
    return O.forward(O.cast(states[backbone], torch.float64, "cuda"), O.preprocess(x.double()), backbone)


def test_backbone_21(data, states, extractors):
    name, seed, shape, backbone = REGEN["bb21"]
    x = torch.from_numpy(G.images(seed, shape)).cuda()
    assert extractors[21].backbone == 21
    _all_outputs(name, extractors[21], x, *_oracle64(states, 21, x), data)


def test_full_size_image(data, states, extractor):
    name, seed, shape, backbone = REGEN["full"]
    x = torch.from_numpy(G.images(seed, shape)).cuda()
    dec = _all_outputs(name, extractor, x, *_oracle64(states, 53, x), data)
    idx = torch.from_numpy(data["indices"].astype(np.int64)).cuda()
    assert torch.equal(extractor.extract(x, feature="lidargen"), dec.flatten(1)[:, idx])


def test_determinism_and_batching(states, b2):
    x2, _ = b2
    x = torch.cat([x2, torch.from_numpy(G.images(61, (1, 5, 4, 64))).cuda()])
    e = rangenet.RangeNetExtractor(states[53], device="cuda")
    for feature in ("decoder", None):
        got = e.extract(x, feature=feature)
        assert torch.equal(e.extract(x, feature=feature), got)  # a second call: the same bits
        for k in range(3):  # a row does not depend on the rest of the batch
            assert torch.equal(e.extract(x[k:k + 1], feature=feature), got[k:k + 1]), (feature, k)
    want = e.extract(x, feature="lidargen")
    e.max_batch = 2  # one image more than a pass takes
    assert torch.equal(e.extract(x, feature="lidargen"), want)
    assert torch.equal(e.segment(x), e.extract(x, feature=None).argmax(1, keepdim=True))


def test_mask(extractor, b2):
    x, dec = b2
    mask = torch.logical_and(x[:, [0]] > 0.5, x[:, [0]] < 63.0).float()
    assert 0.1 < mask.mean().item() < 0.9
    assert torch.equal(extractor.extract(x, mask, feature="decoder"), dec)  # the default mask is evaluate.py's depth window
    y = x.clone()  # the raw values of a masked pixel take no part, whatever they are
    off = (mask == 0).expand_as(y)
    y[off] = y[off] * -3.0 + 1000.0
    y[:, 1][mask[:, 0] == 0] = float("nan")
    assert torch.equal(extractor.extract(y, mask, feature="decoder"), dec)
    # another mask is another result, and the depth window given as numbers is the same as the mask given as a tensor
    wide = (x[:, [0]] > 0.25).float()
    got = extractor.extract(x, wide, feature="decoder")
    assert not torch.equal(got, dec)
    assert torch.equal(extractor.extract(x, feature="decoder", image_min_depth=0.25, image_max_depth=1e9), got)
    want, _ = O.forward(O.cast(extractor_state(extractor), torch.float64, "cuda"), O.preprocess(x.double(), wide.double()), 53)
    assert (got.double() - want).abs().max().item() < 1e-4 * want.abs().max().item()


_STATE = {}


def extractor_state(e):
    if e.backbone not in _STATE:
        _STATE[e.backbone] = synthetic.synthetic_rangenet_state(G.STATE_SEED, e.backbone)
    return _STATE[e.backbone]


def test_shapes_and_error_paths(states, extractor, b2):
    x, dec = b2
    for feature, shape in (("lidargen", (0, 4096)), ("decoder", (0, 32, 4, 64)), (None, (0, 20, 4, 64))):
        assert extractor.extract(x[:0], feature=feature).shape == shape
    assert extractor.segment(x[:0]).shape == (0, 1, 4, 64) and extractor.segment(x[:0]).dtype == torch.int64
    with pytest.raises(ValueError, match="multiple of 32"):
        extractor.extract(torch.zeros(1, 5, 4, 48, device="cuda"))
    with pytest.raises(ValueError, match="4096"):
        extractor.extract(torch.zeros(1, 5, 2, 32, device="cuda"), feature="lidargen")
    with pytest.raises(ValueError, match=r"expected \(B,5,H,W\)"):
        extractor.extract(torch.zeros(1, 4, 4, 64, device="cuda"))
    with pytest.raises(ValueError, match="mask"):
        extractor.extract(x, torch.ones(2, 4, 64, device="cuda"))
    with pytest.raises(ValueError, match="feature"):
        extractor.extract(x, feature="encoder")
    with pytest.raises(Exception, match="no CPU fallback"):
        extractor.extract(x.cpu())
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="extractor on"):
            extractor.extract(x.to("cuda:1"))
    seen = torch.logical_and(x[:, 0] > 0.5, x[:, 0] < 63.0).nonzero()[5]
    for bad in (float("inf"), float("-inf"), float("nan")):
        y = x.clone()
        y[seen[0], 2, seen[1], seen[2]] = bad
        with pytest.raises(ValueError, match="non-finite"):
            extractor.extract(y, feature="decoder")
    assert torch.equal(extractor.extract(x, feature="decoder"), dec)  # the flag does not stick
    big = dict(states[53])
    big["stem.0.weight"] = states[53]["stem.0.weight"] * 1e6
    with pytest.raises(RuntimeError, match="fp16 operand range"):
        rangenet.RangeNetExtractor(big, device="cuda").extract(x, feature="decoder")
    nan = dict(states[53])
    nan["enc5.conv.0.weight"] = states[53]["enc5.conv.0.weight"].clone()
    nan["enc5.conv.0.weight"][5, 7, 0, 1] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        rangenet.RangeNetExtractor(nan, device="cuda")


def test_label_colours_on_the_device(data):
    labels = torch.arange(20, device="cuda").view(1, 1, 4, 5)
    got = render.colorize_labels(labels)
    assert got.dtype == torch.uint8 and got.shape == (1, 3, 4, 5)
    assert np.array_equal(got[0].flatten(1).T.cpu().numpy(), data["label_colors"])


# ---- evaluate.py -------------------------------------------------------------------------------
def test_evaluate_writes_the_frd(tmp_path, states, extractor, monkeypatch):
    sys.path.insert(0, ROOT)
    import copy
    import hashlib

    import evaluate
    from r2dm_amd import pointnet

    # The Frechet distance of two 4096-dimensional feature sets is a 4096 x 4096 matrix square root on the host, some 20 s: every
    # pair of feature sets -- identified by its bits -- goes through the real function once, and the runs below share the result.
    frechet, seen = metrics.compute_frechet_distance, {}

    def frechet_once(a, b):
        key = tuple(hashlib.sha1(torch.as_tensor(t).cpu().numpy().tobytes()).hexdigest() for t in (a, b))
        if key not in seen:
            seen[key] = frechet(a, b)
        return seen[key]

    monkeypatch.setattr(metrics, "compute_frechet_distance", frechet_once)

    H, W = GOLDEN_RES
    assert W % 32 == 0 and 32 * H * W >= 4096
    ckpt, weights, pn_weights = tmp_path / "synthetic.pth", tmp_path / "rangenet.pth", tmp_path / "cls_model.pth"
    torch.save(synthetic_ckpt(resolution=GOLDEN_RES), ckpt)
    torch.save(states[53], weights)
    pn_state = synthetic.synthetic_pointnet_state(0)
    torch.save(pn_state, pn_weights)
    gen, real = tmp_path / "gen", tmp_path / "real"
    imgs = torch.from_numpy(G.images(71, (13, 5, H, W)))
    for out, part in ((gen, imgs[:6]), (real, imgs[6:])):
        out.mkdir()
        for i, img in enumerate(part):
            torch.save(img.clone(), out / f"samples_{i:04d}.pth")
    args = Namespace(ckpt=ckpt, sample_dir=str(gen), dataset="test", batch_size=4, num_workers=0, real_set=None, real_dir=str(real),
                     real_scans=None, pointnet_weights=None, rangenet_weights=str(weights), mmd_seed=7)
    r = json.loads(open(evaluate.evaluate(args)).read())
    f_gen, f_real = extractor.extract(imgs[:6].cuda()), extractor.extract(imgs[6:].cuda())
    assert set(r["img"]) == {"frechet_distance", "squared_mmd"} and r["pts"] == {}
    assert r["info"]["#real"] == 7 and r["info"]["#fake"] == 6
    assert r["info"]["note"] == "pts (FPD) is not computed: it needs the PointNet weights"
    assert r["img"]["frechet_distance"] == metrics.compute_frechet_distance(f_real, f_gen)
    assert r["img"]["squared_mmd"] == metrics.compute_squared_mmd(f_real, f_gen, rng=np.random.RandomState(7))
    assert np.isfinite(r["img"]["frechet_distance"]) and np.isfinite(r["img"]["squared_mmd"])
    assert len(seen) == 1  # (evaluate.py's features are, bit for bit, the extractor's)
    # both weight files: all four groups, no note
    args.pointnet_weights, args.sample_dir = str(pn_weights), str(gen) + "_both"
    os.rename(gen, args.sample_dir)
    both = json.loads(open(evaluate.evaluate(args)).read())
    assert both["img"] == r["img"] and both["bev"] == r["bev"] and "note" not in both["info"]
    pn = pointnet.pretrained_pointnet(pn_state, device="cuda")
    p_gen, p_real = pointnet.pointnet_features(pn, imgs[:6].cuda()), pointnet.pointnet_features(pn, imgs[6:].cuda())
    assert both["pts"] == {"frechet_distance": metrics.compute_frechet_distance(p_real, p_gen),
                           "squared_mmd": metrics.compute_squared_mmd(p_real, p_gen, rng=np.random.RandomState(7))}
    # without the option (a Namespace that does not even have it): exactly as before
    old = Namespace(**{k: v for k, v in vars(args).items() if k != "rangenet_weights"})
    old.pointnet_weights, old.sample_dir = None, str(gen) + "_again"
    os.rename(args.sample_dir, old.sample_dir)
    q = json.loads(open(evaluate.evaluate(old)).read())
    assert q["pts"] == {} and q["img"] == {} and q["bev"] == r["bev"]
    assert q["info"]["note"] == "img (FRD) and pts (FPD) are not computed: they need the RangeNet-53 and PointNet weights"
    old.pointnet_weights, old.sample_dir = str(pn_weights), str(gen) + "_pts"
    os.rename(str(gen) + "_again", old.sample_dir)
    q = json.loads(open(evaluate.evaluate(old)).read())
    assert q["pts"] == both["pts"] and q["img"] == {} and q["info"]["note"] == "img (FRD) is not computed: it needs the RangeNet-53 weights"
    # a checkpoint trained without reflectance: no FRD, as in the reference, and the note says why
    plain = copy.deepcopy(synthetic_ckpt(resolution=GOLDEN_RES)["cfg"])
    plain["data"]["train_reflectance"] = False
    torch.save({"cfg": plain}, tmp_path / "plain.pth")
    args.ckpt, args.pointnet_weights, args.sample_dir = tmp_path / "plain.pth", None, str(gen) + "_plain"
    os.rename(old.sample_dir, args.sample_dir)
    q = json.loads(open(evaluate.evaluate(args)).read())
    assert q["img"] == {} and q["pts"] == {} and q["bev"] == r["bev"]
    assert q["info"]["note"].startswith("img (FRD) is not computed: the checkpoint was trained without reflectance")


# ---- completion_demo.py ------------------------------------------------------------------------
def test_completion_demo_segments(tmp_path, states, extractor):
    import r2dm_amd

    H, W = GOLDEN_RES
    ckpt, weights, scan = tmp_path / "synthetic.pth", tmp_path / "rangenet.pth", tmp_path / "scan.bin"
    torch.save(synthetic_ckpt(resolution=GOLDEN_RES), ckpt)
    torch.save(states[53], weights)
    GP.make_cloud("free_64x1024").tofile(scan)
    out = tmp_path / "demo" / "completion.png"
    r = subprocess.run([sys.executable, f"{ROOT}/completion_demo.py", "--ckpt", str(ckpt), "--scan", str(scan), "--out", str(out),
                        "--num_steps", "2", "--num_resample_steps", "2", "--jump_length", "1", "--seed", "3", "--rangenet_weights", str(weights)],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    data = out.read_bytes()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR"
    width, height = struct.unpack(">II", data[16:24])
    assert (width, height) == (4 * (W + 2) + 2, 4 * H + 2 * W + H + 4)  # the rows of test_completion_demo and the label row's H
    state = torch.load(out.parent / "completion.pt")
    assert set(state) == {"x_in", "mask", "x_out", "labels"}
    _, lidar, _ = r2dm_amd.setup_model(str(ckpt), device="cuda", show_info=False, max_batch=4)
    sys.path.insert(0, ROOT)
    import completion_demo

    samples, mask = completion_demo.semseg_inputs(state["x_out"].cuda(), lidar)
    assert samples.shape == (4, 5, H, W) and mask.shape == (4, 1, H, W)
    labels = extractor.segment(samples, mask)
    assert state["labels"].dtype == torch.int64 and torch.equal(state["labels"], labels.cpu())
    assert 0 <= int(labels.min()) and int(labels.max()) <= 19
