"""-m gpu: the kNN vote and the CRF-RNN on the GPU (r2dm_amd.postproc, postproc.hip) against the torch restatements
(tests/postproc_oracle.py) and the reference's recorded runs (tests/golden/postproc.npz, tests/golden/make_golden_postproc.py);
``RangeNetExtractor.segment(postprocess=...)``, the hub entries and completion_demo.py's ``--semseg_postprocess``."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, GOLDEN_RES, ROOT, synthetic_ckpt

sys.path.insert(0, GOLDEN)
import make_golden_postproc as G  # noqa: E402  (the fixture's integer-only input generators)
import make_golden_projection as GP  # noqa: E402  (a raw scan for the completion demo)
import make_golden_rangenet as GR  # noqa: E402
import postproc_oracle as O  # noqa: E402

from r2dm_amd import _lib, metrics, postproc, rangenet, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

KNN_CASES = {c[0]: c for c in G.KNN_CASES}
CRF_CASES = {c[0]: c for c in G.CRF_CASES}


@pytest.fixture(scope="module")
def data():
    with np.load(os.path.join(GOLDEN, "postproc.npz")) as z:
        return {k: z[k] for k in z.files}


_KNN = {}


def knn_case(name):
    """inputs (CPU), the fp32 oracle's labels, the fp64 truth and the sure pixels of a case, computed once"""
    if name not in _KNN:
        _, seed, shape, ks, k, cutoff, _, kind = KNN_CASES[name]
        depth, label = (torch.from_numpy(a) for a in G.knn_scene(seed, shape, kind))
        d32, d64 = O.knn_dist(depth, O.knn_weight(ks, 1.0, torch.float32)), O.knn_dist(depth, O.knn_weight(ks, 1.0, torch.float64))
        o32, o64 = (O.knn_vote(d, label, ks, k, cutoff, G.NUM_CLASSES) for d in (d32, d64))
        _KNN[name] = (depth, label, o32, o64, O.knn_sure(d64, d32, k, cutoff)[0])
    return _KNN[name]


def knn_module(name):
    _, _, _, ks, k, cutoff, _, _ = KNN_CASES[name]
    return postproc.KNN(G.NUM_CLASSES, k=k, kernel_size=ks, cutoff=cutoff)


# ---- kNN ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(KNN_CASES))
def test_knn_equals_the_fp32_oracle_on_every_pixel(data, name):
    depth, label, o32, o64, sure = knn_case(name)
    knn = knn_module(name)
    got = knn(depth.cuda(), label.cuda())
    assert got.dtype == torch.int64 and got.is_cuda and got.shape == label.shape
    same = (got.cpu() == o32).double().mean().item()
    print(f"{name}: equal to the fp32 oracle on {same:.4%} of the pixels; sure pixels {sure.double().mean().item():.3%}")
    assert torch.equal(got.cpu(), o32)  # no exclusions
    assert torch.equal(got.cpu()[sure], o64[sure]) and torch.equal(o64, torch.from_numpy(data[f"knn64_{name}"]).long())
    assert torch.equal(knn(depth.cuda(), label.cuda()), got)  # the same bits on a second call
    assert torch.equal(knn(depth.cuda(), label.cuda()[:, None]), got)  # (B,1,H,W) labels


def test_knn_guard_elements_and_the_c_entry():
    depth, label, o32, _, _ = knn_case("edge")
    B, H, W = label.shape
    n, guard = B * H * W, 64
    buf = torch.full((n + 2 * guard,), -7, dtype=torch.int64, device="cuda")
    d, l = depth.cuda(), label.cuda()
    w = postproc.KNN(20).dist_kernel.cuda()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    L = _lib.lib()
    call = lambda kh, kw, k, classes: L.r2dm_knn_vote(d.data_ptr(), l.data_ptr(), w.data_ptr(), buf.data_ptr() + 8 * guard, B, H, W, kh, kw, k, classes,
                                                      1.0, flag.data_ptr(), _lib.stream_ptr(d.device))
    assert call(3, 3, 3, 20) == 0
    assert torch.equal(buf[guard:guard + n].view(B, H, W).cpu(), o32) and int(flag.item()) == 0
    assert bool((buf[:guard] == -7).all()) and bool((buf[guard + n:] == -7).all())
    buf.fill_(-7)
    for bad in ((9, 3, 3, 20), (3, 4, 3, 20), (3, 3, 10, 20), (5, 5, 9, 20), (3, 3, 0, 20), (3, 3, 3, 33)):  # a status, and nothing is launched
        assert call(*bad) != 0, bad
        assert b"knn_vote" in L.r2dm_last_error()
    torch.cuda.synchronize()
    assert bool((buf == -7).all())


def test_knn_batches(data):
    depth, label, o32, _, _ = knn_case("edge")
    knn = knn_module("edge")
    d, l = depth.cuda(), label.cuda()
    for b in range(d.shape[0]):  # an image alone equals its slice of the batch
        assert torch.equal(knn(d[b:b + 1], l[b:b + 1]).cpu(), o32[b:b + 1])
    knn.max_batch = 2  # one image more than a launch takes
    assert torch.equal(knn(d, l).cpu(), o32)
    empty = knn(d[:0], l[:0])
    assert empty.shape == (0, *l.shape[1:]) and empty.dtype == torch.int64


def test_knn_label_out_of_range_and_nan_depth():
    depth, label, o32, _, _ = knn_case("edge")
    knn = knn_module("edge")
    d, l = depth.cuda(), label.cuda()
    for bad in (G.NUM_CLASSES, -1, 2**40):
        m = l.clone()
        m[1, 3, 17] = bad
        with pytest.raises(ValueError, match="label is outside"):
            knn(d, m)
    assert torch.equal(knn(d, l).cpu(), o32)  # the call returned, and the flag does not stick
    invalid = d < 0
    assert 0.005 < invalid.double().mean().item() < 0.05
    for bad in (float("nan"), float("inf"), float("-inf")):  # a depth that is not finite is the invalid marker
        e = d.clone()
        e[invalid] = bad
        assert torch.equal(knn(e, l).cpu(), o32), bad
    assert torch.equal(O.knn(torch.where(invalid, torch.full_like(d, float("nan")), d).cpu(), label, 3, 3, 1.0, 1.0, 20), o32)


# ---- CRF-RNN -----------------------------------------------------------------------------------
def crf_module(data, name):
    _, seed, shape, ks, iters, stored, params = CRF_CASES[name]
    N = shape[1]
    if params != "custom":
        return postproc.CRFRNN(N, kernel_size=ks, num_iters=iters, **G.crf_kwargs(params, N))
    state = {k[len("crfstate_custom_"):]: torch.from_numpy(v) for k, v in data.items() if k.startswith("crfstate_custom_")}
    crf = postproc.CRFRNN(N, kernel_size=ks, num_iters=iters).load_state_dict(state)  # a state saved by the reference, non-default everywhere
    back = crf.state_dict()
    assert list(back) == list(state) and all(torch.equal(back[k], state[k]) for k in state)
    return crf


@pytest.mark.parametrize("name", list(CRF_CASES))
def test_crf_against_the_references_fp64(data, name):
    """rms <= 2x and max <= 4x the reference's own fp32 error against its fp64 run on the same inputs; the argmax equals the fp64 argmax
    wherever the fp64 top-two margin exceeds 8x that max error, at least 99 % of the pixels."""
    _, seed, shape, ks, iters, stored, params = CRF_CASES[name]
    unary, xyz, mask = (torch.from_numpy(a).cuda() for a in G.crf_inputs(seed, shape))
    crf = crf_module(data, name)
    got = crf(unary, xyz, mask)
    if stored:
        q64 = torch.from_numpy(data[f"q64_{name}"])
    else:  # the fp64 oracle (equal to the reference's fp64 run to 1e-12: tests/test_postproc_cpu.py), torch ops on the device
        q64 = O.crf(unary, xyz, mask, crf.state_dict(), ks, iters, torch.float64).cpu()
    err = data[f"err_crf_{name}"]
    d = got.double().cpu() - q64
    rms, mx = d.pow(2).mean().sqrt().item(), d.abs().max().item()
    print(f"{name}: |hip - fp64| rms {rms:.3e} max {mx:.3e}; reference's own rms {err[0]:.3e} max {err[1]:.3e} "
          f"(ratios {rms / err[0]:.2f}, {mx / err[1]:.2f})")
    assert got.dtype == torch.float32 and got.is_cuda and got.shape == unary.shape and torch.isfinite(got).all()
    assert rms <= 2 * err[0] and mx <= 4 * err[1]
    top2 = q64.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > G.MARGIN * err[1]
    assert 1 - sure.double().mean().item() <= G.MAX_EXCLUDED
    assert torch.equal(got.argmax(1).cpu()[sure], q64.argmax(1)[sure])
    assert torch.equal(crf(unary, xyz, mask[:, None]), got)  # the same bits on a second call; a (B,1,H,W) mask


def test_crf_batches(data):
    _, seed, shape, ks, iters, _, _ = CRF_CASES["custom"]
    unary, xyz, mask = (torch.from_numpy(a).cuda() for a in G.crf_inputs(seed, shape))
    crf = crf_module(data, "custom")
    got = crf(unary, xyz, mask)
    for b in range(shape[0]):  # an image alone equals its slice of the batch
        assert torch.equal(crf(unary[b:b + 1], xyz[b:b + 1], mask[b:b + 1]), got[b:b + 1])
    crf.max_batch = 1
    assert torch.equal(crf(unary, xyz, mask), got)
    assert crf(unary[:0], xyz[:0], mask[:0]).shape == (0, *shape[1:])
    for iters in (0, 1, 2):  # no iteration: the unary; one and two: the buffers alternate differently
        crf.num_iters = iters
        want = O.crf(unary, xyz, mask, crf.state_dict(), ks, iters, torch.float64)
        assert (crf(unary, xyz, mask).double() - want).abs().max().item() <= 4 * data["err_crf_custom"][1]
    L = _lib.lib()
    out = torch.full_like(unary, -7.0)
    p = crf._params.cuda()
    for kh, kw, n in ((9, 3, 20), (3, 2, 20), (3, 5, 33)):  # a status, and nothing is launched
        assert L.r2dm_crf_iter(unary.data_ptr(), unary.data_ptr(), xyz.data_ptr(), mask.data_ptr(), p.data_ptr(), out.data_ptr(), shape[0], n,
                               shape[2], shape[3], kh, kw, 0, _lib.stream_ptr(unary.device)) != 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# ---- segment, the hub entries, completion_demo.py ----------------------------------------------
@pytest.fixture(scope="module")
def state():
    return synthetic.synthetic_rangenet_state(GR.STATE_SEED, 53)


@pytest.fixture(scope="module")
def rn_data():
    with np.load(os.path.join(GOLDEN, "rangenet.npz")) as z:
        return {k: z[k] for k in ("x_b2", "log64_b2", "err_log_b2")}


def test_segment_postprocess(state, rn_data):
    e = rangenet.RangeNetExtractor(state, device="cuda")
    x = torch.from_numpy(rn_data["x_b2"]).cuda()
    plain = e.segment(x)
    logits = e.extract(x, feature=None)
    assert torch.equal(e.segment(x, postprocess=None), plain) and torch.equal(plain[:, 0], logits.argmax(1))
    knn, crf = postproc.KNN(20), postproc.CRFRNN(20, theta_beta=0.5, init_weight_smoothness=0.2, init_weight_appearance=1.0)
    depth = x[:, [0]]
    m = torch.logical_and(depth > metrics.MIN_DEPTH, depth < metrics.MAX_DEPTH).float()
    q = crf(logits, x[:, 1:4] * m, m)
    invalid = torch.where(m != 0, depth, torch.full_like(depth, -1.0))
    assert torch.equal(e.segment(x, postprocess=crf), q.argmax(1, keepdim=True))
    assert torch.equal(e.segment(x, postprocess=knn), knn(invalid, plain)[:, None])
    both = e.segment(x, postprocess=(crf, knn))
    assert both.shape == plain.shape and both.dtype == torch.int64
    assert torch.equal(both, knn(invalid, q.argmax(1))[:, None])
    assert not torch.equal(both, plain)
    given = (depth > 0.25).float()  # a mask given as a tensor
    assert torch.equal(e.segment(x, given, postprocess=knn),
                       knn(torch.where(given != 0, depth, torch.full_like(depth, -1.0)), e.segment(x, given))[:, None])
    assert e.segment(x[:0], postprocess=(crf, knn)).shape == (0, 1, 4, 64)
    with pytest.raises(ValueError, match="before every KNN"):
        e.segment(x, postprocess=(knn, crf))


def test_hub_rangenet(tmp_path, monkeypatch):
    """``rangenet(path)`` on a synthetic archive (backbone 21: the smaller file): ``model(preprocess(x, mask))`` meets the extractor's bars"""
    sys.path.insert(0, ROOT)
    import hubconf
    import rangenet_oracle as RO

    name, seed, shape, backbone = {c[0]: c for c in GR.REGEN_CASES}["bb21"]
    with np.load(os.path.join(GOLDEN, "rangenet.npz")) as z:
        err = z[f"err_log_{name}"]
    sd = synthetic.synthetic_rangenet_state(GR.STATE_SEED, backbone)
    sensor = {"img_means": list(rangenet.DEFAULT_MEAN), "img_stds": list(rangenet.DEFAULT_STD)}  # (the statistics the recorded errors were made with)
    monkeypatch.setattr(GR, "ARCH_YAML", {**GR.ARCH_YAML, "dataset": {"sensor": sensor}})
    path = tmp_path / "darknet21.tar.gz"
    GR.write_archive(path, sd, layers=backbone)
    model, preprocess = hubconf.rangenet(str(path), device="cuda")
    x = torch.from_numpy(GR.images(seed, shape)).cuda()
    mask = torch.logical_and(x[:, [0]] > 0.5, x[:, [0]] < 63.0).float()
    pre = preprocess(x, mask)
    mean, std = (torch.tensor(v, device="cuda")[None, :, None, None] for v in (rangenet.DEFAULT_MEAN, rangenet.DEFAULT_STD))
    assert torch.equal(pre, (x - mean) / std * mask) and torch.equal(preprocess(x), (x - mean) / std * (x[:, [0]] > 0).float())
    logits = model(pre)
    want = RO.forward(RO.cast(sd, torch.float64, "cuda"), RO.preprocess(x.double()), backbone)[1]  # the fp64 oracle, torch ops on the device
    d = (logits.double() - want).cpu()
    rms, mx = d.pow(2).mean().sqrt().item(), d.abs().max().item()
    print(f"hub rangenet: |hip - fp64| rms {rms:.3e} max {mx:.3e}; reference's own rms {err[0]:.3e} max {err[1]:.3e}")
    B, _, H, W = shape
    assert logits.shape == (B, 20, H, W) and rms <= 2 * err[0] and mx <= 4 * err[1]
    assert model(pre, feature="decoder").shape == (B, 32, H, W) and model(pre, feature="lidargen").shape == (B, 4096)
    assert model.backbone == 21 and model.num_classes == 20


def test_completion_demo_postprocess(tmp_path, state):
    import r2dm_amd

    ckpt, weights, scan = tmp_path / "synthetic.pth", tmp_path / "rangenet.pth", tmp_path / "scan.bin"
    torch.save(synthetic_ckpt(resolution=GOLDEN_RES), ckpt)
    torch.save(state, weights)
    GP.make_cloud("free_64x1024").tofile(scan)
    sys.path.insert(0, ROOT)
    import completion_demo

    saved = {}
    try:  # (main switches the gradients off for the process)
        for tag, extra in (("flagless", []), ("none", ["--semseg_postprocess", "none"]), ("knn", ["--semseg_postprocess", "knn"])):
            out = tmp_path / tag / "completion.png"
            completion_demo.main(completion_demo.parser().parse_args(
                ["--ckpt", str(ckpt), "--scan", str(scan), "--out", str(out), "--num_steps", "2", "--num_resample_steps", "1", "--jump_length", "1",
                 "--seed", "3", "--rangenet_weights", str(weights), *extra]))
            assert out.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
            saved[tag] = torch.load(out.parent / "completion.pt")
    finally:
        torch.set_grad_enabled(True)
    a, b, c = saved["flagless"], saved["none"], saved["knn"]
    assert set(a) == set(b) == set(c) == {"x_in", "mask", "x_out", "labels"}
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert all(torch.equal(a[k], c[k]) for k in ("x_in", "mask", "x_out"))
    _, lidar, _ = r2dm_amd.setup_model(str(ckpt), device="cuda", show_info=False, max_batch=4)
    samples, mask = completion_demo.semseg_inputs(c["x_out"].cuda(), lidar)
    depth = torch.where(mask != 0, samples[:, [0]], torch.full_like(mask, -1.0))
    want = postproc.KNN(20)(depth, a["labels"].cuda())[:, None]
    assert c["labels"].dtype == torch.int64 and torch.equal(c["labels"], want.cpu())
