"""Without a GPU: the torch restatements of the kNN vote and the CRF-RNN (tests/postproc_oracle.py) against the reference's recorded
fp32 / fp64 runs (tests/golden/postproc.npz, tests/golden/make_golden_postproc.py), the tables, state dict, hub entries and argument
checks of r2dm_amd.postproc."""
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
import make_golden_postproc as G  # noqa: E402  (the fixture's integer-only input generators)
import postproc_oracle as O  # noqa: E402

from r2dm_amd import _lib, postproc  # noqa: E402


@pytest.fixture(scope="module")
def data():
    with np.load(os.path.join(GOLDEN, "postproc.npz")) as z:
        return {k: z[k] for k in z.files}


def knn_inputs(data, case):
    name, seed, shape, ks, k, cutoff, stored, kind = case
    if stored:
        return torch.from_numpy(data[f"depth_{name}"]), torch.from_numpy(data[f"label_{name}"]).long()
    depth, label = G.knn_scene(seed, shape, kind)
    return torch.from_numpy(depth), torch.from_numpy(label)


def test_stored_inputs_are_the_generators(data):
    for case in G.KNN_CASES:
        if case[6]:
            depth, label = G.knn_scene(case[1], case[2], case[7])
            assert np.array_equal(depth, data[f"depth_{case[0]}"]) and np.array_equal(label, data[f"label_{case[0]}"])
    for name, seed, shape, ks, iters, stored, params in G.CRF_CASES:
        if stored:
            for key, a in zip(("unary", "xyz", "mask"), G.crf_inputs(seed, shape)):
                assert np.array_equal(a, data[f"{key}_{name}"]), (name, key)


@pytest.mark.parametrize("case", G.KNN_CASES, ids=[c[0] for c in G.KNN_CASES])
def test_knn_oracle_against_the_reference(data, case):
    """fp64: the reference's fp64 labels on every pixel.  fp32: its fp32 labels on the sure pixels, which are at least 99 % (measured when
    the fixture was made: 0.07 % / 0.75 % / 0 % / 0.22 % / 0.85 % / 0 % / 0.41 % left out, and equal on every pixel)."""
    name, seed, shape, ks, k, cutoff = case[:6]
    depth, label = knn_inputs(data, case)
    d32, d64 = O.knn_dist(depth, O.knn_weight(ks, 1.0, torch.float32)), O.knn_dist(depth, O.knn_weight(ks, 1.0, torch.float64))
    o32, o64 = (O.knn_vote(d, label, ks, k, cutoff, G.NUM_CLASSES) for d in (d32, d64))
    r32, r64 = torch.from_numpy(data[f"knn32_{name}"]).long(), torch.from_numpy(data[f"knn64_{name}"]).long()
    assert torch.equal(o64, r64)
    sure, margin = O.knn_sure(d64, d32, k, cutoff)
    excluded = 1 - sure.double().mean().item()
    print(f"{name}: margin {margin:.3e}, excluded {excluded:.3%}, fp32 oracle == reference fp32 on {(o32 == r32).double().mean().item():.4%}")
    assert excluded <= G.MAX_EXCLUDED
    assert torch.equal(o32[sure], r32[sure]) and torch.equal(o32[sure], r64[sure])
    assert torch.equal(O.knn(depth, label, ks, k, 1.0, cutoff, G.NUM_CLASSES), o32)


def crf_state(data, name, N, ks, iters, params):
    """the reference module's state dict of a case: recorded for "custom", else what the constructor arguments give"""
    if params == "custom":
        return {k[len("crfstate_custom_"):]: torch.from_numpy(v) for k, v in data.items() if k.startswith("crfstate_custom_")}
    return postproc.CRFRNN(N, kernel_size=ks, num_iters=iters, **G.crf_kwargs(params, N)).state_dict()


@pytest.mark.parametrize("case", [c for c in G.CRF_CASES if c[5]], ids=[c[0] for c in G.CRF_CASES if c[5]])
def test_crf_oracle_against_the_reference(data, case):
    name, seed, shape, ks, iters, stored, params = case
    unary, xyz, mask = (torch.from_numpy(data[f"{k}_{name}"]) for k in ("unary", "xyz", "mask"))
    q64 = torch.from_numpy(data[f"q64_{name}"])
    got = O.crf(unary, xyz, mask, crf_state(data, name, shape[1], ks, iters, params), ks, iters, torch.float64)
    assert (got - q64).abs().max().item() <= 1e-12 * q64.abs().max().item()
    err = data[f"err_crf_{name}"]
    d = O.crf(unary, xyz, mask, crf_state(data, name, shape[1], ks, iters, params), ks, iters, torch.float32).double() - q64
    assert d.pow(2).mean().sqrt().item() <= 2 * err[0] and d.abs().max().item() <= 4 * err[1]  # (the bar of the GPU test is reachable)


def test_tables_equal_the_references(data):
    assert torch.equal(postproc.KNN(20).dist_kernel, torch.from_numpy(data["gauss_3"]))
    assert torch.equal(postproc.KNN(20, k=5, kernel_size=5).dist_kernel, torch.from_numpy(data["gauss_5"]))
    assert torch.equal(O.knn_weight(5, 1.0), torch.from_numpy(data["gauss_5"]))
    crf = postproc.CRFRNN(20)
    assert torch.equal(crf.state_dict()["kernel_gamma"], torch.from_numpy(data["kernel_gamma"]))
    assert torch.equal(crf.state_dict()["kernel_alpha"], torch.from_numpy(data["kernel_gamma"]))  # (the same theta by default)


def test_crf_state_dict(data):
    crf = postproc.CRFRNN(20)
    sd = crf.state_dict()
    assert list(sd) == list(data["crf_keys"]) == list(postproc.crf_state_spec(20))
    assert [",".join(str(n) for n in v.shape) for v in sd.values()] == list(data["crf_shapes"])
    assert all(v.dtype == torch.float32 for v in sd.values())
    custom = crf_state(data, "custom", 20, (3, 5), 3, "custom")
    crf.load_state_dict(custom)
    back = crf.state_dict()
    assert list(back) == list(custom) and all(torch.equal(back[k], custom[k]) for k in custom)
    assert not crf._uniform_beta and postproc.CRFRNN(20)._uniform_beta
    # the kernel's parameter block holds the diagonals, the weights, 2 theta_beta^2 and the compatibility matrix
    N, K = 20, 15
    p = crf._params
    assert p.shape == (2 * N * K + 3 * N + N * N,)
    assert torch.equal(p[:N * K].view(N, 3, 5), torch.stack([custom["kernel_gamma"][c, c] for c in range(N)]))
    assert torch.equal(p[2 * N * K + 2 * N:2 * N * K + 3 * N], 2 * custom["theta_beta"] ** 2)
    assert torch.equal(p[-N * N:].view(N, N), custom["label_compatibility.weight"][:, :, 0, 0])
    bad = {k: v.clone() for k, v in custom.items()}
    bad["kernel_alpha"][3, 4, 1, 1] = 0.5
    with pytest.raises(ValueError, match="off the class diagonal"):
        crf.load_state_dict(bad)
    assert all(torch.equal(crf.state_dict()[k], custom[k]) for k in custom)  # (a refused state leaves the module as it was)
    with pytest.raises(KeyError, match="theta_beta"):
        crf.load_state_dict({k: v for k, v in custom.items() if k != "theta_beta"})
    with pytest.raises(ValueError, match="shape"):
        crf.load_state_dict({**custom, "weight_smoothness": torch.zeros(20)})


def _signature(fn):
    return [[p.name, None if p.default is inspect.Parameter.empty else (list(p.default) if isinstance(p.default, tuple) else p.default), p.kind.name]
            for p in inspect.signature(fn).parameters.values()]


def test_hub_entries_and_signatures(data):
    sys.path.insert(0, ROOT)
    import hubconf

    want = json.loads(str(data["hub"]))
    for name in ("rangenet", "rangenet21", "rangenet53", "knn", "crf_rnn"):
        assert _signature(getattr(hubconf, name)) == want[name], name
    assert _signature(postproc.KNN.__init__)[1:] == want["KNN"]
    assert _signature(postproc.CRFRNN.__init__)[1:] == want["CRFRNN"]
    knn, crf = hubconf.knn(), hubconf.crf_rnn(kernel_size=(3, 3), num_iters=1)
    assert isinstance(knn, postproc.KNN) and knn.num_classes == 20 and (knn.k, knn.kernel_size, knn.sigma, knn.cutoff) == (3, (3, 3), 1.0, 1.0)
    assert isinstance(crf, postproc.CRFRNN) and crf.num_classes == 20 and crf.kernel_size == (3, 3) and crf.num_iters == 1
    with pytest.raises(ValueError, match="weights"):
        hubconf.rangenet53("KITTI_8x8")
    with pytest.raises(ValueError, match="untrained"):
        hubconf.rangenet21(None)


def test_bad_arguments_raise_without_a_gpu():
    for kw in (dict(kernel_size=4), dict(kernel_size=(3, 2)), dict(kernel_size=9)):
        with pytest.raises(ValueError, match="window"):
            postproc.KNN(20, **kw)
        with pytest.raises(ValueError, match="window"):
            postproc.CRFRNN(20, **kw)
    with pytest.raises(ValueError, match="k must be"):
        postproc.KNN(20, k=10, kernel_size=3)  # k > K
    with pytest.raises(ValueError, match="k must be"):
        postproc.KNN(20, k=9, kernel_size=5)   # k > 8
    with pytest.raises(ValueError, match="k must be"):
        postproc.KNN(20, k=0)
    with pytest.raises(ValueError, match="classes"):
        postproc.KNN(33)
    with pytest.raises(ValueError, match="classes"):
        postproc.CRFRNN(33)
    with pytest.raises(ValueError, match="theta_gamma"):
        postproc.CRFRNN(20, theta_gamma=(0.9, 0.8))
    with pytest.raises(ValueError, match="before every KNN"):
        postproc.split_postprocess((postproc.KNN(20), postproc.CRFRNN(20)))
    with pytest.raises(TypeError, match="postprocess"):
        postproc.split_postprocess("knn")
    knn, crf = postproc.KNN(20), postproc.CRFRNN(20)
    assert postproc.split_postprocess(None) == ((), ()) and postproc.split_postprocess(knn) == ((), (knn,))
    assert postproc.split_postprocess([crf, knn]) == ((crf,), (knn,))


def test_cpu_tensors_are_refused():
    depth, label = torch.ones(1, 1, 4, 8), torch.zeros(1, 4, 8, dtype=torch.int64)
    with pytest.raises(_lib.R2DMError, match="no CPU fallback"):
        postproc.KNN(20)(depth, label)
    with pytest.raises(_lib.R2DMError, match="no CPU fallback"):
        postproc.CRFRNN(20)(torch.zeros(1, 20, 4, 8), torch.zeros(1, 3, 4, 8), torch.ones(1, 4, 8))
    with pytest.raises(ValueError, match=r"\(B,1,H,W\) depth"):
        postproc.KNN(20)(torch.ones(1, 2, 4, 8), label)
    with pytest.raises(ValueError, match="labels"):
        postproc.KNN(20)(depth, torch.zeros(1, 4, 9, dtype=torch.int64))
    with pytest.raises(ValueError, match="unary"):
        postproc.CRFRNN(20)(torch.zeros(1, 19, 4, 8), torch.zeros(1, 3, 4, 8), torch.ones(1, 4, 8))
