"""CPU tests of the FPD's host side: the fp64 oracle against the reference's recorded features (tests/golden/pointnet.npz,
tests/golden/make_golden_pointnet.py), the BatchNorm fold, state-dict errors, evaluate.py's options and the subset draws."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
import make_golden_pointnet as G  # noqa: E402  (the fixture's integer-only input generators)
import pointnet_oracle as O  # noqa: E402

from r2dm_amd import metrics, pointnet, synthetic  # noqa: E402

STORED = [c[0] for c in G.CLOUD_CASES] + ["images"]


@pytest.fixture(scope="module")
def data():
    with np.load(os.path.join(GOLDEN, "pointnet.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def state():
    return synthetic.synthetic_pointnet_state(G.STATE_SEED)


def _clouds(data, name):
    x = torch.from_numpy(data[f"x_{name}"])
    return O.sample_clouds(x) if name == "images" else x


def _err(got, want):
    d = got.double() - want.double()
    return d.pow(2).mean().sqrt().item(), d.abs().max().item()


def test_synthetic_state_is_deterministic_and_adversarial(state):
    again = synthetic.synthetic_pointnet_state(G.STATE_SEED)
    assert len(state) == 74 and set(state) == set(again) and all(torch.equal(state[k], again[k]) for k in state)
    assert set(pointnet.state_spec()) == {k for k in state if not k.endswith("num_batches_tracked")}
    other = synthetic.synthetic_pointnet_state(G.STATE_SEED + 1)
    assert not torch.equal(state["feat.conv3.weight"], other["feat.conv3.weight"])
    for k, v in state.items():
        if ".bn" in "." + k and k.endswith(".weight"):
            assert (v < 0).any() and (v > 0).any() and v.abs().min() >= 0.5, k
        if k.endswith("running_var"):
            assert v.min() >= 0.5, k


def test_generators_reproduce_the_stored_inputs(data):
    for name, seed, B, N in G.CLOUD_CASES:
        assert np.array_equal(G.cloud(seed, B, N), data[f"x_{name}"]), name
    assert np.array_equal(G.images(), data["x_images"])
    img = data["x_images"]
    special = [np.float32(0.5), np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1)),
               np.float32(63), np.nextafter(np.float32(63), np.float32(0)), np.nextafter(np.float32(63), np.float32(100))]
    assert all((img[:, 0] == v).any() for v in special)


@pytest.mark.parametrize("name", STORED)
def test_oracle_reproduces_the_references_fp64_features(data, state, name):
    got, trans = O.features(state, _clouds(data, name).double(), return_trans=True)
    want = torch.from_numpy(data[f"f64_{name}"])
    assert got.shape == want.shape == (want.shape[0], 1808)
    assert (got - want).abs().max().item() <= 1e-12
    assert (trans - torch.from_numpy(data[f"trans_{name}"])).abs().max().item() <= 1e-12
    assert (want[:, :1024] < 0).double().mean().item() > 0.25  # a maximum that starts at 0 is wrong for these


@pytest.mark.parametrize("name", STORED)
def test_folded_fp32_weights_stay_within_the_references_own_error(data, state, name):
    """BatchNorm folded in fp64 and cast to fp32, the network then evaluated exactly (fp64): the weights' rounding alone."""
    got = O.folded_features(pointnet.fold_state(state), _clouds(data, name).double())
    rms, mx = _err(got, torch.from_numpy(data[f"f64_{name}"]))
    ref_rms, ref_max = data[f"err_{name}"]
    print(f"{name}: folded fp32 weights rms {rms:.3e} max {mx:.3e}; reference rms {ref_rms:.3e} max {ref_max:.3e}")
    assert rms <= ref_rms and mx <= ref_max


def test_fold_is_in_the_weights(state):
    f = pointnet.fold_state(state)
    s = (state["feat.bn3.weight"].double() / torch.sqrt(state["feat.bn3.running_var"].double() + 1e-5))
    assert (s < 0).any()
    want = state["feat.conv3.weight"].double()[:, :, 0] * s[:, None]
    assert torch.equal(f["feat.conv3.weight"], want.float())
    assert set(f) == {f"{n}.{leaf}" for n in ("feat.stn.conv1", "feat.stn.conv2", "feat.stn.conv3", "feat.stn.fc1", "feat.stn.fc2",
                                                "feat.stn.fc3", "feat.conv1", "feat.conv2", "feat.conv3", "fc1", "fc2", "fc3")
                      for leaf in ("weight", "bias")}


def test_state_dict_errors_name_the_key(state, tmp_path):
    missing = {k: v for k, v in state.items() if k != "feat.stn.bn4.running_var"}
    with pytest.raises(KeyError, match="feat.stn.bn4.running_var"):
        pointnet.pretrained_pointnet(missing)
    bad = dict(state)
    bad["fc3.weight"] = torch.zeros(2, 256)  # (a classifier with another number of classes)
    with pytest.raises(ValueError, match="fc3.weight"):
        pointnet.pretrained_pointnet(bad)
    path = tmp_path / "weights.pth"
    torch.save(missing, path)
    with pytest.raises(KeyError, match="feat.stn.bn4.running_var"):
        pointnet.pretrained_pointnet(path)
    without_counters = {k: v for k, v in state.items() if not k.endswith("num_batches_tracked")}
    assert len(without_counters) == 64 and set(pointnet.check_state(without_counters)) == set(without_counters)


def test_extractor_has_no_cpu_fallback(state):
    from r2dm_amd import _lib

    with pytest.raises(_lib.R2DMError, match="no CPU fallback"):
        pointnet.pretrained_pointnet(state, device="cpu")
    for call in (lambda: metrics.feature_moments(torch.zeros(4, 8)),
                 lambda: metrics.compute_frechet_distance(torch.zeros(4, 8), torch.zeros(4, 8)),
                 lambda: metrics.compute_squared_mmd(torch.zeros(4, 8), torch.zeros(4, 8), num_subsets=2)):
        with pytest.raises(_lib.R2DMError, match="no CPU fallback"):
            call()


def test_evaluate_options():
    sys.path.insert(0, ROOT)
    import evaluate

    base = ["--ckpt", "model.pth", "--sample_dir", "samples"]
    args = evaluate.build_parser().parse_args(base)
    assert args.pointnet_weights is None and args.mmd_seed is None
    assert args.batch_size == 64 and args.num_workers == 4 and args.dataset == "all"
    args = evaluate.build_parser().parse_args(base + ["--pointnet_weights", "cls_model_39.pth", "--mmd_seed", "7"])
    assert args.pointnet_weights == "cls_model_39.pth" and args.mmd_seed == 7
    with pytest.raises(SystemExit):
        evaluate.build_parser().parse_args(base + ["--mmd_seed", "x"])


@pytest.mark.parametrize("case", G.MMD_CASES, ids=[c[0] for c in G.MMD_CASES])
def test_subset_draws_are_the_recorded_ones(data, case):
    name, (_, n1), (_, n2), _, subsets, seed = case
    idx1, idx2 = metrics.draw_mmd_subsets(n1, n2, num_subsets=subsets, rng=np.random.RandomState(seed))
    assert np.array_equal(idx1, data[f"idx1_{name}"]) and np.array_equal(idx2, data[f"idx2_{name}"])
    state = np.random.get_state()
    try:  # rng = None: numpy's global state, as the reference
        np.random.seed(seed)
        g1, g2 = metrics.draw_mmd_subsets(n1, n2, num_subsets=subsets)
    finally:
        np.random.set_state(state)
    assert np.array_equal(g1, idx1) and np.array_equal(g2, idx2)
    assert idx1.shape == (subsets, min(n1, n2, 1000)) and all(len(set(r)) == len(r) for r in idx1)
