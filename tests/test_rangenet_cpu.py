"""CPU tests of the FRD's host side: the state-dict layout against the reference module's recorded keys, the BatchNorm fold, the
subsample indices, the weight-file loaders and their errors, the label colours and the scripts' options (tests/golden/rangenet.npz,
tests/golden/make_golden_rangenet.py)."""
import os
import random
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
import make_golden_rangenet as G  # noqa: E402  (the fixture's integer-only input generators and the archive writer)
import rangenet_oracle as O  # noqa: E402

from r2dm_amd import rangenet, render, synthetic  # noqa: E402


@pytest.fixture(scope="module")
def data():
    with np.load(os.path.join(GOLDEN, "rangenet.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def state():
    return synthetic.synthetic_rangenet_state(G.STATE_SEED)


@pytest.mark.parametrize("backbone", [53, 21])
def test_state_spec_is_the_reference_modules_key_list(data, backbone):
    assert list(rangenet.state_spec(backbone)) == list(data[f"keys_{backbone}"])
    sd = synthetic.synthetic_rangenet_state(G.STATE_SEED, backbone)
    assert [k for k in sd if not k.endswith("num_batches_tracked")] == list(data[f"keys_{backbone}"])
    assert all(tuple(sd[k].shape) == shape for k, shape in rangenet.state_spec(backbone).items())
    assert rangenet.infer_arch(sd) == (backbone, 5, 20)
    blocks = len({k.split(".residual.")[0] for k in sd if ".residual." in k})
    assert blocks == sum(rangenet.RESIDUAL_BLOCKS[backbone]) + 5
    assert rangenet.state_spec(53, in_ch=4, num_classes=7)["stem.0.weight"] == (32, 4, 3, 3)
    assert rangenet.state_spec(53, num_classes=7)["head.1.bias"] == (7,)
    with pytest.raises(ValueError, match="21 or 53"):
        rangenet.state_spec(34)


def test_synthetic_state_is_deterministic_and_adversarial(state):
    again = synthetic.synthetic_rangenet_state(G.STATE_SEED)
    assert set(state) == set(again) and all(torch.equal(state[k], again[k]) for k in state)
    assert not torch.equal(state["enc3.conv.0.weight"], synthetic.synthetic_rangenet_state(G.STATE_SEED + 1)["enc3.conv.0.weight"])
    scales = [v for k, v in state.items() if k.endswith(".1.weight") and v.ndim == 1]
    assert len(scales) == 1 + 2 * 5 + 2 * 28 and all((v < 0).any() and (v > 0).any() for v in scales)
    assert all(v.min() >= 0.75 for k, v in state.items() if k.endswith("running_var"))


def test_generators_reproduce_the_stored_inputs(data):
    for name, seed, shape, _ in G.STORED_CASES:
        assert np.array_equal(G.images(seed, shape), data[f"x_{name}"]), name
    depth = np.concatenate([data[f"x_{name}"][:, 0].ravel() for name, *_ in G.STORED_CASES])
    f = np.float32
    for v in (f(0.5), np.nextafter(f(0.5), f(0)), np.nextafter(f(0.5), f(1)), f(63), np.nextafter(f(63), f(0)), np.nextafter(f(63), f(100)), f(0)):
        assert (depth == v).any(), v


def test_fold_state_against_fp64_batch_norm(state):
    sd = {k: v.clone() for k, v in state.items()}
    sd["dec3.conv.1.weight"][3] = -abs(sd["dec3.conv.1.weight"][3])  # (negative scales on purpose, where the bias is folded too)
    sd["enc2.conv.1.weight"][5] = -abs(sd["enc2.conv.1.weight"][5])
    folded = rangenet.fold_state(sd)
    assert len(folded) == 2 * (1 + 5 + 5 + 2 * 28 + 1)
    d = O.cast(sd, torch.float64)
    g = torch.Generator().manual_seed(1)

    def bn(h, name):
        return F.batch_norm(h, d[name + ".running_mean"], d[name + ".running_var"], d[name + ".weight"], d[name + ".bias"], False, 0.0, 1e-5)

    def close(a, b):
        assert (a - b).abs().max().item() <= 1e-6 * b.abs().max().item()

    for conv, kw in (("stem.0", dict(padding=1)), ("enc2.conv.0", dict(stride=(1, 2), padding=1)),
                     ("enc3.residual_blocks.4.residual.0.0", {}), ("dec1.residual_blocks.0.residual.1.0", dict(padding=1))):
        x = torch.randn(2, d[conv + ".weight"].shape[1], 3, 8, generator=g, dtype=torch.float64)
        want = bn(F.conv2d(x, d[conv + ".weight"], None, **kw), conv[:-1] + "1")
        close(F.conv2d(x, folded[conv + ".weight"].double(), folded[conv + ".bias"].double(), **kw), want)
        assert folded[conv + ".weight"].dtype == torch.float32 and folded[conv + ".weight"].shape == d[conv + ".weight"].shape
    # the transposed convolution: (Cin,Cout,1,4), the scale runs along dim 1, the convolution's own bias goes through the BatchNorm
    x = torch.randn(2, 256, 3, 4, generator=g, dtype=torch.float64)
    kw = dict(stride=(1, 2), padding=(0, 1))
    want = bn(F.conv_transpose2d(x, d["dec3.conv.0.weight"], d["dec3.conv.0.bias"], **kw), "dec3.conv.1")
    close(F.conv_transpose2d(x, folded["dec3.conv.0.weight"].double(), folded["dec3.conv.0.bias"].double(), **kw), want)
    assert (folded["dec3.conv.0.weight"][:, 3] * d["dec3.conv.0.weight"][:, 3]).sum() < 0  # (the negative scale reached the weights)
    # the head has no BatchNorm: unchanged
    assert torch.equal(folded["head.1.weight"], sd["head.1.weight"]) and torch.equal(folded["head.1.bias"], sd["head.1.bias"])


def test_state_dict_errors_name_the_key(state):
    sd = dict(state)
    del sd["enc4.residual_blocks.6.residual.1.1.running_var"]
    with pytest.raises(KeyError, match="enc4.residual_blocks.6.residual.1.1.running_var"):
        rangenet.fold_state(sd)
    sd = dict(state)
    sd["dec2.conv.0.weight"] = state["dec2.conv.0.weight"].transpose(0, 1)
    with pytest.raises(ValueError, match="dec2.conv.0.weight"):
        rangenet.check_state(sd)
    sd = dict(state)
    sd["enc1.conv.0.weight"] = state["enc1.conv.0.weight"].clone()
    sd["enc1.conv.0.weight"][3, 2, 1, 1] = float("nan")
    with pytest.raises(ValueError, match="enc1.conv.0.weight.*non-finite"):
        rangenet.check_state(sd)
    with pytest.raises(KeyError, match="enc2.residual_blocks.1.residual.0.0.weight"):  # a backbone-21 state is not a backbone-53 one
        rangenet.check_state(synthetic.synthetic_rangenet_state(0, 21), backbone=53)
    rangenet.check_state({k: v for k, v in state.items() if not k.endswith("num_batches_tracked")})  # (optional)
    with pytest.raises(Exception, match="no CPU fallback"):
        rangenet.RangeNetExtractor(state, device="cpu")


def test_subsample_indices_are_the_references_and_leave_the_global_generator_alone(data):
    random.seed(123)
    before = random.getstate()
    idx = rangenet.subsample_indices(32 * 64 * 1024)
    assert random.getstate() == before
    assert idx == data["indices"].tolist() and len(set(idx)) == 4096
    random.seed(0)
    assert rangenet.subsample_indices(32 * 4 * 64) == random.sample(range(32 * 4 * 64), 4096)
    with pytest.raises(ValueError, match="4096"):
        rangenet.subsample_indices(32 * 2 * 32)


def test_archive_loader(tmp_path, state):
    path = tmp_path / "darknet53-1024.tar.gz"
    G.write_archive(path, state)
    sd, mean, std, backbone, classes = rangenet.load_weights(path)
    assert list(sd) == list(state) and all(torch.equal(sd[k], state[k]) for k in state)
    sensor = G.ARCH_YAML["dataset"]["sensor"]
    assert (mean, std, backbone, classes) == (sensor["img_means"], sensor["img_stds"], 53, 20)
    # every official name maps back to the key it came from
    for key in state:
        assert rangenet.module_key(G.bonnetal_name(key)[1]) == key
    with pytest.raises(ValueError, match="unknown RangeNet parameter name"):
        rangenet.module_key("enc1.residual_0.conv3.weight")
    small = synthetic.synthetic_rangenet_state(0, 21)
    G.write_archive(tmp_path / "darknet21.tar.gz", small, layers=21)
    sd21, _, _, backbone, _ = rangenet.load_weights(str(tmp_path / "darknet21.tar.gz"))
    assert backbone == 21 and list(sd21) == list(small)
    # an archive under another name has other member names
    os.rename(path, tmp_path / "other.tar.gz")
    with pytest.raises(KeyError, match="other/backbone"):
        rangenet.load_weights(tmp_path / "other.tar.gz")


def test_state_dict_file_loader(tmp_path, state):
    torch.save(state, tmp_path / "rangenet.pth")
    sd, mean, std, backbone, classes = rangenet.load_weights(tmp_path / "rangenet.pth")
    assert all(torch.equal(sd[k], state[k]) for k in state)
    assert (mean, std, backbone, classes) == ([12.12, 10.88, 0.23, -1.04, 0.21], [12.32, 11.47, 6.91, 0.86, 0.16], 53, 20)
    assert (mean, std) == (list(O.MEAN), list(O.STD))


@pytest.mark.parametrize("name", ["http://www.ipb.uni-bonn.de/html/projects/bonnetal/lidar/semantic/models/darknet53-1024.tar.gz",
                                  "https://example.org/darknet53.tar.gz", "SemanticKITTI_64x1024", "darknet53"])
def test_nothing_is_downloaded(name, monkeypatch):
    def no_io(*a, **k):
        raise AssertionError("I/O before the name was refused")

    monkeypatch.setattr(torch, "load", no_io)
    monkeypatch.setattr(rangenet.tarfile, "open", no_io)
    with pytest.raises(ValueError, match="nothing is downloaded"):
        rangenet.load_weights(name)
    with pytest.raises(ValueError, match="nothing is downloaded"):
        rangenet.pretrained_rangenet(name)


def test_label_colours_are_the_references(data):
    assert np.array_equal(np.array(render.LABEL_COLORS, np.uint8), data["label_colors"])
    # colorize(labels / 19, lut) as the reference computes it: ids = (labels / 19 * 256).clamp(0, 255), table sampled at linspace(0, 1, 256)
    lut = render.label_lut()
    assert lut.shape == (256, 3)
    ids = (torch.arange(20).float() / 19 * 256).clamp(0, 255).long()
    assert np.array_equal(lut[ids].mul(255).clamp(0, 255).byte().numpy(), data["label_colors"])


def test_scripts_have_the_option():
    sys.path.insert(0, ROOT)
    import completion_demo
    import evaluate

    args = evaluate.build_parser().parse_args(["--ckpt", "c.pth", "--sample_dir", "d", "--rangenet_weights", "w.tar.gz"])
    assert args.rangenet_weights == "w.tar.gz" and args.pointnet_weights is None
    assert evaluate.build_parser().parse_args(["--ckpt", "c.pth", "--sample_dir", "d"]).rangenet_weights is None
    args = completion_demo.parser().parse_args(["--ckpt", "c.pth", "--scan", "s.bin", "--rangenet_weights", "w.pth"])
    assert args.rangenet_weights == "w.pth"
    assert completion_demo.parser().parse_args(["--ckpt", "c.pth", "--scan", "s.bin"]).rangenet_weights is None
