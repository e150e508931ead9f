#!/usr/bin/env python3
"""Generate tests/golden/rangenet.npz by running the REAL reference's RangeNet (metrics/extractor/rangenet.py) on the CPU in fp32 and,
with ``.double()``, in fp64, with r2dm_amd.synthetic.synthetic_rangenet_state(0).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rangenet.py /path/to/reference

torchvision, which the reference module imports at the top for its Preprocess, is replaced by a stub: Preprocess is checked by its
formula (tests/rangenet_oracle.py: preprocess) instead.

Contents (data only):
  - stored cases (2,5,4,64) -- bottleneck 2 wide --, (1,5,5,96) -- odd H, bottleneck 3 wide -- and (3,5,2,32) -- bottleneck 1 wide:
    every 3 x 3 tap there is padding --: the inputs (``x_*``), the reference's fp64 decoder map and logits (``dec64_*``, ``log64_*``);
  - for those and for (1,5,4,64) with backbone 21 and (1,5,64,1024), whose inputs the tests regenerate from integer draws (``images``):
    ``err_dec_*`` / ``err_log_*`` = [rms, max] of the reference's fp32 run against its fp64 run;
  - ``keys_53`` / ``keys_21``: the reference module's state-dict keys without ``num_batches_tracked``; ``indices``: the reference's
    subsample indices of a 32 x 64 x 1024 map; ``label_colors``: colorize(labels / 19, cmap) of the reference for labels 0 .. 19.
Asserted here: tests/rangenet_oracle.py equals the reference in fp64 to 1e-12; on the synthetic state every layer's fp64 activation has
|max| < 1e3 and rms > 1e-3 and a quarter of the pre-activations are negative; the reference's fp32 labels equal the fp64 ones wherever
the fp64 top-two margin exceeds 8x its max logit error, and those pixels are at least 99 %; the archive written by
``archive_members`` loads in the reference's own loader to the tensors r2dm_amd.rangenet.load_weights returns."""
import io
import os
import random
import sys
import tarfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "rangenet.npz")

STATE_SEED = 0
STORED_CASES = [("b2", 51, (2, 5, 4, 64), 53), ("oddh", 52, (1, 5, 5, 96), 53), ("w32", 53, (3, 5, 2, 32), 53)]  # name, seed, shape, backbone
REGEN_CASES = [("bb21", 54, (1, 5, 4, 64), 21), ("full", 55, (1, 5, 64, 1024), 53)]
MARGIN, MAX_EXCLUDED = 8.0, 0.01
ARCH_YAML = {"backbone": {"name": "darknet", "input_depth": {"range": True, "xyz": True, "remission": True},
                          "extra": {"layers": 53}},
             "dataset": {"sensor": {"img_means": [12.0, 10.5, 0.25, -1.0, 0.2], "img_stds": [12.5, 11.0, 7.0, 0.875, 0.125]}}}


def images(seed, shape):
    """(B,5,H,W) samples [depth, x, y, z, reflectance] from integer draws: a quarter of the depths on 0.5 / 63 and one ulp either side
    (and 0), x and y in [-75, 75), z in [-4, 4), reflectance in [0, 1)."""
    g = np.random.Generator(np.random.PCG64(seed))
    B, _, H, W = shape
    img = np.empty(shape, np.float32)
    img[:, 0] = g.integers(0, 80 * 2**10, size=(B, H, W)) / 2**10
    f = np.float32
    special = np.array([0.5, np.nextafter(f(0.5), f(0)), np.nextafter(f(0.5), f(1)), 63.0, np.nextafter(f(63), f(0)),
                        np.nextafter(f(63), f(100)), 0.0], np.float32)
    sel = g.integers(0, 4, size=(B, H, W)) == 0
    img[:, 0][sel] = special[g.integers(0, len(special), size=int(sel.sum()))]
    img[:, 1:3] = g.integers(-75 * 2**12, 75 * 2**12, size=(B, 2, H, W)) / 2**12
    img[:, 3] = g.integers(-4 * 2**12, 4 * 2**12, size=(B, H, W)) / 2**12
    img[:, 4] = g.integers(0, 2**12, size=(B, H, W)) / 2**12
    return img


def bonnetal_name(key):
    """The inverse of r2dm_amd.rangenet.module_key: (member, name in the official file) of a module-layout key."""
    parts = key.split(".")
    leaf = parts[-1]
    if parts[0] == "head":
        return "segmentation_head", f"1.{leaf}"
    if parts[0] == "stem":
        return "backbone", f"{'conv1' if parts[1] == '0' else 'bn1'}.{leaf}"
    member = "backbone" if parts[0].startswith("enc") else "segmentation_decoder"
    if parts[1] == "conv":
        conv = "conv" if member == "backbone" else "upconv"
        return member, f"{parts[0]}.{conv if parts[2] == '0' else 'bn'}.{leaf}"
    block = f"residual_{parts[2]}" if member == "backbone" else "residual"
    return member, f"{parts[0]}.{block}.{'conv' if parts[5] == '0' else 'bn'}{int(parts[4]) + 1}.{leaf}"


def write_archive(path, state, layers=53):
    """An archive under the official member names holding ``state`` (module layout) under the official parameter names."""
    import torch
    import yaml

    arch = os.path.basename(str(path))[:-len(".tar.gz")]
    members = {"backbone": {}, "segmentation_decoder": {}, "segmentation_head": {}}
    for key, value in state.items():
        member, name = bonnetal_name(key)
        members[member][name] = value
    cfg = {**ARCH_YAML, "backbone": {**ARCH_YAML["backbone"], "extra": {"layers": layers}}}
    with tarfile.open(path, "w:gz") as tar:
        def add(name, data):
            info = tarfile.TarInfo(f"{arch}/{name}")
            info.size = len(data)
            tar.addfile(info, io.BytesIO(data))

        for member, sd in members.items():
            buf = io.BytesIO()
            torch.save(sd, buf)
            add(member, buf.getvalue())
        add("arch_cfg.yaml", yaml.safe_dump(cfg).encode())


def main(reference):
    sys.modules.setdefault("torchvision", types.ModuleType("torchvision"))  # (only Preprocess uses it)
    sys.path.insert(0, reference)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(HERE))
    import tempfile

    import torch
    from metrics.extractor import rangenet as ref  # (reference)

    import rangenet_oracle as O
    from r2dm_amd import rangenet as ours
    from r2dm_amd import synthetic

    torch.manual_seed(0)
    inputs = {"range": True, "xyz": True, "remission": True}
    out, models = {}, {}
    for backbone in (53, 21):
        sd = synthetic.synthetic_rangenet_state(STATE_SEED, backbone)
        assert any((v < 0).any() for k, v in sd.items() if k.endswith(".1.weight") and v.ndim == 1), "negative BatchNorm scales"
        m32 = ref.RangeNet(inputs, 20, backbone=backbone)
        m32.load_state_dict(sd, strict=True)
        m32.eval().requires_grad_(False)
        m64 = ref.RangeNet(inputs, 20, backbone=backbone)
        m64.load_state_dict(sd, strict=True)
        m64.eval().requires_grad_(False).double()
        models[backbone] = (sd, m32, m64)
        keys = [k for k in m32.state_dict() if not k.endswith("num_batches_tracked")]
        assert keys == list(ours.state_spec(backbone)), "state_spec differs from the reference module"
        out[f"keys_{backbone}"] = np.array(keys)

    def run(name, x, backbone, store):
        sd, m32, m64 = models[backbone]
        t = torch.from_numpy(x)
        with torch.no_grad():
            p32, p64 = O.preprocess(t), O.preprocess(t.double())
            dec32, log32 = m32(p32, feature="decoder").numpy(), m32(p32).numpy()
            dec64, log64 = m64(p64, feature="decoder"), m64(p64)
            trace = []
            odec, olog = O.forward(O.cast(sd, torch.float64), p64, backbone, trace)
        for a, b in ((odec, dec64), (olog, log64)):
            assert (a - b).abs().max().item() <= 1e-12 * b.abs().max().item(), "the oracle differs from the reference"
        for layer, pre, act in trace:
            assert act.abs().max().item() < 1e3, (layer, act.abs().max().item())
            assert act.pow(2).mean().sqrt().item() > 1e-3, (layer, act.pow(2).mean().sqrt().item())
        neg = sum((pre < 0).sum().item() for _, pre, _ in trace) / sum(pre.numel() for _, pre, _ in trace)
        assert neg > 0.25, neg
        amax = max(act.abs().max().item() for _, _, act in trace)
        dec64, log64 = dec64.numpy(), log64.numpy()
        errs = {}
        for tag, a, b in (("dec", dec32, dec64), ("log", log32, log64)):
            d = a.astype(np.float64) - b
            errs[tag] = np.array([np.sqrt(np.mean(d * d)), np.abs(d).max()])
            assert errs[tag][0] > 0, "the reference's own error must be measurable"
            out[f"err_{tag}_{name}"] = errs[tag]
        top2 = np.sort(log64, axis=1)[:, -2:]
        sure = (top2[:, 1] - top2[:, 0]) > MARGIN * errs["log"][1]
        assert (log32.argmax(1) == log64.argmax(1))[sure].all() and 1 - sure.mean() <= MAX_EXCLUDED, (name, 1 - sure.mean())
        print(f"{name}: {x.shape} backbone {backbone}; fp32 against fp64: decoder rms {errs['dec'][0]:.3e} max {errs['dec'][1]:.3e}, logits rms "
              f"{errs['log'][0]:.3e} max {errs['log'][1]:.3e}; |act| max {amax:.1f}, decoder rms {np.sqrt(np.mean(dec64**2)):.2f}, negative "
              f"pre-activations {neg:.1%}, pixels within the label margin {1 - sure.mean():.3%}")
        if store:
            out[f"x_{name}"], out[f"dec64_{name}"], out[f"log64_{name}"] = x, dec64, log64

    for name, seed, shape, backbone in STORED_CASES:
        run(name, images(seed, shape), backbone, True)
    for name, seed, shape, backbone in REGEN_CASES:
        run(name, images(seed, shape), backbone, False)

    # the reference's subsample indices (global generator, as it draws them) and ours
    state = random.getstate()
    random.seed(0)
    idx = random.sample(range(32 * 64 * 1024), 4096)
    random.setstate(state)
    assert idx == ours.subsample_indices(32 * 64 * 1024)
    out["indices"] = np.array(idx, np.int32)

    # label colours: the reference's colorize(labels / 19, cmap)
    import make_golden_render

    make_golden_render.install_kornia_stand_in()  # (the reference's render module imports kornia; colorize does not use it)
    from utils import render as ref_render  # (reference)

    labels = torch.arange(20).view(1, 1, 1, 20)
    out["label_colors"] = ref_render.colorize(labels.float() / 19, ref.make_semantickitti_cmap())[0, :, 0].T.numpy().astype(np.uint8)

    # the archive loader against the reference's own
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "darknet53-1024.tar.gz")
        write_archive(path, models[53][0])
        ref.Preprocess = lambda mean, std: (mean, std)
        ref_sd, (ref_mean, ref_std), ref_cfg = ref._download_pretrained_weights(path)
        sd, mean, std, backbone, classes = ours.load_weights(path)
        assert list(ref_sd) == list(sd) and all(torch.equal(ref_sd[k], sd[k]) for k in sd), "archive loader differs from the reference's"
        assert (mean, std, backbone, classes) == (ref_mean, ref_std, ref_cfg["backbone"], ref_cfg["num_classes"])
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
