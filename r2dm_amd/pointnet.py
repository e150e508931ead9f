"""PointNet feature extractor of the evaluation's FPD (the reference's metrics/extractor/pointnet.py) as HIP kernels.

The network is SpareNet's ShapeNet classifier (``cls_model_39.pth``, 16 classes) in eval mode:

- a spatial transformer ``feat.stn``: point-wise 3 -> 64 -> 128 -> 1024 (BatchNorm + ReLU each), maximum over the points,
  1024 -> 512 -> 256 -> 9, plus the identity: a 3 x 3 matrix ``trans`` per cloud;
- the feature trunk ``feat``: points @ trans, point-wise 3 -> 64 -> 128 -> 1024 (BatchNorm each, ReLU on the first two),
  maximum over the points: ``x1``;
- the head: 1024 -> 512 (``x2``) -> 256 (``x3``) -> 16 (``x4``); the feature is ``cat(x1, x2, x3, x4)``, 1808 values.

Every BatchNorm (running statistics, eps 1e-5) is folded into the weights and bias of the layer in front of it on the host in
fp64 -- in the weights, because a BatchNorm scale may be negative and does not commute with the maximum.  A trunk is ONE kernel
(csrc/pointnet.hip): the 64-, 128- and 1024-channel activations never leave the chip, the two wide layers run on the fp16 matrix
pipe with split fp32 operands (three products per multiply-add, fp32 accumulation).  There is no CPU or PyTorch fallback and
nothing is ever downloaded: the weight file is given by the caller.
"""
from __future__ import annotations

import os
from typing import Dict, Union

import numpy as np
import torch

from . import _lib
from .metrics import MAX_DEPTH, MIN_DEPTH

DATASET_MAX_DEPTH = 80.0  # evaluate.py: the point clouds are divided by it before the extractor
FEATURE_DIM = 1808
BN_EPS = 1e-5
NUM_CLASSES = 16

_FLAG_COORD, _FLAG_RANGE, _FLAG_WEIGHT = 1, 2, 4


def state_spec(k: int = NUM_CLASSES) -> Dict[str, tuple]:
    """Key -> shape of the state dict in the SpareNet layout, without the BatchNorms' ``num_batches_tracked``."""
    spec: Dict[str, tuple] = {}

    def layer(name, cout, cin, conv):
        spec[name + ".weight"] = (cout, cin, 1) if conv else (cout, cin)
        spec[name + ".bias"] = (cout,)

    def norm(name, c):
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            spec[f"{name}.{leaf}"] = (c,)

    for pre in ("feat.stn.", "feat."):
        for i, (cout, cin) in enumerate(((64, 3), (128, 64), (1024, 128)), 1):
            layer(f"{pre}conv{i}", cout, cin, True)
            norm(f"{pre}bn{i}", cout)
    layer("feat.stn.fc1", 512, 1024, False)
    layer("feat.stn.fc2", 256, 512, False)
    layer("feat.stn.fc3", 9, 256, False)
    norm("feat.stn.bn4", 512)
    norm("feat.stn.bn5", 256)
    layer("fc1", 512, 1024, False)
    layer("fc2", 256, 512, False)
    layer("fc3", k, 256, False)
    norm("bn1", 512)
    norm("bn2", 256)
    return spec


def check_state(state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The tensors of ``state_spec`` as fp64 CPU tensors; KeyError / ValueError naming the first missing / mis-shaped key."""
    out = {}
    for key, shape in state_spec().items():
        if key not in state:
            raise KeyError(f"PointNet state dict lacks {key!r}")
        t = torch.as_tensor(state[key]).detach().cpu()
        if tuple(t.shape) != shape:
            raise ValueError(f"PointNet state dict: {key!r} has shape {tuple(t.shape)}, expected {shape}")
        out[key] = t.double()
    return out


def fold_state(state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Eval-mode BatchNorms folded into the layers in front of them, in fp64, cast to fp32 at the end:
    ``{layer}.weight`` (cout, cin) and ``{layer}.bias`` (cout,) for the 12 layers."""
    sd = check_state(state)
    pairs = [(f"{pre}conv{i}", f"{pre}bn{i}") for pre in ("feat.stn.", "feat.") for i in (1, 2, 3)]
    pairs += [("feat.stn.fc1", "feat.stn.bn4"), ("feat.stn.fc2", "feat.stn.bn5"), ("feat.stn.fc3", None),
              ("fc1", "bn1"), ("fc2", "bn2"), ("fc3", None)]
    out = {}
    for layer, bn in pairs:
        w, b = sd[layer + ".weight"].reshape(sd[layer + ".weight"].shape[0], -1), sd[layer + ".bias"]
        if bn is not None:
            s = sd[bn + ".weight"] / torch.sqrt(sd[bn + ".running_var"] + BN_EPS)
            w = w * s[:, None]
            b = (b - sd[bn + ".running_mean"]) * s + sd[bn + ".bias"]
        out[layer + ".weight"], out[layer + ".bias"] = w.float().contiguous(), b.float().contiguous()
    return out


class _Trunk:
    """Device-side weights of one 3 -> 64 -> 128 -> 1024 trunk and of the MLP behind its maximum."""

    def __init__(self, folded, pre, fcs, device, flag):
        L = _lib.lib()
        dev = lambda t: t.to(device).contiguous()
        self.w1b = dev(torch.cat([folded[pre + "conv1.weight"], folded[pre + "conv1.bias"][:, None]], 1))  # (64,4)
        self.b2, self.b3 = dev(folded[pre + "conv2.bias"]), dev(folded[pre + "conv3.bias"])
        self.packed, self.scale = [], []
        for name in ("conv2", "conv3"):
            w = dev(folded[f"{pre}{name}.weight"])
            cout, cin = w.shape
            packed = torch.empty(L.r2dm_pointnet_packed_bytes(cout, cin), dtype=torch.uint8, device=device)
            scale = torch.zeros(2, dtype=torch.float32, device=device)
            _lib.check(L.r2dm_pointnet_pack(_lib.ptr(w), cout, cin, _lib.ptr(packed), _lib.ptr(scale), _lib.ptr(flag),
                                            _lib.stream_ptr(device)))
            self.packed.append(packed)
            self.scale.append(scale)
        self.fc = [dev(folded[f"{n}.{leaf}"]) for n in fcs for leaf in ("weight", "bias")]
        self.outputs = self.fc[4].shape[0]


class PointNetExtractor:
    """Callable as the reference's extractor: ``(B,3,N)`` fp32 clouds on the GPU -> ``(B,1808)`` fp32 features."""

    max_batch = 4096  # clouds per launch

    def __init__(self, state: Dict[str, torch.Tensor], device="cuda"):
        folded = fold_state(state)  # (first: a bad state dict is reported without a GPU)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.R2DMError(f"PointNet extractor on {self.device}: r2dm_amd has no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._stn = _Trunk(folded, "feat.stn.", ("feat.stn.fc1", "feat.stn.fc2", "feat.stn.fc3"), self.device, self._flag)
            self._feat = _Trunk(folded, "feat.", ("fc1", "fc2", "fc3"), self.device, self._flag)
            if int(self._flag.item()) & _FLAG_WEIGHT:
                raise ValueError("PointNet state dict holds a non-finite weight")

    def _trunk(self, t: _Trunk, src, layout, B, n, trans, lo, hi, div, scratch, out, stn):
        L, s = _lib.lib(), _lib.stream_ptr(self.device)
        _lib.check(L.r2dm_pointnet_trunk(_lib.ptr(src), layout, B, n, _lib.ptr(trans), lo, hi, div, _lib.ptr(t.w1b), _lib.ptr(t.packed[0]),
                                         t.scale[0].data_ptr() + 4, _lib.ptr(t.b2), _lib.ptr(t.packed[1]), _lib.ptr(scratch), scratch.numel(),
                                         _lib.ptr(self._flag), s))
        _lib.check(L.r2dm_pointnet_head(_lib.ptr(scratch), t.scale[1].data_ptr() + 4, _lib.ptr(t.b3), int(stn), *[_lib.ptr(w) for w in t.fc],
                                        t.outputs, _lib.ptr(out), B, s))

    @torch.no_grad()
    def extract(self, src: torch.Tensor, layout: int, n: int, image_min_depth: float = MIN_DEPTH, image_max_depth: float = MAX_DEPTH,
                divisor: float = DATASET_MAX_DEPTH, return_trans: bool = False):
        """``src`` in kernel layout 0 ``(B,5,H,W)`` samples (masked by the depth window and divided by ``divisor`` in the kernel),
        1 ``(B,N,3)`` or 2 ``(B,3,N)`` clouds (taken as they are)."""
        _lib.require_gpu(src, "clouds")
        if src.device != self.device:
            raise ValueError(f"clouds on {src.device}, extractor on {self.device}")
        if n == 0:
            raise ValueError("a point cloud must have at least one point")
        src = _lib.f32c(src)
        B = src.shape[0]
        feats = torch.empty(B, FEATURE_DIM, dtype=torch.float32, device=self.device)
        trans = torch.empty(B, 9, dtype=torch.float32, device=self.device)
        if B == 0:
            return (feats, trans.view(0, 3, 3)) if return_trans else feats
        L = _lib.lib()
        with torch.cuda.device(self.device):
            self._flag.zero_()
            for k in range(0, B, self.max_batch):
                part, nb = src[k:k + self.max_batch], min(self.max_batch, B - k)
                scratch = torch.empty(L.r2dm_pointnet_scratch_bytes(nb), dtype=torch.uint8, device=self.device)
                args = (float(image_min_depth), float(image_max_depth), float(divisor), scratch)
                self._trunk(self._stn, part, layout, nb, n, None, *args, trans[k:k + nb], True)
                self._trunk(self._feat, part, layout, nb, n, trans[k:k + nb], *args, feats[k:k + nb], False)
            flag = int(self._flag.item())
        if flag & _FLAG_COORD:
            raise RuntimeError("PointNet extractor: a point has a non-finite coordinate")
        if flag & _FLAG_RANGE:
            raise RuntimeError("PointNet extractor: an activation left the fp16 operand range (65504) of the matrix-core layers; "
                               "the features of this call are not valid")
        return (feats, trans.view(B, 3, 3)) if return_trans else feats

    def __call__(self, clouds: torch.Tensor) -> torch.Tensor:
        if clouds.ndim != 3 or clouds.shape[1] != 3:
            raise ValueError(f"expected (B,3,N) point clouds, got {tuple(clouds.shape)}")
        return self.extract(clouds, 2, clouds.shape[2])


def pretrained_pointnet(weights: Union[str, os.PathLike, Dict[str, torch.Tensor]], device="cuda") -> PointNetExtractor:
    """The extractor with the weights of ``weights``: a state dict in the SpareNet key layout (``cls_model_39.pth``) or the path
    of one.  A missing key is a KeyError, a mis-shaped one a ValueError, both naming it."""
    if not isinstance(weights, dict):
        weights = torch.load(os.fspath(weights), map_location="cpu")
    return PointNetExtractor(weights, device=device)


def pointnet_features(extractor: PointNetExtractor, samples_or_clouds: torch.Tensor) -> torch.Tensor:
    """``(B,1808)`` features of ``(B,5,H,W)`` samples [depth, x, y, z, reflectance] -- xyz zeroed where not ``0.5 < depth < 63``,
    all H W points kept, coordinates divided by 80, as evaluate.py prepares them, inside the kernel -- or of ``(B,N,3)`` clouds."""
    x = samples_or_clouds
    if x.ndim == 4 and x.shape[1] == 5:
        return extractor.extract(x, 0, x.shape[2] * x.shape[3])
    if x.ndim == 3 and x.shape[2] == 3:
        return extractor.extract(x, 1, x.shape[1])
    raise ValueError(f"expected (B,5,H,W) samples or (B,N,3) point clouds, got {tuple(x.shape)}")
