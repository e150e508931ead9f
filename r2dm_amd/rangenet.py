"""RangeNet-53 / -21 of the evaluation's FRD and of the completion demo's segmentation (the reference's
metrics/extractor/rangenet.py) as HIP kernels.

The network is a DarkNet encoder / decoder over the 5-channel range image [depth, x, y, z, reflectance], in eval mode:

- the stem, 3 x 3, 5 -> 32, behind the sensor normalisation ``(v - mean[c]) / std[c] * mask``;
- five encoder stages: a 3 x 3 convolution of stride (1, 2) that doubles the channels -- only the width halves -- and
  ``[1, 2, 8, 8, 4]`` (backbone 21: ``[1, 1, 2, 2, 1]``) residual blocks ``h + conv3x3(conv1x1(h))``;
- five decoder stages: a transposed 1 x 4 convolution of stride (1, 2) with a bias that halves the channels, one residual block,
  and the encoder's activation of the same width added: the last sum is the ``(B,32,H,W)`` decoder map of the FRD;
- the head, 3 x 3, 32 -> classes, with a bias: the logits whose argmax are the labels.

Every convolution but the head is followed by a BatchNorm (running statistics, eps 1e-5) and LeakyReLU(0.1); Dropout2d is the
identity.  The BatchNorms are folded into weights and biases on the host in fp64; every layer is one launch of ONE implicit-GEMM
kernel (csrc/rangenet.hip) on the fp16 matrix pipe with split fp32 operands (three products per multiply-add, fp32 accumulation),
the transposed convolution two launches, one per output-column parity.  Weights are packed and split once, at construction.  There
is no CPU or PyTorch fallback.  The extractor is built from a local weight file and downloads nothing; only the reference's hub
interface at the end of the module (``build_rangenet``) fetches a URL, through torch.hub's checkpoint cache.
"""
from __future__ import annotations

import io
import os
import random
import re
import tarfile
from typing import Dict, List, Optional, Tuple, Union

import torch

from . import _lib
from .metrics import MAX_DEPTH, MIN_DEPTH

BN_EPS = 1e-5
LRELU_SLOPE = 0.1
NUM_FEATURES = 4096  # the "lidargen" subsample of the decoder map
DECODER_CHANNELS = 32
RESIDUAL_BLOCKS = {21: (1, 1, 2, 2, 1), 53: (1, 2, 8, 8, 4)}
# Preprocess defaults of the reference: (range, x, y, z, remission)
DEFAULT_MEAN = (12.12, 10.88, 0.23, -1.04, 0.21)
DEFAULT_STD = (12.32, 11.47, 6.91, 0.86, 0.16)

_FLAG_INPUT, _FLAG_RANGE, _FLAG_WEIGHT = 1, 2, 4
_K1, _K3, _KDOWN, _KUP_EVEN, _KUP_ODD, _KSTEM = range(6)
_BN_LEAVES = ("weight", "bias", "running_mean", "running_var")


def _ch(i: int) -> int:
    return 32 << i


def _layers(backbone: int) -> List[Tuple[str, Optional[str], str]]:
    """(convolution, BatchNorm or None, kind) of every layer in forward order; kind in stem / down / up / 1x1 / 3x3 / head."""
    if backbone not in RESIDUAL_BLOCKS:
        raise ValueError(f"RangeNet backbone must be 21 or 53, got {backbone!r}")
    out = [("stem.0", "stem.1", "stem")]

    def blocks(stage, n):
        for k in range(n):
            pre = f"{stage}.residual_blocks.{k}.residual"
            out.append((f"{pre}.0.0", f"{pre}.0.1", "1x1"))
            out.append((f"{pre}.1.0", f"{pre}.1.1", "3x3"))

    for i, n in enumerate(RESIDUAL_BLOCKS[backbone], 1):
        out.append((f"enc{i}.conv.0", f"enc{i}.conv.1", "down"))
        blocks(f"enc{i}", n)
    for i in range(5, 0, -1):
        out.append((f"dec{i}.conv.0", f"dec{i}.conv.1", "up"))
        blocks(f"dec{i}", 1)
    out.append(("head.1", None, "head"))
    return out


def state_spec(backbone: int = 53, in_ch: int = 5, num_classes: int = 20) -> Dict[str, tuple]:
    """Key -> shape of the state dict in the reference's module layout, in its order, without the BatchNorms' ``num_batches_tracked``."""
    spec: Dict[str, tuple] = {}
    for conv, bn, kind in _layers(backbone):
        if kind == "stem":
            cout, shape = 32, (32, in_ch, 3, 3)
        elif kind == "head":
            cout, shape = num_classes, (num_classes, 32, 3, 3)
        else:
            i = int(conv[3])
            wide, narrow = _ch(i), _ch(i - 1)
            enc = conv.startswith("enc")
            if kind == "down":
                cout, shape = wide, (wide, narrow, 3, 3)
            elif kind == "up":
                cout, shape = narrow, (wide, narrow, 1, 4)  # (Cin, Cout, 1, 4)
            elif kind == "1x1":  # ResidualBlock(out_ch, in_ch, out_ch): out_ch -> in_ch -> out_ch
                cout, shape = (narrow, (narrow, wide, 1, 1)) if enc else (wide, (wide, narrow, 1, 1))
            else:
                cout, shape = (wide, (wide, narrow, 3, 3)) if enc else (narrow, (narrow, wide, 3, 3))
        spec[conv + ".weight"] = shape
        if kind in ("up", "head"):
            spec[conv + ".bias"] = (cout,)
        if bn is not None:
            for leaf in _BN_LEAVES:
                spec[f"{bn}.{leaf}"] = (cout,)
    return spec


def infer_arch(state: Dict[str, torch.Tensor]) -> Tuple[int, int, int]:
    """(backbone, in_ch, num_classes) of a state dict in the module layout."""
    for key in ("stem.0.weight", "head.1.bias"):
        if key not in state:
            raise KeyError(f"RangeNet state dict lacks {key!r}")
    backbone = 53 if "enc2.residual_blocks.1.residual.0.0.weight" in state else 21
    return backbone, int(state["stem.0.weight"].shape[1]), int(state["head.1.bias"].shape[0])


def check_state(state: Dict[str, torch.Tensor], backbone: int = 53, in_ch: int = 5, num_classes: int = 20) -> Dict[str, torch.Tensor]:
    """The tensors of ``state_spec`` as fp64 CPU tensors; KeyError / ValueError naming the first missing / mis-shaped / non-finite
    key.  ``num_batches_tracked`` entries are accepted and ignored."""
    out = {}
    for key, shape in state_spec(backbone, in_ch, num_classes).items():
        if key not in state:
            raise KeyError(f"RangeNet state dict lacks {key!r}")
        t = torch.as_tensor(state[key]).detach().cpu()
        if tuple(t.shape) != shape:
            raise ValueError(f"RangeNet state dict: {key!r} has shape {tuple(t.shape)}, expected {shape}")
        t = t.double()
        if not bool(torch.isfinite(t).all()):
            raise ValueError(f"RangeNet state dict: {key!r} holds a non-finite value")
        out[key] = t
    return out


def fold_state(state: Dict[str, torch.Tensor], backbone: int = 53, in_ch: int = 5, num_classes: int = 20) -> Dict[str, torch.Tensor]:
    """Eval-mode BatchNorms folded into the convolutions in front of them, in fp64, cast to fp32 at the end: ``{conv}.weight`` in the
    convolution's own layout -- (Cout,Cin,KH,KW), the transposed ones (Cin,Cout,1,4) -- and ``{conv}.bias`` (Cout,) for every layer."""
    sd = check_state(state, backbone, in_ch, num_classes)
    out = {}
    for conv, bn, kind in _layers(backbone):
        w = sd[conv + ".weight"]
        cout = w.shape[1] if kind == "up" else w.shape[0]
        b = sd.get(conv + ".bias", torch.zeros(cout, dtype=torch.float64))
        if bn is not None:
            s = sd[bn + ".weight"] / torch.sqrt(sd[bn + ".running_var"] + BN_EPS)
            w = w * (s[None, :, None, None] if kind == "up" else s[:, None, None, None])
            b = (b - sd[bn + ".running_mean"]) * s + sd[bn + ".bias"]
        out[conv + ".weight"], out[conv + ".bias"] = w.float().contiguous(), b.float().contiguous()
    return out


def subsample_indices(numel: int) -> List[int]:
    """The reference's ``random.seed(0); random.sample(range(numel), 4096)`` without touching the global generator."""
    if numel < NUM_FEATURES:
        raise ValueError(f'the "lidargen" feature takes {NUM_FEATURES} of the decoder map\'s 32 H W values, the map has only {numel}')
    return random.Random(0).sample(range(numel), NUM_FEATURES)


# ---- weight files ------------------------------------------------------------------------------------------------------------------
def module_key(name: str) -> str:
    """A parameter name of the official lidar-bonnetal files (``backbone``, ``segmentation_decoder``, ``segmentation_head``) in the
    module layout of ``state_spec``."""
    parts = name.split(".")
    leaf = parts[-1]
    if parts[0] == "1" and len(parts) == 2:
        return f"head.1.{leaf}"
    if parts[0] in ("conv1", "bn1") and len(parts) == 2:
        return f"stem.{0 if parts[0] == 'conv1' else 1}.{leaf}"
    if re.fullmatch(r"(enc|dec)[1-5]", parts[0]) and len(parts) == 3 and parts[1] in ("conv", "upconv", "bn"):
        return f"{parts[0]}.conv.{1 if parts[1] == 'bn' else 0}.{leaf}"
    if re.fullmatch(r"(enc|dec)[1-5]", parts[0]) and len(parts) == 4:
        block = re.fullmatch(r"residual(?:_(\d+))?", parts[1])
        sub = re.fullmatch(r"(conv|bn)([12])", parts[2])
        if block and sub:
            return f"{parts[0]}.residual_blocks.{int(block.group(1) or 0)}.residual.{int(sub.group(2)) - 1}.{0 if sub.group(1) == 'conv' else 1}.{leaf}"
    raise ValueError(f"unknown RangeNet parameter name {name!r}")


_CHANNELS = {"range": 1, "xyz": 3, "remission": 1, "mask": 1}


def load_weights(path: Union[str, os.PathLike]):
    """``(state, mean, std, backbone, num_classes)`` of a LOCAL weight file: the official ``darknet53*.tar.gz`` / ``darknet21.tar.gz``
    archive (members ``<arch>/backbone``, ``<arch>/segmentation_decoder``, ``<arch>/segmentation_head``, ``<arch>/arch_cfg.yaml``), or a
    ``.pth`` state dict in the module layout (mean and std are then the reference's Preprocess defaults)."""
    name = os.fspath(path)
    if "://" in name:
        raise ValueError(f"RangeNet weights {name!r}: nothing is downloaded here; fetch the archive yourself and give its local path")
    if not (name.endswith(".tar.gz") or name.endswith(".pth") or name.endswith(".pt")):
        raise ValueError(f"RangeNet weights {name!r}: expected the local path of a darknet*.tar.gz archive or of a .pth state dict "
                         "(a name such as 'SemanticKITTI_64x1024' would need a download, and nothing is downloaded here)")
    if not name.endswith(".tar.gz"):
        state = torch.load(name, map_location="cpu", weights_only=True)
        backbone, _, classes = infer_arch(state)
        return state, list(DEFAULT_MEAN), list(DEFAULT_STD), backbone, classes
    import yaml

    arch = os.path.basename(name)[:-len(".tar.gz")]
    state, cfg = {}, None
    with tarfile.open(name, "r:gz") as tar:
        members = set(tar.getnames())
        for member in (f"{arch}/backbone", f"{arch}/segmentation_decoder", f"{arch}/segmentation_head", f"{arch}/arch_cfg.yaml"):
            if member not in members:
                raise KeyError(f"RangeNet archive {name!r} lacks the member {member!r} (the members are looked up under the archive's "
                               "file name without .tar.gz, as the reference does: keep the official file name)")
            data = io.BytesIO(tar.extractfile(member).read())
            if member.endswith(".yaml"):
                cfg = yaml.safe_load(data)
                continue
            for key, value in torch.load(data, map_location="cpu", weights_only=True).items():
                new = module_key(key)
                if new in state:
                    raise ValueError(f"RangeNet archive {name!r}: {key!r} of {member!r} maps to {new!r}, which is already there")
                state[new] = value.cpu()
    in_ch = sum(_CHANNELS[k] for k, on in cfg["backbone"]["input_depth"].items() if on)
    sensor = cfg["dataset"]["sensor"]
    mean, std = list(sensor["img_means"][:in_ch]), list(sensor["img_stds"][:in_ch])
    return state, mean, std, int(cfg["backbone"]["extra"]["layers"]), int(state["head.1.bias"].shape[0])


# ---- the extractor -----------------------------------------------------------------------------------------------------------------
class _Layer:
    """One packed convolution on the device: fragments, the inverse weight scale and the folded bias."""

    def __init__(self, w: torch.Tensor, bias: torch.Tensor, device, flag):
        L = _lib.lib()
        cout, taps, cin = w.shape  # (Cout, taps, Cin)
        w = w.to(device).contiguous()
        self.cout, self.cin = cout, cin
        self.packed = torch.empty(L.r2dm_rangenet_packed_bytes(cout, cin, taps), dtype=torch.uint8, device=device)
        self.scale = torch.zeros(2, dtype=torch.float32, device=device)
        _lib.check(L.r2dm_rangenet_pack(_lib.ptr(w), cout, cin, taps, _lib.ptr(self.packed), _lib.ptr(self.scale), _lib.ptr(flag),
                                        _lib.stream_ptr(device)))
        self.bias = bias.to(device).contiguous()


def _taps3x3(w):  # (Cout,Cin,3,3) -> (Cout, 9, Cin), taps row-major
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], 9, w.shape[1])


class RangeNetExtractor:
    """``extract``: ``(B,5,H,W)`` fp32 samples on the GPU -> the FRD feature, the decoder map or the logits; ``segment``: labels."""

    max_batch = 8  # images per pass: bounds the activations held at once (about 60 MB per 64 x 1024 image)

    def __init__(self, state: Dict[str, torch.Tensor], mean=None, std=None, device="cuda"):
        self.backbone, in_ch, self.num_classes = infer_arch(state)
        if in_ch != 5:
            raise ValueError(f"RangeNet extractor: the network takes {in_ch} input channels; the samples have 5 [depth, x, y, z, reflectance]")
        folded = fold_state(state, self.backbone, in_ch, self.num_classes)  # (first: a bad state dict is reported without a GPU)
        mean, std = list(DEFAULT_MEAN if mean is None else mean), list(DEFAULT_STD if std is None else std)
        if len(mean) != 5 or len(std) != 5 or not all(s > 0 for s in std):
            raise ValueError("RangeNet extractor: mean and std must have 5 values, std positive")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.R2DMError(f"RangeNet extractor on {self.device}: r2dm_amd has no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._norm = torch.tensor(mean + std, dtype=torch.float32, device=self.device)
        self._indices: Dict[tuple, torch.Tensor] = {}
        self._layers: Dict[str, object] = {}
        with torch.cuda.device(self.device):
            for conv, _, kind in _layers(self.backbone):
                w, b = folded[conv + ".weight"], folded[conv + ".bias"]
                if kind == "up":  # (Cin,Cout,1,4): even columns in[j] w1 + in[j-1] w3, odd columns in[j] w2 + in[j+1] w0
                    t = w[:, :, 0, :].permute(1, 2, 0)  # (Cout, 4, Cin)
                    self._layers[conv] = (_Layer(t[:, [1, 3]], b, self.device, self._flag), _Layer(t[:, [2, 0]], b, self.device, self._flag))
                elif kind == "1x1":
                    self._layers[conv] = _Layer(w.reshape(w.shape[0], 1, w.shape[1]), b, self.device, self._flag)
                else:
                    self._layers[conv] = _Layer(_taps3x3(w), b, self.device, self._flag)
            if int(self._flag.item()) & _FLAG_WEIGHT:
                raise ValueError("RangeNet state dict holds a non-finite weight")

    # one launch: out = LeakyReLU(conv(x)) + add + add2
    def _conv(self, layer: _Layer, kind: int, x, B, H, Win, out, add=None, add2=None, mask=None, lo=0.0, hi=0.0, slope=LRELU_SLOPE):
        _lib.check(_lib.lib().r2dm_rangenet_conv(_lib.ptr(x), _lib.ptr(mask), _lib.ptr(self._norm) if kind == _KSTEM else None, lo, hi,
                                                 _lib.ptr(layer.packed), layer.scale.data_ptr() + 4, _lib.ptr(layer.bias), _lib.ptr(add), _lib.ptr(add2),
                                                 _lib.ptr(out), B, layer.cin, H, Win, layer.cout, kind, slope, _lib.ptr(self._flag),
                                                 _lib.stream_ptr(self.device)))
        return out

    def _forward(self, x, mask, lo, hi, want_logits: bool):
        B, _, H, W = x.shape
        new = lambda c, w: torch.empty(B, c, H, w, dtype=torch.float32, device=self.device)
        Ls = self._layers

        def residual(stage, n, h, w, skip=None):
            for k in range(n):
                pre = f"{stage}.residual_blocks.{k}.residual"
                mid = self._conv(Ls[f"{pre}.0.0"], _K1, h, B, H, w, new(Ls[f"{pre}.0.0"].cout, w))
                h = self._conv(Ls[f"{pre}.1.0"], _K3, mid, B, H, w, new(h.shape[1], w), add=h, add2=skip if k == n - 1 else None)
            return h

        h = self._conv(Ls["stem.0"], _KSTEM, x, B, H, W, new(32, W), mask=mask, lo=lo, hi=hi)
        skips, w = [h], W
        for i, n in enumerate(RESIDUAL_BLOCKS[self.backbone], 1):
            h = self._conv(Ls[f"enc{i}.conv.0"], _KDOWN, h, B, H, w, new(_ch(i), w // 2))
            w //= 2
            h = residual(f"enc{i}", n, h, w)
            skips.append(h)
        for i in range(5, 0, -1):
            even, odd = Ls[f"dec{i}.conv.0"]
            up = new(_ch(i - 1), 2 * w)
            self._conv(even, _KUP_EVEN, h, B, H, w, up)
            self._conv(odd, _KUP_ODD, h, B, H, w, up)
            w *= 2
            h = residual(f"dec{i}", 1, up, w, skip=skips[i - 1])
        if not want_logits:
            return h
        return self._conv(Ls["head.1"], _K3, h, B, H, W, new(self.num_classes, W), slope=1.0)

    def _check_input(self, samples, mask):
        if samples.ndim != 4 or samples.shape[1] != 5:
            raise ValueError(f"expected (B,5,H,W) samples [depth, x, y, z, reflectance], got {tuple(samples.shape)}")
        _lib.require_gpu(samples, "samples")
        if samples.device != self.device:
            raise ValueError(f"samples on {samples.device}, extractor on {self.device}")
        B, _, H, W = samples.shape
        if W % 32 or W < 32:
            raise ValueError(f"RangeNet halves the width five times: W must be a multiple of 32, got {W}")
        if mask is not None:
            if tuple(mask.shape) != (B, 1, H, W):
                raise ValueError(f"expected a (B,1,H,W) = {(B, 1, H, W)} mask, got {tuple(mask.shape)}")
            if mask.device != self.device:
                raise ValueError(f"mask on {mask.device}, extractor on {self.device}")
            mask = _lib.f32c(mask)
        return _lib.f32c(samples), mask

    @torch.no_grad()
    def extract(self, samples: torch.Tensor, mask: Optional[torch.Tensor] = None, feature: Optional[str] = "lidargen",
                image_min_depth: float = MIN_DEPTH, image_max_depth: float = MAX_DEPTH) -> torch.Tensor:
        """``feature`` "decoder": the (B,32,H,W) decoder map; "lidargen": (B,4096), the flattened map at the reference's fixed random
        indices; None: the (B,classes,H,W) logits.  ``mask`` (B,1,H,W) is BINARY (zeros and ones, as the reference's scripts build it):
        a pixel with 0 enters as zeros whatever its raw values, one with 1 as ``(v - mean) / std``; by default it is
        ``image_min_depth < depth < image_max_depth``, taken in the kernel."""
        if feature not in ("decoder", "lidargen", None):
            raise ValueError(f'feature must be "decoder", "lidargen" or None, got {feature!r}')
        samples, mask = self._check_input(samples, mask)
        B, _, H, W = samples.shape
        index = None
        if feature == "lidargen":
            if (H, W) not in self._indices:
                self._indices[(H, W)] = torch.tensor(subsample_indices(DECODER_CHANNELS * H * W), dtype=torch.int64, device=self.device)
            index = self._indices[(H, W)]
            out = torch.empty(B, NUM_FEATURES, dtype=torch.float32, device=self.device)
        else:
            out = torch.empty(B, DECODER_CHANNELS if feature == "decoder" else self.num_classes, H, W, dtype=torch.float32, device=self.device)
        if B == 0:
            return out
        with torch.cuda.device(self.device):
            self._flag.zero_()
            for k in range(0, B, self.max_batch):
                part = self._forward(samples[k:k + self.max_batch], None if mask is None else mask[k:k + self.max_batch],
                                     float(image_min_depth), float(image_max_depth), feature is None)
                out[k:k + self.max_batch] = part if index is None else part.flatten(1)[:, index]
            flag = int(self._flag.item())
        if flag & _FLAG_INPUT:
            raise ValueError("RangeNet extractor: an unmasked pixel of the samples has a non-finite value")
        if flag & _FLAG_RANGE:
            raise RuntimeError("RangeNet extractor: an activation left the fp16 operand range (65504) of the matrix-core layers; "
                               "the results of this call are not valid")
        return out

    @torch.no_grad()
    def segment(self, samples: torch.Tensor, mask: Optional[torch.Tensor] = None, image_min_depth: float = MIN_DEPTH,
                image_max_depth: float = MAX_DEPTH, postprocess=None) -> torch.Tensor:
        """int64 (B,1,H,W) labels: the argmax of the logits over the classes, the lowest index on a tie (as ``torch.argmax``).
        ``postprocess``: a ``postproc.KNN``, a ``postproc.CRFRNN`` or a tuple of them, every CRFRNN before every KNN -- a CRFRNN refines the
        logits (its ``xyz`` are the samples' ``xyz * mask``), the argmax follows, a KNN filters the labels over the depth, in which the
        masked pixels are -1 (the reference's invalid marker)."""
        from . import postproc

        crfs, knns = postproc.split_postprocess(postprocess)
        logits = self.extract(samples, mask, None, image_min_depth, image_max_depth)
        B, C, H, W = logits.shape
        if (crfs or knns) and B:
            depth = samples[:, [0]].to(torch.float32)
            m = torch.logical_and(depth > image_min_depth, depth < image_max_depth).float() if mask is None else mask.to(torch.float32)
            if crfs:
                xyz = samples[:, 1:4].to(torch.float32)
                xyz = torch.where(m != 0, xyz * m, torch.zeros_like(xyz))  # (the raw values of a masked pixel take no part)
            for crf in crfs:
                logits = crf(logits, xyz, m)
        labels = torch.empty(B, 1, H, W, dtype=torch.int64, device=self.device)
        if B:
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().r2dm_rangenet_argmax(_lib.ptr(logits), _lib.ptr(labels), B, C, H * W, _lib.stream_ptr(self.device)))
            if knns:
                depth = torch.where(m != 0, depth, torch.full_like(depth, -1.0))
                for knn in knns:
                    labels = knn(depth, labels)[:, None]
        return labels

    def __call__(self, samples: torch.Tensor) -> torch.Tensor:
        return self.extract(samples)


def pretrained_rangenet(weights: Union[str, os.PathLike, Dict[str, torch.Tensor]], device="cuda") -> RangeNetExtractor:
    """The extractor with the weights of ``weights``: a state dict in the module layout, or a local path ``load_weights`` accepts."""
    if isinstance(weights, dict):
        return RangeNetExtractor(weights, device=device)
    state, mean, std, _, _ = load_weights(weights)
    return RangeNetExtractor(state, mean, std, device=device)


# ---- the reference's hub interface: (model, preprocess) ------------------------------------------------------------------------------
OFFICIAL_ARCHIVES = {
    21: {"SemanticKITTI_64x2048": "darknet21"},
    53: {"SemanticKITTI_64x2048": "darknet53", "SemanticKITTI_64x1024": "darknet53-1024", "SemanticKITTI_64x512": "darknet53-512"},
}


def official_url(key: str) -> str:
    return f"http://www.ipb.uni-bonn.de/html/projects/bonnetal/lidar/semantic/models/{key}.tar.gz"


class Preprocess:
    """The reference's ``Preprocess``: ``preprocess(img, mask=None) = (img - mean) / std * mask`` in torch, the default mask
    ``img[:, [0]] > 0``."""

    def __init__(self, mean=None, std=None):
        mean, std = list(DEFAULT_MEAN if mean is None else mean), list(DEFAULT_STD if std is None else std)
        if len(mean) != len(std):
            raise ValueError("Preprocess: mean and std must have the same length")
        self.num_channels = len(mean)
        self.mean, self.std = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)

    def __call__(self, img: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        if img.ndim != 4 or img.shape[1] != self.num_channels:
            raise ValueError(f"Preprocess: expected a (B,{self.num_channels},H,W) image, got {tuple(img.shape)}")
        if mask is None:
            mask = (img[:, [0]] > 0).float()
        if mask.ndim != 4:
            raise ValueError(f"Preprocess: expected a (B,1,H,W) mask, got {tuple(mask.shape)}")
        mean, std = self.mean.to(img.device)[None, :, None, None], self.std.to(img.device)[None, :, None, None]
        return (img - mean) / std * mask


class PreprocessedRangeNet:
    """``model(x, feature=None)`` of the reference's hub entries: the extractor on ALREADY preprocessed input -- the stem gets the identity
    normalisation (mean 0, std 1) and a mask of ones -- returning the logits, the decoder map ("decoder") or the FRD feature ("lidargen")."""

    def __init__(self, state: Dict[str, torch.Tensor], device="cuda"):
        self.extractor = RangeNetExtractor(state, [0.0] * 5, [1.0] * 5, device=device)
        self.num_classes, self.backbone = self.extractor.num_classes, self.extractor.backbone

    @torch.no_grad()
    def __call__(self, img: torch.Tensor, feature: Optional[str] = None) -> torch.Tensor:
        _lib.require_gpu(img, "img")
        ones = torch.ones(img.shape[0], 1, *img.shape[2:], dtype=torch.float32, device=img.device)
        return self.extractor.extract(img, ones, feature)


def build_rangenet(url_or_file: Union[str, os.PathLike], device="cuda", progress: bool = True) -> Tuple[PreprocessedRangeNet, Preprocess]:
    """``(model, preprocess)`` from a local ``darknet*.tar.gz`` / ``.pth`` file, or from a URL through ``torch.hub``'s checkpoint cache (the
    only place of this module that may download, and only for a URL)."""
    name = os.fspath(url_or_file)
    if "://" in name:
        from urllib.parse import urlparse

        model_dir = os.path.join(torch.hub.get_dir(), "checkpoints")
        os.makedirs(model_dir, exist_ok=True)
        cached = os.path.join(model_dir, os.path.basename(urlparse(name).path))
        if not os.path.exists(cached):
            torch.hub.download_url_to_file(name, cached, None, progress=progress)
        name = cached
    state, mean, std, _, _ = load_weights(name)
    return PreprocessedRangeNet(state, device=device), Preprocess(mean, std)
