"""The two post-processors of the reference's RangeNet module (metrics/extractor/rangenet.py:197-405) as HIP kernels: the kNN label
filter of RangeNet++ and the CRF-RNN refinement of SqueezeSeg.  Inference only.

- ``KNN``: every pixel takes the labels of the ``k`` pixels of its window that are nearest in depth -- the depth jumps weighed by an
  inverted Gaussian over the window -- and the majority wins; a neighbour further than ``cutoff`` does not vote.  One launch
  (csrc/postproc.hip: ``knn_vote_kernel``); the result is a function of the input bits (include/r2dm_hip.h pins every operation).
- ``CRFRNN``: ``num_iters`` mean-field iterations ``Q <- unary - compat . (w_s smooth_gamma(S) + w_a bilateral(S))``, ``S`` the softmax
  of ``Q``; one launch per iteration on two alternating buffers.  The reference's (B,N,K-1,HW) appearance kernel is never built: the
  kernel takes it from ``xyz``.  The smoothness kernels are per-class (diagonal), as the reference builds them.

Both pad with zeros at every image edge, the azimuth seam included, as the reference does.  There is no CPU or PyTorch fallback.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple, Union

import torch

from . import _lib

MAX_WINDOW, MAX_TOP, MAX_CLASSES = 7, 8, 32
_FLAG_LABEL = 1


def _pair(v) -> Tuple[int, int]:
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"kernel_size must be an int or a pair, got {v!r}")
        return int(v[0]), int(v[1])
    return int(v), int(v)


def _check_window(what: str, kernel_size) -> Tuple[int, int]:
    kh, kw = _pair(kernel_size)
    if kh < 1 or kw < 1 or kh % 2 == 0 or kw % 2 == 0:
        raise ValueError(f"{what}: the window sides must be odd, got {kh} x {kw}")
    if kh > MAX_WINDOW or kw > MAX_WINDOW:
        raise ValueError(f"{what}: the window sides must be at most {MAX_WINDOW}, got {kh} x {kw}")
    return kh, kw


def _check_classes(what: str, num_classes: int) -> int:
    num_classes = int(num_classes)
    if not 1 <= num_classes <= MAX_CLASSES:
        raise ValueError(f"{what}: 1 to {MAX_CLASSES} classes, got {num_classes}")
    return num_classes


def _window_pdist(kh: int, kw: int) -> torch.Tensor:
    """Squared pixel distance to the window's centre, (kh,kw) int64: the reference's expressions."""
    hs = torch.arange(kh) - kh // 2
    ws = torch.arange(kw) - kw // 2
    coord = torch.meshgrid(hs, ws, indexing="ij")
    return torch.stack(coord, dim=-1).pow(2).sum(dim=-1)


def gaussian_kernel(kernel_size, sigma: float) -> torch.Tensor:
    """The reference's ``_get_gaussian_kernel``: (kh,kw) fp32, normalised to sum 1."""
    kh, kw = _pair(kernel_size)
    kernel = torch.exp(-_window_pdist(kh, kw) / (2 * sigma**2))
    kernel /= kernel.sum()
    return kernel


def smoothness_kernel(num_classes: int, kernel_size, theta: torch.Tensor) -> torch.Tensor:
    """The reference's ``CRFRNN.get_smoothness_kernel``: (N,N,kh,kw) fp32, class c's Gaussian of width ``theta[c]`` with a zero centre on
    the diagonal, zeros elsewhere."""
    kh, kw = _pair(kernel_size)
    pdist = _window_pdist(kh, kw)
    kernel = torch.zeros(num_classes, num_classes, kh, kw)
    for c in range(num_classes):
        _kernel = torch.exp(-pdist / (2 * theta[c] ** 2))
        _kernel[kh // 2, kw // 2] = 0
        kernel[c, c] = _kernel
    return kernel


def _ntuple(v, n: int, what: str) -> torch.Tensor:
    if isinstance(v, (tuple, list)):
        if len(v) != n:
            raise ValueError(f"{what} must be a number or {n} of them, got {len(v)}")
        return torch.tensor(tuple(v))
    return torch.tensor((v,) * n)


class KNN:
    """``KNN(num_classes, ...)(depth, label) -> (B,H,W) int64``: the reference's ``kNN`` (signature and defaults)."""

    max_batch = 4096  # images per launch (the grid's third dimension holds 65535)

    def __init__(self, num_classes: int, k: int = 3, kernel_size=3, sigma: float = 1.0, cutoff: float = 1.0):
        self.num_classes = _check_classes("KNN", num_classes)
        self.kernel_size = _check_window("KNN", kernel_size)
        self.k = int(k)
        K = self.kernel_size[0] * self.kernel_size[1]
        if not 1 <= self.k <= min(K, MAX_TOP):
            raise ValueError(f"KNN: k must be in [1, {min(K, MAX_TOP)}] for a {self.kernel_size[0]} x {self.kernel_size[1]} window, got {k}")
        if not sigma > 0:
            raise ValueError(f"KNN: sigma must be positive, got {sigma}")
        self.sigma, self.cutoff = sigma, float(cutoff)
        self.dist_kernel = (1 - gaussian_kernel(self.kernel_size, self.sigma)).float().contiguous()  # (kh,kw): penalises far pixels
        self._device: Dict[torch.device, Tuple[torch.Tensor, torch.Tensor]] = {}

    def _tables(self, device):
        if device not in self._device:
            self._device[device] = (self.dist_kernel.to(device), torch.zeros(1, dtype=torch.int32, device=device))
        return self._device[device]

    @torch.no_grad()
    def __call__(self, depth: torch.Tensor, label: torch.Tensor) -> torch.Tensor:
        if depth.ndim != 4 or depth.shape[1] != 1:
            raise ValueError(f"KNN: expected a (B,1,H,W) depth, got {tuple(depth.shape)}")
        B, _, H, W = depth.shape
        if label.ndim == 4 and label.shape[1] == 1:
            label = label[:, 0]
        if tuple(label.shape) != (B, H, W):
            raise ValueError(f"KNN: expected (B,H,W) or (B,1,H,W) = {(B, H, W)} labels, got {tuple(label.shape)}")
        _lib.require_gpu(depth, "depth")
        _lib.require_gpu(label, "label")
        if label.device != depth.device:
            raise ValueError(f"KNN: label on {label.device}, depth on {depth.device}")
        depth, label = _lib.f32c(depth), label.detach().to(torch.int64).contiguous()
        out = torch.empty(B, H, W, dtype=torch.int64, device=depth.device)
        if B == 0:
            return out
        kh, kw = self.kernel_size
        with torch.cuda.device(depth.device):
            weight, flag = self._tables(depth.device)
            flag.zero_()
            for s in range(0, B, self.max_batch):
                n = min(self.max_batch, B - s)
                _lib.check(_lib.lib().r2dm_knn_vote(_lib.ptr(depth[s:s + n]), _lib.ptr(label[s:s + n]), _lib.ptr(weight), _lib.ptr(out[s:s + n]), n, H,
                                                    W, kh, kw, self.k, self.num_classes, self.cutoff, _lib.ptr(flag), _lib.stream_ptr(depth.device)))
            bad = int(flag.item())
        if bad & _FLAG_LABEL:
            raise ValueError(f"KNN: a label is outside [0, {self.num_classes})")
        return out


# the reference module's state dict: key -> shape, in its order
def crf_state_spec(num_classes: int, kernel_size=(3, 5)) -> Dict[str, tuple]:
    N, (kh, kw) = num_classes, _pair(kernel_size)
    return {"weight_appearance": (1, N, 1, 1), "weight_smoothness": (1, N, 1, 1), "theta_gamma": (N,), "theta_alpha": (N,), "theta_beta": (N,),
            "kernel_gamma": (N, N, kh, kw), "kernel_alpha": (N, N, kh, kw), "label_compatibility.weight": (N, N, 1, 1)}


class CRFRNN:
    """``CRFRNN(num_classes, ...)(unary, xyz, mask) -> (B,N,H,W) fp32``: the reference's ``CRFRNN`` in eval mode (signature and defaults;
    ``state_dict`` / ``load_state_dict`` in its keys and shapes)."""

    max_batch = 64  # images per pass: bounds the two work buffers (5 MB per 20-class 64 x 1024 image)

    def __init__(self, num_classes: int, kernel_size=(3, 5), init_weight_smoothness: float = 0.02, init_weight_appearance: float = 0.1,
                 theta_gamma=0.9, theta_alpha=0.9, theta_beta=0.015, num_iters: int = 3):
        N = self.num_classes = _check_classes("CRFRNN", num_classes)
        self.kernel_size = _check_window("CRFRNN", kernel_size)
        self.num_iters = int(num_iters)
        if self.num_iters < 0:
            raise ValueError(f"CRFRNN: num_iters must not be negative, got {num_iters}")
        self._state = {
            "weight_appearance": torch.ones(1, N, 1, 1) * init_weight_appearance,
            "weight_smoothness": torch.ones(1, N, 1, 1) * init_weight_smoothness,
            "theta_gamma": _ntuple(theta_gamma, N, "theta_gamma"),
            "theta_alpha": _ntuple(theta_alpha, N, "theta_alpha"),
            "theta_beta": _ntuple(theta_beta, N, "theta_beta"),
        }
        self._state["kernel_gamma"] = smoothness_kernel(N, self.kernel_size, self._state["theta_gamma"])
        self._state["kernel_alpha"] = smoothness_kernel(N, self.kernel_size, self._state["theta_alpha"])
        self._state["label_compatibility.weight"] = 1 - torch.eye(N)[..., None, None]  # Potts: [i != j]
        self._pack()

    def _pack(self):
        """The kernel's parameter block: gamma | alpha diagonals (N,kh,kw), the two weights, 2 theta_beta^2, the compatibility matrix."""
        sd, N = self._state, self.num_classes
        kh, kw = self.kernel_size
        diag = lambda k: torch.stack([k[c, c] for c in range(N)])
        for key in ("kernel_gamma", "kernel_alpha"):
            k = sd[key]
            off = k.clone()
            for c in range(N):
                off[c, c] = 0
            if bool((off != 0).any()):
                raise ValueError(f"CRFRNN: {key} has a non-zero entry off the class diagonal; only per-class smoothness kernels are built")
            if bool((diag(k)[:, kh // 2, kw // 2] != 0).any()):
                raise ValueError(f"CRFRNN: {key} has a non-zero centre; the centre of the window is not a neighbour")
        theta_beta = sd["theta_beta"].float()
        if not bool((theta_beta != 0).all()):
            raise ValueError("CRFRNN: theta_beta must not be zero")
        parts = [diag(sd["kernel_gamma"]), diag(sd["kernel_alpha"]), sd["weight_smoothness"], sd["weight_appearance"], 2 * theta_beta**2,
                 sd["label_compatibility.weight"]]
        params = torch.cat([p.float().reshape(-1) for p in parts]).contiguous()
        if not bool(torch.isfinite(params).all()):
            raise ValueError("CRFRNN: a parameter is not finite")
        self._params = params
        self._uniform_beta = bool((theta_beta == theta_beta[0]).all())
        self._device: Dict[torch.device, torch.Tensor] = {}

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {k: self._state[k].clone() for k in crf_state_spec(self.num_classes, self.kernel_size)}

    def load_state_dict(self, state: Dict[str, torch.Tensor]):
        new = {}
        for key, shape in crf_state_spec(self.num_classes, self.kernel_size).items():
            if key not in state:
                raise KeyError(f"CRFRNN state dict lacks {key!r}")
            t = torch.as_tensor(state[key]).detach().cpu().float()
            if tuple(t.shape) != shape:
                raise ValueError(f"CRFRNN state dict: {key!r} has shape {tuple(t.shape)}, expected {shape}")
            new[key] = t.clone()
        old, self._state = self._state, new
        try:
            self._pack()
        except ValueError:
            self._state = old
            raise
        return self

    @torch.no_grad()
    def __call__(self, unary: torch.Tensor, xyz: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        N = self.num_classes
        if unary.ndim != 4 or unary.shape[1] != N:
            raise ValueError(f"CRFRNN: expected a (B,{N},H,W) unary, got {tuple(unary.shape)}")
        B, _, H, W = unary.shape
        if tuple(xyz.shape) != (B, 3, H, W):
            raise ValueError(f"CRFRNN: expected a (B,3,H,W) = {(B, 3, H, W)} xyz, got {tuple(xyz.shape)}")
        if mask.ndim == 3:
            mask = mask[:, None]
        if tuple(mask.shape) != (B, 1, H, W):
            raise ValueError(f"CRFRNN: expected a (B,H,W) or (B,1,H,W) = {(B, 1, H, W)} mask, got {tuple(mask.shape)}")
        for t, what in ((unary, "unary"), (xyz, "xyz"), (mask, "mask")):
            _lib.require_gpu(t, what)
            if t.device != unary.device:
                raise ValueError(f"CRFRNN: {what} on {t.device}, unary on {unary.device}")
        unary, xyz, mask = _lib.f32c(unary), _lib.f32c(xyz), _lib.f32c(mask)
        if B == 0 or self.num_iters == 0:
            return unary.clone()
        device = unary.device
        if device not in self._device:
            self._device[device] = self._params.to(device)
        params = self._device[device]
        out = torch.empty_like(unary)
        kh, kw = self.kernel_size
        with torch.cuda.device(device):
            n = min(self.max_batch, B)
            work = [torch.empty(n, N, H, W, dtype=torch.float32, device=device) for _ in range(min(2, self.num_iters - 1))]
            for s in range(0, B, self.max_batch):
                n = min(self.max_batch, B - s)
                u, dst = unary[s:s + n], out[s:s + n]
                q = u
                for it in range(self.num_iters):
                    nxt = dst if it == self.num_iters - 1 else work[it % 2][:n]
                    _lib.check(_lib.lib().r2dm_crf_iter(_lib.ptr(q), _lib.ptr(u), _lib.ptr(xyz[s:s + n]), _lib.ptr(mask[s:s + n]), _lib.ptr(params),
                                                        _lib.ptr(nxt), n, N, H, W, kh, kw, int(self._uniform_beta), _lib.stream_ptr(device)))
                    q = nxt
        return out


PostProcess = Union[KNN, CRFRNN, Sequence[Union[KNN, CRFRNN]]]


def split_postprocess(postprocess) -> Tuple[Tuple[CRFRNN, ...], Tuple[KNN, ...]]:
    """``postprocess`` of ``RangeNetExtractor.segment`` as (the CRF-RNNs, the kNNs): the former refine the logits, the latter the labels, so
    in a tuple every CRF-RNN comes before every kNN."""
    if postprocess is None:
        return (), ()
    steps = tuple(postprocess) if isinstance(postprocess, (tuple, list)) else (postprocess,)
    for step in steps:
        if not isinstance(step, (KNN, CRFRNN)):
            raise TypeError(f"postprocess takes a KNN, a CRFRNN or a tuple of them, got {type(step).__name__}")
    crfs = tuple(s for s in steps if isinstance(s, CRFRNN))
    knns = tuple(s for s in steps if isinstance(s, KNN))
    if steps != crfs + knns:
        raise ValueError("postprocess: a CRFRNN refines the logits and a KNN the labels, so every CRFRNN comes before every KNN")
    return crfs, knns
