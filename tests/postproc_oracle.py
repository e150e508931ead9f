"""Torch restatements of the reference's two post-processors (metrics/extractor/rangenet.py:197-405), for the tests of
r2dm_amd.postproc and as the yardstick of scripts/bench_postproc.py.

``knn`` is written in the pinned order of include/r2dm_hip.h, ONE torch op per fp32 operation (eager torch fuses nothing): in fp32 it is
the kernel's expected bits, in fp64 -- with the weights built in fp64 -- the truth.  ``crf`` is the direct per-neighbour sum."""
import torch
import torch.nn.functional as F


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def knn_weight(kernel_size, sigma, dtype=torch.float32):
    """1 - the normalised Gaussian, (kh,kw), with the reference's expressions evaluated in ``dtype``."""
    kh, kw = _pair(kernel_size)
    hs, ws = torch.arange(kh) - kh // 2, torch.arange(kw) - kw // 2
    pdist = torch.stack(torch.meshgrid(hs, ws, indexing="ij"), dim=-1).pow(2).sum(dim=-1).to(dtype)
    kernel = torch.exp(-pdist / (2 * sigma**2))
    kernel = kernel / kernel.sum()
    return 1 - kernel


def knn_dist(depth, weight):
    """(B,K,H,W) dist_o(p) in ``weight``'s dtype: the accumulator starts from 0 and takes one term at a time, window offsets row-major."""
    dtype = weight.dtype
    kh, kw = weight.shape
    rh, rw = kh // 2, kw // 2
    d = depth[:, 0].to(dtype)
    B, H, W = d.shape
    a = torch.where(torch.isfinite(d), d, torch.full_like(d, -1.0))  # a depth that is not finite is read as -1
    n = torch.where(a < 0, torch.full_like(a, float("inf")), a)
    npad = F.pad(n, (2 * rw, 2 * rw, 2 * rh, 2 * rh))
    apad = F.pad(a, (rw, rw, rh, rh))
    inside = F.pad(torch.ones(B, H, W, dtype=torch.bool, device=d.device), (rw, rw, rh, rh))
    zero = torch.zeros((), dtype=dtype, device=d.device)
    out = []
    for oy in range(kh):
        for ox in range(kw):
            acc = torch.zeros(B, H, W, dtype=dtype, device=d.device)
            for qy in range(kh):
                for qx in range(kw):
                    jump = (npad[:, qy + oy:qy + oy + H, qx + ox:qx + ox + W] - apad[:, qy:qy + H, qx:qx + W]).abs()
                    term = weight[qy, qx] * jump
                    acc = acc + torch.where(inside[:, qy:qy + H, qx:qx + W], term, zero)
            out.append(acc)
    return torch.stack(out, dim=1)


def knn_vote(dist, label, kernel_size, k, cutoff, num_classes):
    """(B,H,W) int64 labels from (B,K,H,W) distances: the k smallest, ties to the lowest offset, a NaN the largest (a stable sort); the
    majority of the votes, the lowest class on a tie, 0 without votes."""
    kh, kw = _pair(kernel_size)
    rh, rw = kh // 2, kw // 2
    B, K, H, W = dist.shape
    lpad = F.pad(label.reshape(B, H, W).long(), (rw, rw, rh, rh))
    neigh = torch.stack([lpad[:, oy:oy + H, ox:ox + W] for oy in range(kh) for ox in range(kw)], dim=1)
    d_sorted, order = torch.sort(dist, dim=1, stable=True)
    d_top, l_top = d_sorted[:, :k], neigh.gather(1, order[:, :k])
    votes = torch.logical_and(l_top >= 0, l_top < num_classes)
    if cutoff > 0:
        votes = torch.logical_and(votes, ~(d_top > cutoff))
    bins = torch.zeros(B, num_classes + 1, H, W, dtype=torch.int64, device=dist.device)
    bins.scatter_add_(1, torch.where(votes, l_top, torch.full_like(l_top, num_classes)), torch.ones_like(l_top))
    return bins[:, :-1].argmax(dim=1)


def knn(depth, label, kernel_size=3, k=3, sigma=1.0, cutoff=1.0, num_classes=20, dtype=torch.float32):
    dist = knn_dist(depth, knn_weight(kernel_size, sigma, dtype).to(depth.device))
    return knn_vote(dist, label, kernel_size, k, cutoff, num_classes)


def knn_sure(dist64, dist32, k, cutoff):
    """(B,H,W) bool: the pixels whose vote cannot turn on fp32 roundoff, and the margin = 8 x the largest fp32 error of a finite dist.  Sure:
    the gap between the k-th and the (k+1)-th smallest fp64 dist exceeds the margin (two infinities count as a gap when there is a cutoff:
    both vote for nothing), and
    each of the k winners is further than the margin from the cutoff."""
    finite = torch.isfinite(dist64)
    assert torch.equal(finite, torch.isfinite(dist32))
    err = (dist32.double() - dist64)[finite].abs().max().item() if bool(finite.any()) else 0.0
    margin = 8 * err
    s = torch.sort(dist64, dim=1).values
    K = s.shape[1]
    if k < K:
        gap = s[:, k] - s[:, k - 1]
        sure = gap > margin
        if cutoff > 0:  # (without a cutoff they are two votes, and their order is a tie like any other)
            sure = torch.logical_or(sure, torch.logical_and(torch.isinf(s[:, k]), torch.isinf(s[:, k - 1])))
    else:
        sure = torch.ones_like(s[:, 0], dtype=torch.bool)
    if cutoff > 0:
        sure = torch.logical_and(sure, ((s[:, :k] - cutoff).abs() > margin).all(dim=1))
    return sure, margin


def crf(unary, xyz, mask, state, kernel_size=(3, 5), num_iters=3, dtype=torch.float64, trace=None):
    """CRFRNN.forward with the tensors of ``state`` (the reference module's state dict), every sum taken neighbour by neighbour.
    ``trace`` (a list) takes (weighted smoothness term, weighted appearance term) of every iteration."""
    kh, kw = _pair(kernel_size)
    rh, rw = kh // 2, kw // 2
    dev = unary.device
    sd = {k: v.to(dev, dtype) for k, v in state.items()}
    unary, xyz = unary.to(dtype), xyz.to(dtype)
    mask = (mask[:, None] if mask.ndim == 3 else mask).to(dtype)
    B, N, H, W = unary.shape
    pad = lambda t: F.pad(t, (rw, rw, rh, rh))
    offsets = [(oy, ox) for oy in range(kh) for ox in range(kw) if (oy, ox) != (rh, rw)]
    xpad = pad(xyz)
    beta = (2 * sd["theta_beta"] ** 2)[None, :, None, None]
    kbeta = []
    for oy, ox in offsets:
        d2 = (xpad[:, :, oy:oy + H, ox:ox + W] - xyz).pow(2).sum(dim=1, keepdim=True)
        kbeta.append(torch.exp(-d2 / beta))
    diag = lambda k: torch.stack([k[c, c] for c in range(N)])  # (N,kh,kw)
    kg, ka = diag(sd["kernel_gamma"]), diag(sd["kernel_alpha"])
    compat = sd["label_compatibility.weight"][:, :, 0, 0]
    Q = unary
    for _ in range(num_iters):
        S = torch.softmax(Q, dim=1)
        spad, mpad = pad(S), pad(S * mask)
        sg, sa, ap = torch.zeros_like(S), torch.zeros_like(S), torch.zeros_like(S)
        for (oy, ox), kb in zip(offsets, kbeta):
            s = spad[:, :, oy:oy + H, ox:ox + W]
            sg = sg + kg[None, :, oy, ox, None, None] * s
            sa = sa + ka[None, :, oy, ox, None, None] * s
            ap = ap + mpad[:, :, oy:oy + H, ox:ox + W] * kb
        smooth, appear = sd["weight_smoothness"] * sg, sd["weight_appearance"] * ((ap * mask) * sa)
        if trace is not None:
            trace.append((smooth, appear))
        Q = unary - torch.einsum("ij,bjhw->bihw", compat, smooth + appear)
    return Q
