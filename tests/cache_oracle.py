"""The feature cache's contract in torch ops, composed from the public functions of oracle/r2dm_oracle.py (``time_embedding``, ``fourier_features``,
``conv_ring``, ``block``): what a full forward leaves in the cache at depth d -- the output of up stage 7 - d, i.e. ``u_block{d + 1}`` -- and what a
shallow forward computes from it.  Float64 when its inputs are.  ``CachedNet`` is the stateful denoiser of a sampling loop under ``cache_interval``."""
import torch

from oracle import r2dm_oracle as O


def _stem(sd, cfg, x, cond):
    """-> (temb, in_conv's output): efficient_unet.py:275-282"""
    B = x.shape[0]
    if cond.ndim == 0:
        cond = cond[None].repeat_interleave(B, dim=0)
    temb = O.time_embedding(sd, cfg, cond.to(x))
    cenc = O.fourier_features(sd["coords"].to(x), sd["coords_encoding.freqs"], sd["coords_encoding.phase"])
    h = torch.cat([x, cenc.repeat_interleave(B, dim=0)], dim=1)
    return temb, O.conv_ring(h, sd["in_conv.weight"], sd["in_conv.bias"])


def _down(sd, cfg, h, temb, levels):
    """the skip tensors h1 .. h<levels> of the down path"""
    hs = []
    for lv in range(1, levels + 1):
        h = O.block(sd, f"d_block{lv}.", cfg, cfg.num_residual_blocks[lv - 1], h, temb)
        hs.append(h)
    return hs


def _up(sd, cfg, h, hs, temb, first):
    """up stages u_block<first> .. u_block1 from `h`, each over cat([h, skip])"""
    for lv in range(first, 0, -1):
        h = O.block(sd, f"u_block{lv}.", cfg, cfg.num_residual_blocks[lv - 1], torch.cat([h, hs[lv - 1]], 1), temb)
    return h


def cached_feature(sd, cfg, x, cond, depth):
    """The tensor a full forward at (x, cond) caches at ``depth``: the output of ``u_block{depth + 1}`` (after its FIR up-sampling and convolution)."""
    assert depth in (1, 2, 3)
    temb, h0 = _stem(sd, cfg, x, cond)
    hs = _down(sd, cfg, h0, temb, 4)
    h = O.block(sd, "u_block4.", cfg, cfg.num_residual_blocks[3], hs[3], temb)
    for lv in range(3, depth, -1):
        h = O.block(sd, f"u_block{lv}.", cfg, cfg.num_residual_blocks[lv - 1], torch.cat([h, hs[lv - 1]], 1), temb)
    return h


def shallow_forward(sd, cfg, x, cond, cached, depth):
    """The shallow forward at (x, cond): in_conv, ``d_block1 .. d_block{depth}``, then ``u_block{depth} .. u_block1`` from ``cached`` in place of
    ``u_block{depth + 1}``'s output, out_conv."""
    assert depth in (1, 2, 3)
    temb, h0 = _stem(sd, cfg, x, cond)
    hs = _down(sd, cfg, h0, temb, depth)
    h = _up(sd, cfg, cached.to(x), hs, temb, depth)
    return O.conv_ring(h, sd["out_conv.weight"], sd["out_conv.bias"])


class CachedNet:
    """``net(x, cond)`` for the oracle's sampling loops under a feature cache: call i is a full forward when ``i % interval == 0`` (it keeps
    ``cached_feature``), a shallow one otherwise."""

    def __init__(self, sd, cfg, interval, depth=1):
        self.sd, self.cfg, self.interval, self.depth = sd, cfg, interval, depth
        self.calls, self.cached = 0, None

    def __call__(self, x, cond):
        full = self.calls % self.interval == 0
        self.calls += 1
        if full:
            self.cached = cached_feature(self.sd, self.cfg, x, cond, self.depth)
            return O.unet_forward(self.sd, self.cfg, x, cond)
        return shallow_forward(self.sd, self.cfg, x, cond, self.cached, self.depth)
