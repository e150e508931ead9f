"""An independent torch implementation of the reference's RangeNet (metrics/extractor/rangenet.py, eval mode) straight from the state
dict in the module layout: F.conv2d / F.conv_transpose2d / F.batch_norm / F.leaky_relu in whatever dtype and on whatever device the
state and the input have.  tests/golden/make_golden_rangenet.py asserts it equal to the reference module in fp64 (1e-12 relative)."""
import torch
import torch.nn.functional as F

BLOCKS = {21: (1, 1, 2, 2, 1), 53: (1, 2, 8, 8, 4)}
MEAN = (12.12, 10.88, 0.23, -1.04, 0.21)
STD = (12.32, 11.47, 6.91, 0.86, 0.16)


def cast(state, dtype, device="cpu"):
    return {k: v.to(device=device, dtype=dtype) for k, v in state.items() if v.is_floating_point()}


def preprocess(samples, mask=None, mean=MEAN, std=STD, lo=0.5, hi=63.0):
    """Samples.__getitem__ and Preprocess of the reference: ((img * mask) - mean) / std * mask, in the dtype of ``samples``."""
    if mask is None:
        mask = torch.logical_and(samples[:, [0]] > lo, samples[:, [0]] < hi)
    mask = mask.to(samples.dtype)
    m = torch.tensor(mean, dtype=samples.dtype, device=samples.device)[None, :, None, None]
    s = torch.tensor(std, dtype=samples.dtype, device=samples.device)[None, :, None, None]
    return (samples * mask - m) / s * mask


def forward(sd, x, backbone=53, trace=None):
    """(decoder map, logits) of the preprocessed (B,5,H,W) input; ``trace`` (a list) receives (name, pre-activation, activation)."""

    def cnl(name_conv, name_bn, h, **kw):
        if kw.pop("transposed", False):
            h = F.conv_transpose2d(h, sd[name_conv + ".weight"], sd[name_conv + ".bias"], **kw)
        else:
            h = F.conv2d(h, sd[name_conv + ".weight"], None, **kw)
        pre = F.batch_norm(h, sd[name_bn + ".running_mean"], sd[name_bn + ".running_var"], sd[name_bn + ".weight"], sd[name_bn + ".bias"],
                           False, 0.0, 1e-5)
        act = F.leaky_relu(pre, 0.1)
        if trace is not None:
            trace.append((name_conv, pre, act))
        return act

    def block(stage, n, h, **kw):
        h = cnl(f"{stage}.conv.0", f"{stage}.conv.1", h, **kw)
        for k in range(n):
            p = f"{stage}.residual_blocks.{k}.residual"
            h = h + cnl(f"{p}.1.0", f"{p}.1.1", cnl(f"{p}.0.0", f"{p}.0.1", h), padding=1)
        return h

    hs = [cnl("stem.0", "stem.1", x, padding=1)]
    for i, n in enumerate(BLOCKS[backbone], 1):
        hs.append(block(f"enc{i}", n, hs[-1], stride=(1, 2), padding=1))
    h = hs[5]
    for i in range(5, 0, -1):
        h = block(f"dec{i}", 1, h, transposed=True, stride=(1, 2), padding=(0, 1)) + hs[i - 1]
    return h, F.conv2d(h, sd["head.1.weight"], sd["head.1.bias"], padding=1)
