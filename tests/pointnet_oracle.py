"""Plain functional restatement of the FPD's PointNet (SpareNet's classifier, 16 classes, eval mode) in torch, in the dtype of the
input (fp64 for the oracles): the yardstick of tests/test_pointnet_cpu.py and tests/test_hip_pointnet.py.  No nn.Module, no folding:
every BatchNorm is applied as written, (x - mean) / sqrt(var + eps) * weight + bias."""
import torch

EPS = 1e-5


def _bn(sd, name, x):
    """x (B,C) or (B,C,N)"""
    shape = (1, -1) + (1,) * (x.ndim - 2)
    g = lambda leaf: sd[f"{name}.{leaf}"].to(x).reshape(shape)
    return (x - g("running_mean")) / torch.sqrt(g("running_var") + EPS) * g("weight") + g("bias")


def _conv(sd, name, x):
    w = sd[name + ".weight"].to(x)
    return torch.einsum("oc,bcn->bon", w.reshape(w.shape[0], -1), x) + sd[name + ".bias"].to(x)[None, :, None]


def _fc(sd, name, x):
    return x @ sd[name + ".weight"].to(x).T + sd[name + ".bias"].to(x)


def transform(sd, x):
    """feat.stn: (B,3,N) -> (B,3,3)"""
    p = "feat.stn."
    h = torch.relu(_bn(sd, p + "bn1", _conv(sd, p + "conv1", x)))
    h = torch.relu(_bn(sd, p + "bn2", _conv(sd, p + "conv2", h)))
    h = torch.relu(_bn(sd, p + "bn3", _conv(sd, p + "conv3", h)))
    h = h.amax(dim=2)
    h = torch.relu(_bn(sd, p + "bn4", _fc(sd, p + "fc1", h)))
    h = torch.relu(_bn(sd, p + "bn5", _fc(sd, p + "fc2", h)))
    return _fc(sd, p + "fc3", h).reshape(-1, 3, 3) + torch.eye(3).to(x)


def features(sd, clouds, return_trans=False):
    """(B,3,N) clouds -> (B,1808) = cat(x1, x2, x3, x4)"""
    trans = transform(sd, clouds)
    x = torch.bmm(clouds.transpose(1, 2), trans).transpose(1, 2)
    h = torch.relu(_bn(sd, "feat.bn1", _conv(sd, "feat.conv1", x)))
    h = torch.relu(_bn(sd, "feat.bn2", _conv(sd, "feat.conv2", h)))
    x1 = _bn(sd, "feat.bn3", _conv(sd, "feat.conv3", h)).amax(dim=2)
    x2 = torch.relu(_bn(sd, "bn1", _fc(sd, "fc1", x1)))
    x3 = torch.relu(_bn(sd, "bn2", _fc(sd, "fc2", x2)))
    x4 = _fc(sd, "fc3", x3)
    out = torch.cat([x1, x2, x3, x4], dim=1)
    return (out, trans) if return_trans else out


def folded_features(folded, clouds):
    """The same network from r2dm_amd.pointnet.fold_state's folded layers ({layer}.weight (cout,cin), {layer}.bias), in the
    dtype of ``clouds``."""
    w = lambda n: folded[n + ".weight"].to(clouds)
    b = lambda n: folded[n + ".bias"].to(clouds)
    conv = lambda n, x: torch.einsum("oc,bcn->bon", w(n), x) + b(n)[None, :, None]
    fc = lambda n, x: x @ w(n).T + b(n)
    p = "feat.stn."
    h = torch.relu(conv(p + "conv3", torch.relu(conv(p + "conv2", torch.relu(conv(p + "conv1", clouds)))))).amax(dim=2)
    trans = fc(p + "fc3", torch.relu(fc(p + "fc2", torch.relu(fc(p + "fc1", h))))).reshape(-1, 3, 3) + torch.eye(3).to(clouds)
    x = torch.bmm(clouds.transpose(1, 2), trans).transpose(1, 2)
    x1 = conv("feat.conv3", torch.relu(conv("feat.conv2", torch.relu(conv("feat.conv1", x))))).amax(dim=2)
    x2 = torch.relu(fc("fc1", x1))
    x3 = torch.relu(fc("fc2", x2))
    return torch.cat([x1, x2, x3, fc("fc3", x3)], dim=1)


def sample_clouds(images, min_depth=0.5, max_depth=63.0, divisor=80.0):
    """evaluate.py's preparation of (B,5,H,W) samples, in fp32: xyz * (min < depth < max), flattened to (B,3,H W), / 80."""
    depth = images[:, [0]]
    mask = torch.logical_and(depth > min_depth, depth < max_depth).float()
    return (images[:, 1:4] * mask).flatten(2) / divisor
