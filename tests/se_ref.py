"""Float64 restatement of the SE bottleneck in eval mode and of its BatchNorm fold, written
from the formulas (not from the reference's modules), for the SE tests and their goldens.

With x (N, C, H, W) the activated output of a Conv2dBlock and eps = 1e-5:

    h1  = relu(bn1(conv1(x)))          conv1: 1x1, no bias
    h2  = relu(bn2(conv2(h1)))         conv2: 3x3, zero padding 1, no bias
    u   = bn3(conv3(h2))               conv3: 1x1, no bias
    p   = mean over H, W of u
    g   = sigmoid(W_b relu(W_a p))     W_a = se.fc.0.weight (C//16, C), W_b = se.fc.2.weight
    out = relu(g * u + x)

bn(y) = (y - running_mean) / sqrt(running_var + eps) * weight + bias per channel.
"""
import numpy as np
import torch
import torch.nn.functional as F

from ld_ref import _d, key_table  # noqa: F401  (one definition each, shared)

EPS = 1e-5
PREFIX = "blk.attention_block."  # rpst.synth's SE rules apply to keys holding '.attention_block.'


def golden_config(g, i):
    """The MultiScaleAdaINRPNet config of network case i of tests/golden/se.npz."""
    from helpers import multiscale_config
    return dict(multiscale_config(int(g[f"net{i}_hidden"]), int(g[f"net{i}_blocks"]), 0),
                attention="se", use_mask=bool(g[f"net{i}_use_mask"]))


def batchnorm(y, sd, name):
    g, b = _d(sd[name + ".weight"]), _d(sd[name + ".bias"])
    m, v = _d(sd[name + ".running_mean"]), _d(sd[name + ".running_var"])
    return (y - m.view(1, -1, 1, 1)) / torch.sqrt(v.view(1, -1, 1, 1) + EPS) * g.view(1, -1, 1, 1) \
        + b.view(1, -1, 1, 1)


def se_block(x, sd, prefix=""):
    """-> (out (N, C, H, W), gate (N, C, 1, 1)), float64; sd: the block's state_dict (tensors
    or arrays), its keys under `prefix`."""
    sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    x = _d(x)
    h1 = torch.relu(batchnorm(F.conv2d(x, _d(sd["conv1.weight"])), sd, "bn1"))
    h2 = torch.relu(batchnorm(F.conv2d(h1, _d(sd["conv2.weight"]), padding=1), sd, "bn2"))
    u = batchnorm(F.conv2d(h2, _d(sd["conv3.weight"])), sd, "bn3")
    p = u.mean(dim=(2, 3))
    z = torch.relu(p @ _d(sd["se.fc.0.weight"]).t())
    g = torch.sigmoid(z @ _d(sd["se.fc.2.weight"]).t())
    out = torch.relu(g[:, :, None, None] * u + x)
    return out, g[:, :, None, None]


def fold(w, sd, name):
    """BatchNorm `name` folded into the bias-free conv weight w before it, float64:
    w' = w * s, b' = bias - running_mean * s per output channel, s = weight / sqrt(var + eps)."""
    s = _d(sd[name + ".weight"]) / torch.sqrt(_d(sd[name + ".running_var"]) + EPS)
    return _d(w) * s.view(-1, 1, 1, 1), _d(sd[name + ".bias"]) - _d(sd[name + ".running_mean"]) * s


def se_block_folded(x, sd):
    """se_block with every BatchNorm folded first (the form the kernels run), the gate from
    the pooled h2: mean(conv3'(h2)) = conv3'(mean(h2)) for a 1x1 conv."""
    x = _d(x)
    w1, b1 = fold(sd["conv1.weight"], sd, "bn1")
    w2, b2 = fold(sd["conv2.weight"], sd, "bn2")
    w3, b3 = fold(sd["conv3.weight"], sd, "bn3")
    h1 = torch.relu(F.conv2d(x, w1, b1))
    h2 = torch.relu(F.conv2d(h1, w2, b2, padding=1))
    p = h2.mean(dim=(2, 3)) @ w3[:, :, 0, 0].t() + b3
    g = torch.sigmoid(torch.relu(p @ _d(sd["se.fc.0.weight"]).t()) @ _d(sd["se.fc.2.weight"]).t())
    out = torch.relu(g[:, :, None, None] * F.conv2d(h2, w3, b3) + x)
    return out, g[:, :, None, None]


def module_input(seed, shape):
    """The module goldens' input: LeakyReLU(0.2) of uniform [-1, 1) values (what a Conv2dBlock
    hands its attention block), image n (1-based) scaled by 2^(n-1) so the gates differ
    between the images of a batch."""
    from rpst import synth
    u = 2.0 * synth.uniform01(seed, "sefeat", int(np.prod(shape))).reshape(shape) - 1.0
    x = np.where(u > 0, u, 0.2 * u)
    x *= (2.0 ** np.arange(shape[0], dtype=np.float64)).reshape(-1, 1, 1, 1)
    return x.astype(np.float32)


def synth_block_(block, seed):
    """Synthetic weights for a stand-alone SEBottleneck by rpst.synth's attention rules (its
    keys are generated under PREFIX, as if it sat in a Conv2dBlock) -> checksum."""
    from rpst import synth
    shapes = [(PREFIX + k, tuple(v.shape)) for k, v in block.state_dict().items()]
    new = synth.synth_state_dict(shapes, seed)
    block.load_state_dict({k[len(PREFIX):]: torch.from_numpy(v) for k, v in new.items()})
    return np.array(synth.checksum(new))
