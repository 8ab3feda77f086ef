"""Float64 restatement of LDMSAdaINRPNet (`network: ld_adain`) inference, written from the
formulas (not from the reference's modules), for the ld_adain tests and their goldens.

With h = hidden_dim, L = ld_layer_num, eps = 1e-5 and, per Conv2dBlock B (kernel k, padding p),

    B(x) = lrelu(inc_m(... inc_1(conv_k(reflect_pad_p(x))))),  lrelu(v) = v > 0 ? v : 0.2 v,

with the m = inception_num 1x1 convs inc_j and the activation once at the end:

    level_0 = cat([small_0(x), big_0(x)])            both 3x3 pad 1, 3 -> h
    level_i = cat([small_i(level_{i-1}), big_i(level_{i-1})])
                                                     small 3x3 pad 1, big 7x7 pad 3, both
                                                     h 2^i -> h 2^i, so level_i has h 2^(i+1)
    AdaIN(a, b) = (a - mean(a)) / std(a) * std(b) + mean(b) per (n, c),
                  std = sqrt(unbiased variance + eps)
    y = dec_0(AdaIN(c_{L-1}, s_{L-1}))
    y = dec_j(y + AdaIN(y, s_{L-1-j}))               j = 1 .. L-1: the content statistics are
                                                     y's own
    masked: AdaIN(c_{L-1}, s_{L-1}) and every y + AdaIN(...) term become the per-label AdaIN
    of (c_i, s_i) (tests/masked_ref.py), label maps at the image size.
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
CASES = [  # (hidden, layers, inception, shape, use_mask, model seed)
    (4, 3, 0, (2, 3, 24, 40), False, 81),
    (8, 3, 1, (1, 3, 17, 33), False, 82),
    (16, 5, 0, (1, 3, 16, 20), False, 83),
    (4, 3, 0, (2, 3, 24, 40), True, 81),
]


def config(hidden, layers, inception=0, use_mask=False):
    """An ld_adain config: the MultiScale keys plus ld_layer_num, enc_stack_way 'NONE' (the
    parent constructor then builds no stack of its own)."""
    return {"rp_blocks": layers, "hidden_dim": hidden, "content_weight": 1.0,
            "style_weight": 10.0, "resume": False, "use_mask": use_mask, "shuffle": False,
            "shuffle_layers": 1, "sort": False, "stylized_layers": layers,
            "enc_stack_way": "NONE", "inception_num": inception, "attention": "none",
            "ld_layer_num": layers}


def golden_config(g, i):
    """The config of case i of tests/golden/ld.npz."""
    return config(int(g[f"net{i}_hidden"]), int(g[f"net{i}_layers"]), int(g[f"net{i}_inception"]),
                  bool(g[f"net{i}_use_mask"]))


def _d(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(dtype)


def conv_pad(x, w, b, pad_mode="reflect"):
    """conv_k(pad_{k//2}(x)) + b in x's dtype; pad_mode 'reflect' or 'constant' (zeros)."""
    p = w.shape[-1] // 2
    if p:
        x = F.pad(x, (p,) * 4, mode=pad_mode)
    return F.conv2d(x, w, b)


def rp64(sd, dtype=torch.float64):
    """The rp_enc* / rp_dec* entries of a state_dict as float64 tensors (or of `dtype`; the
    frozen VGG is not part of inference)."""
    return {k: _d(v, dtype) for k, v in sd.items() if k.startswith("rp_")}


def block(x, sd, prefix, pad_mode="reflect"):
    """A Conv2dBlock from its state_dict entries under `prefix`, in x's dtype (sd in the same
    dtype): pad k // 2, conv, the 1x1 inception convs, LeakyReLU(0.2) once at the end."""
    y = conv_pad(x, sd[prefix + "conv.weight"], sd[prefix + "conv.bias"], pad_mode)
    j = 0
    while f"{prefix}inception.{j}.0.weight" in sd:
        y = F.conv2d(y, sd[f"{prefix}inception.{j}.0.weight"], sd[f"{prefix}inception.{j}.0.bias"])
        j += 1
    return torch.where(y > 0, y, 0.2 * y)


def mean_std(x):
    n, c = x.shape[:2]
    v = x.reshape(n, c, -1)
    return (v.mean(dim=2).view(n, c, 1, 1),
            torch.sqrt(v.var(dim=2, unbiased=True) + EPS).view(n, c, 1, 1))


def adain(a, b):
    ma, sa = mean_std(a)
    mb, sb = mean_std(b)
    return (a - ma) / sa * sb + mb


def levels(x, sd, layers):
    """The encoder levels of x, in x's dtype (sd in the same dtype)."""
    feats = []
    for i in range(layers):
        x = torch.cat([block(x, sd, f"rp_enc{i}_small_revf."),
                       block(x, sd, f"rp_enc{i}_big_revf.")], dim=1)
        feats.append(x)
    return feats


def encode(x, sd, layers):
    return levels(_d(x), rp64(sd), layers)


def decode(cfs, sfs, sd, c_segs=None, s_segs=None):
    sd = rp64(sd)
    if c_segs is not None:
        import masked_ref as M
        y = block(M._fuse(cfs[-1], sfs[-1], c_segs, s_segs), sd, "rp_dec0.")
        for j, (cf, sf) in enumerate(list(zip(cfs[:-1], sfs[:-1]))[::-1]):
            y = block(M._fuse(cf, sf, c_segs, s_segs, skip=y), sd, f"rp_dec{j + 1}.")
        return y
    y = block(adain(cfs[-1], sfs[-1]), sd, "rp_dec0.")
    for j, sf in enumerate(sfs[:-1][::-1]):
        y = block(y + adain(y, sf), sd, f"rp_dec{j + 1}.")
    return y


def test(content, style, sd, layers, c_segs=None, s_segs=None):
    """LDMSAdaINRPNet.test in float64 -> torch float64 (N, 3, H, W)."""
    with torch.no_grad():
        return decode(encode(content, sd, layers), encode(style, sd, layers), sd, c_segs,
                      s_segs)


def key_table(sd):
    """state_dict -> (names as a unicode array, shapes as int64 (K, 4), padded with -1)."""
    names = np.array(list(sd.keys()))
    shapes = np.full((len(names), 4), -1, dtype=np.int64)
    for i, v in enumerate(sd.values()):
        shapes[i, :len(v.shape)] = tuple(v.shape)
    return names, shapes
