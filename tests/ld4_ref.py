"""Float64 restatement of LDMSAdaINRPNet4 (`network: ld_adain4`) inference, written from the
formulas (not from the reference's modules), for the ld_adain4 tests and their goldens.

With h = hidden_dim, L = ld_layer_num, eps = 1e-5, B a Conv2dBlock (tests/ld_ref.block: reflect
3x3, the inception 1x1s, LeakyReLU 0.2 once at the end) and, per coarse level,

    big(x) = maxpool_2x2,s2,ceil(relu(conv3(reflect1(relu(conv3(reflect1(conv1(x))))))))

    fine_0   = small_0(x),   fine_i   = small_i(fine_{i-1})          all H x W, h channels
    coarse_0 = big_0(x),     coarse_i = big_i(coarse_{i-1})          ceil(H / 2^(i+1)) x ...
    level_i  = cat([fine_i, nearest(coarse_i -> H x W)])              2h channels
    nearest: per axis src = min(floor(dst * (float32(in) / float32(out))), in - 1), the product
             in fp32 (F.interpolate's default mode)
    y_0 = dec_0(F(c_{L-1}, s_{L-1}))
    y_k = dec_k(cat([y_{k-1}, F(c_{L-1-k}, s_{L-1-k})]))             k = 1 .. L-1
    F = AdaIN (tests/ld_ref.adain), or with masks the per-label AdaIN (tests/masked_ref.py),
        label maps at the image size.
"""
import numpy as np
import torch
import torch.nn.functional as F

import ld_ref as L

# (hidden, layers, inception, shape, stylized_layers, use_mask, model seed)
CASES = [
    (4, 3, 0, (2, 3, 24, 40), 3, False, 91),
    (4, 3, 0, (2, 3, 24, 40), 3, True, 91),
    (8, 3, 1, (1, 3, 17, 33), 1, False, 92),
    (8, 4, 0, (1, 3, 19, 37), 2, False, 93),
    (16, 5, 0, (1, 3, 32, 48), 5, False, 94),
    (32, 5, 0, (1, 3, 33, 50), 1, False, 95),
]
LEVEL_BYTES = 1 << 20  # float64 levels are recorded for cases whose levels total less


def config(hidden, layers, inception=0, stylized_layers=None, use_mask=False):
    """An ld_adain4 config (train_ld4_multiscale_rp_adain.yaml's model keys)."""
    cfg = L.config(hidden, layers, inception, use_mask)
    cfg["stylized_layers"] = layers if stylized_layers is None else stylized_layers
    cfg["rp_blocks"] = max(layers, 2)  # (read by the base constructor only, which wants >= 2)
    return cfg


def golden_config(g, i):
    """The config of case i of tests/golden/ld4*.npz."""
    return config(int(g[f"net{i}_hidden"]), int(g[f"net{i}_layers"]), int(g[f"net{i}_inception"]),
                  int(g[f"net{i}_stylized_layers"]), bool(g[f"net{i}_use_mask"]))


def level_bytes(hidden, layers, shape):
    n, _, h, w = shape
    return 8 * layers * n * 2 * hidden * h * w


def nearest_index(size_in, size_out):
    """int64 (size_out,): the source index of every destination index along one axis."""
    scale = np.float32(size_in) / np.float32(size_out)
    src = np.floor(np.arange(size_out, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(src, size_in - 1)


def resize_nearest(x, size):
    iy = torch.from_numpy(nearest_index(x.shape[2], size[0]))
    ix = torch.from_numpy(nearest_index(x.shape[3], size[1]))
    return x[:, :, iy][:, :, :, ix]


def big(x, sd, prefix):
    """A coarse-chain level from its state_dict entries under `prefix` (Sequential indices 0, 2
    and 5 hold the convs), in x's dtype."""
    y = F.conv2d(x, sd[prefix + "0.weight"], sd[prefix + "0.bias"])
    for j in (2, 5):
        y = torch.relu(L.conv_pad(y, sd[f"{prefix}{j}.weight"], sd[f"{prefix}{j}.bias"]))
    return F.max_pool2d(y, 2, 2, ceil_mode=True)


def encode(x, sd, layers):
    fine = coarse = L._d(x)
    sd, feats = L.rp64(sd), []
    for i in range(layers):
        fine = L.block(fine, sd, f"rp_enc{i}_small_revf.")
        coarse = big(coarse, sd, f"rp_enc{i}_big_revf.")
        feats.append(torch.cat([fine, resize_nearest(coarse, fine.shape[2:])], dim=1))
    return feats


def decode(cfs, sfs, sd, c_segs=None, s_segs=None):
    sd = L.rp64(sd)
    if c_segs is not None:
        import masked_ref as M

        def fuse(c, s):
            return M._fuse(c, s, c_segs, s_segs)
    else:
        fuse = L.adain
    y = L.block(fuse(cfs[-1], sfs[-1]), sd, "rp_dec0.")
    for k, (cf, sf) in enumerate(list(zip(cfs[:-1], sfs[:-1]))[::-1]):
        y = L.block(torch.cat([y, fuse(cf, sf)], dim=1), sd, f"rp_dec{k + 1}.")
    return y


def test(content, style, sd, layers, c_segs=None, s_segs=None):
    """LDMSAdaINRPNet4.test in float64 -> torch float64 (N, 3, H, W)."""
    with torch.no_grad():
        return decode(encode(content, sd, layers), encode(style, sd, layers), sd, c_segs,
                      s_segs)


key_table = L.key_table
