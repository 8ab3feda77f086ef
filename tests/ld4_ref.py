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


def encode(x, sd, layers, dtype=torch.float64):
    fine = coarse = L._d(x, dtype)
    sd, feats = L.rp64(sd, dtype), []
    for i in range(layers):
        fine = L.block(fine, sd, f"rp_enc{i}_small_revf.")
        coarse = big(coarse, sd, f"rp_enc{i}_big_revf.")
        feats.append(torch.cat([fine, resize_nearest(coarse, fine.shape[2:])], dim=1))
    return feats


def decode(cfs, sfs, sd, c_segs=None, s_segs=None, dtype=torch.float64):
    sd = L.rp64(sd, dtype)
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


def test(content, style, sd, layers, c_segs=None, s_segs=None, dtype=torch.float64):
    """LDMSAdaINRPNet4.test in float64 -> torch float64 (N, 3, H, W); with dtype
    torch.float32 the same formulas in fp32, whose distance to the float64 run is the
    rounding floor of an fp32 implementation."""
    with torch.no_grad():
        return decode(encode(content, sd, layers, dtype), encode(style, sd, layers, dtype), sd,
                      c_segs, s_segs, dtype)


key_table = L.key_table


# ---- the bandwidth kernels' walk over a plane, restated --------------------------------------
# The constants of rp-style-transfer_amd/csrc/rpst_ld4.hip: keep them equal.
CHUNK = 4096         # kLd4Chunk: destination elements (1024 quads) per workgroup
STRIDE_QUADS = 256   # kLd4Threads: source quads per stride of resized_stats_kernel


def fuse_inputs(ca, hd, size, csize, n=2):
    """ld4_fuse's operands with the content half inside a [content; style] batch of 2n:
    (y or None, fine, coarse, [statistics of the fine half, of the coarse half]), each
    statistics tensor (4, n, hd) = (mean_c, std_c, mean_s, std_s), distinct per image,
    std > 0."""
    from helpers import gen
    fine = gen(51, (2 * n, hd, *size), 1.5, 0.3)
    coarse = gen(52, (2 * n, hd, *csize), 2.0, -0.2)
    y = gen(53, (n, ca, *size), 1.0, 0.1) if ca else None
    stats = [gen(54 + k, (4, n, hd), 0.5, 1.25) for k in range(2)]
    return y, fine, coarse, stats


def fuse_want(fine, coarse, stats, size, n=2, resized=None):
    """float64 (n, 2 hd, H, W): cat([affine(fine[:n]), affine(resize(coarse[:n]))]); `resized`
    stands in for the resize (a planted slip's)."""
    hd = fine.shape[1]

    def affine(v, s):
        mc, sc, ms, ss = (s[k].double().view(n, hd, 1, 1) for k in range(4))
        return (v.double() - mc) / sc * ss + ms

    if resized is None:
        resized = F.interpolate(coarse[:n], size)
    return torch.cat([affine(fine[:n], stats[0]), affine(resized, stats[1])], dim=1)


def write_planes(val, first_plane=0, slip=None):
    """write_plane_chunk's walk over destination planes, in numpy: val (P, HW) holds what
    each element should become; plane p of the (16-byte aligned, contiguous) destination is
    plane first_plane + p of its tensor, so its head is (-(first_plane + p) HW) % 4 elements.
    Head and tail are written one by one, quad q at elements head + 4 q .. + 3, 1024 quads a
    chunk. Unwritten elements stay 0. slip plants a wrong walk:
      'chunk_base'  chunk k > 0 takes its values at chunk 0's quads (q - 1024 k)
      'no_head'     the values of quad q are taken at 4 q where the plane's head is not 0
      'no_tail'     the tail elements are not written"""
    val = np.asarray(val)
    P, HW = val.shape
    out = np.zeros_like(val)
    for p in range(P):
        head = min((-(first_plane + p) * HW) % 4, HW)
        nq = (HW - head) // 4
        out[p, :head] = val[p, :head]
        if slip != "no_tail":
            out[p, head + 4 * nq:] = val[p, head + 4 * nq:]
        q = np.arange(nq)
        src_q = q % (CHUNK // 4) if slip == "chunk_base" else q
        src0 = 0 if slip == "no_head" else head
        j = np.arange(4)
        out[p, (head + 4 * q)[:, None] + j] = val[p, (src0 + 4 * src_q)[:, None] + j]
    return out


def resized_stats(x, size, slip=None):
    """resized_stats_kernel's form in float64: every source element of x (N, C, h, w) weighted
    by its replication count, sums of d = x - x[0] per plane over the quads and the 0-3 tail
    elements, mean = x[0] + t1 / n, std = sqrt((t2 - t1 t1 / n) / (n - 1) + eps), n = H W.
    slip: 'one_stride' (quads past the first 256 are left out), 'no_tail' (the tail is)."""
    x = torch.as_tensor(x).double()
    N, C, h, w = x.shape
    wy = np.bincount(nearest_index(h, size[0]), minlength=h)
    wx = np.bincount(nearest_index(w, size[1]), minlength=w)
    wgt = torch.from_numpy(np.outer(wy, wx).reshape(-1).astype(np.float64)).clone()
    hw, nq = h * w, (h * w) // 4
    if slip == "one_stride":
        wgt[4 * STRIDE_QUADS:4 * nq] = 0
    elif slip == "no_tail":
        wgt[4 * nq:] = 0
    v = x.reshape(N, C, hw)
    d = v - v[..., :1]
    n = float(size[0] * size[1])
    t1, t2 = (wgt * d).sum(-1), (wgt * d * d).sum(-1)
    var = (t2 - t1 * t1 / n) / (n - 1.0)
    return ((v[..., 0] + t1 / n).view(N, C, 1, 1),
            torch.sqrt(var.clamp_min(0) + L.EPS).view(N, C, 1, 1))
