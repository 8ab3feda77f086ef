"""Float64 restatement of segmentation-masked AdaIN, written from its contract (not from the
reference's text), for the tests of the masked kernels:

  for one image pair, content features (C, hc, wc) with label map (hc, wc), style features
  (C, hs, ws) with label map (hs, ws):
    a label l is valid iff, with c / s its pixel counts in the content / style map,
        c > 10 and s > 10 and c / s < 100 and s / c < 100;
    a content pixel with a valid label l becomes, per channel,
        (x - mean_c[l]) / std_c[l] * std_s[l] + mean_s[l],
      mean / std over the pixels labelled l in the content / style feature,
      std = sqrt(unbiased variance + 1e-5);
    every other content pixel is copied.

Also: the two networks' masked test() composed from the oracle's layer restatements, and
the PNG writers the tests and the golden generator share.
"""
import numpy as np
import torch

EPS = 1e-5


def label_counts(c_seg, s_seg):
    """-> int64 (256, 3): content count, style count, valid flag per label."""
    c = np.bincount(np.asarray(c_seg, dtype=np.uint8).reshape(-1), minlength=256).astype(np.int64)
    s = np.bincount(np.asarray(s_seg, dtype=np.uint8).reshape(-1), minlength=256).astype(np.int64)
    valid = (c > 10) & (s > 10) & (c < 100 * s) & (s < 100 * c)
    return np.stack([c, s, valid.astype(np.int64)], axis=1)


def _mean_std(x):
    """x float64 (C, k) -> mean, std (C,)."""
    k = x.shape[1]
    mean = x.sum(axis=1) / k
    var = ((x - mean[:, None]) ** 2).sum(axis=1) / (k - 1)
    return mean, np.sqrt(var + EPS)


def masked_params(content, style, c_seg, s_seg):
    """One image pair -> float64 (C, 256, 4) = (mean_c, std_c, std_s, mean_s) per label (the
    kernels' row order), and the (256, 3) label counts. Rows of labels that are not valid
    hold (0, -1, 1, 0): pass-through."""
    content = np.asarray(content, dtype=np.float64)
    style = np.asarray(style, dtype=np.float64)
    C = content.shape[0]
    cf, sf = content.reshape(C, -1), style.reshape(C, -1)
    cl, sl = np.asarray(c_seg).reshape(-1), np.asarray(s_seg).reshape(-1)
    counts = label_counts(c_seg, s_seg)
    rows = np.tile(np.array([0.0, -1.0, 1.0, 0.0]), (C, 256, 1))
    for lab in np.nonzero(counts[:, 2])[0]:
        mc, sc = _mean_std(cf[:, cl == lab])
        ms, ss = _mean_std(sf[:, sl == lab])
        rows[:, lab] = np.stack([mc, sc, ss, ms], axis=1)
    return rows, counts


def masked_adain(content, style, c_seg, s_seg, skip=None):
    """One image pair, float64: content (C, hc, wc), style (C, hs, ws) -> (C, hc, wc)."""
    content = np.asarray(content, dtype=np.float64)
    rows, counts = masked_params(content, style, c_seg, s_seg)
    C = content.shape[0]
    out = content.reshape(C, -1).copy()
    cl = np.asarray(c_seg).reshape(-1)
    for lab in np.nonzero(counts[:, 2])[0]:
        m = cl == lab
        mc, sc, ss, ms = (rows[:, lab, k][:, None] for k in range(4))
        out[:, m] = (out[:, m] - mc) / sc * ss + ms
    out = out.reshape(content.shape)
    return out if skip is None else np.asarray(skip, dtype=np.float64) + out


def masked_adain_batch(content, style, c_segs, s_segs, skip=None):
    """Batch (N, C, h, w); image n uses c_segs[n], s_segs[n] -> float64 numpy."""
    content, style = np.asarray(content), np.asarray(style)
    return np.stack([masked_adain(content[n], style[n], c_segs[n], s_segs[n],
                                  None if skip is None else np.asarray(skip)[n])
                     for n in range(content.shape[0])])


def _fuse(cf, sf, c_segs, s_segs, skip=None):
    """Masked AdaIN of torch features in float64, returned in the features' dtype."""
    out = masked_adain_batch(cf.double().numpy(), sf.double().numpy(), c_segs, s_segs)
    out = torch.from_numpy(out).to(cf.dtype)
    return out if skip is None else skip + out


def multiscale_test(content, style, sd, rp_blocks, c_segs, s_segs):
    """MultiScaleAdaINRPNet.test with use_mask (constant stack): the deepest level decodes
    the masked AdaIN, every shallower one stylized + masked AdaIN of its level. The label
    maps are at the image size, which every level shares. Layers run in content's dtype."""
    from oracle import restate as R
    with torch.no_grad():
        def enc(x):
            feats = []
            for i in range(rp_blocks):
                x = R.conv2d_block(x, sd, f"rp_shared_encoder.{i}.")
                feats.append(x)
            return feats
        cfs, sfs = enc(content), enc(style)
        y = R.conv2d_block(_fuse(cfs[-1], sfs[-1], c_segs, s_segs), sd, "rp_decoder.0.")
        for i, (cf, sf) in enumerate(list(zip(cfs[:-1], sfs[:-1]))[::-1]):
            y = R.conv2d_block(_fuse(cf, sf, c_segs, s_segs, skip=y), sd, f"rp_decoder.{i + 1}.")
        return y


def sourcenet_test(content, style, sd, c_segs, s_segs):
    """SourceNet.test with use_mask: decoder(masked AdaIN of relu4_1); label maps at the
    relu4_1 size."""
    from oracle import restate as R
    with torch.no_grad():
        c4 = R.encode_with_intermediate(content, sd)[-1]
        s4 = R.encode_with_intermediate(style, sd)[-1]
        return R.decoder(_fuse(c4, s4, c_segs, s_segs), sd, "decoder.")


# ---- mask files --------------------------------------------------------------------------
def write_mask_png(path, labels, mode):
    """uint8 (h, w) label map -> PNG in mode 'L' (greyscale) or 'P' (palette index = label,
    explicit 256-entry grey palette); asserts that the labels survive a save / load."""
    from PIL import Image
    labels = np.ascontiguousarray(labels, dtype=np.uint8)
    h, w = labels.shape
    if mode == "L":
        im = Image.frombytes("L", (w, h), labels.tobytes())
    elif mode == "P":
        im = Image.frombytes("P", (w, h), labels.tobytes())
        im.putpalette([v for i in range(256) for v in (i, i, i)])
    else:
        raise ValueError(mode)
    im.save(path)
    with Image.open(path) as back:
        assert back.mode == mode, (back.mode, mode)
        assert np.array_equal(np.asarray(back), labels), f"{mode} labels changed on disk"
    return path


def blocks_mask(h, w, labels, seed, dot=None):
    """A piecewise-constant label map (h, w): a grid of rectangles, labels drawn from
    `labels` in a fixed pseudo-random order; dot = (label, y, x, hh, ww) stamps a small
    rectangle of another label."""
    rng = np.random.default_rng(seed)
    gy, gx = 2, 3
    m = np.zeros((h, w), dtype=np.uint8)
    ys = np.linspace(0, h, gy + 1).astype(int)
    xs = np.linspace(0, w, gx + 1).astype(int)
    order = [labels[k % len(labels)] for k in rng.permutation(gy * gx)]
    for j in range(gy):
        for i in range(gx):
            m[ys[j]:ys[j + 1], xs[i]:xs[i + 1]] = order[j * gx + i]
    if dot is not None:
        lab, y, x, hh, ww = dot
        m[y:y + hh, x:x + ww] = lab
    return m
