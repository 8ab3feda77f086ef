"""Generate tests/golden/masked.npz by running the REFERENCE's segmentation-masked AdaIN
(`use_mask: True`) on CPU: network/base.py:421-530 and the two networks whose test() uses it.

Runs only in the build container, like gen_golden.py, whose stub-and-import approach it
reuses by importing that module. Nothing of the reference is copied: only inputs, label
arrays, outputs and weight checksums are written. The reference reads its masks from PNG
files (and prints their labels), so the label arrays are written to a temporary directory;
both the arrays at file resolution and the resized arrays the reference actually saw are
stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_masked.py
"""
from __future__ import annotations

import copy
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (stubs, reference import, synth helpers)

import helpers  # noqa: E402  (tests/helpers.py, on sys.path through gen_golden)
import masked_ref as M  # noqa: E402  (tests/masked_ref.py: mask writers)
from rpst import synth  # noqa: E402

# (name, content shape, style (h, w), mask mode, file-resolution factor, mask kind)
OP_CASES = [
    ("blocks_L", (2, 8, 24, 40), (24, 40), "L", 2, "blocks"),
    ("odd_P", (1, 3, 13, 9), (13, 9), "P", 1, "blocks"),
    ("wide_P", (1, 40, 17, 33), (17, 33), "P", 2, "blocks"),
    ("sizes_L", (1, 8, 24, 40), (16, 28), "L", 2, "blocks"),
    ("stripes_P", (1, 8, 24, 40), (24, 40), "P", 1, "stripes"),
    ("single_P", (1, 8, 24, 40), (24, 40), "P", 1, "single"),
]


def file_mask(kind, h, w, seed, style):
    if kind == "stripes":  # one-pixel-wide vertical stripes of three labels
        return np.tile((np.arange(w) % 3).astype(np.uint8) * 100, (h, 1))
    if kind == "single":
        return np.full((h, w), 5, dtype=np.uint8)
    # the content map has a label the style lacks (7) and the reverse (9), and a dot of
    # fewer than 11 pixels (label 200 in both maps)
    # (no label 255: the reference's `np.max(content_segment) + 1` wraps to 0 in uint8 and
    # its indicator array comes out empty, so it cannot run a content map that holds 255)
    labels = [0, 60, 120, 180, 9 if style else 7]
    return M.blocks_mask(h, w, labels, seed, dot=(200, h // 3, w // 4, 2, 3))


def gen_ops(nb, tmp, out):
    for i, (name, cshape, shw, mode, f, kind) in enumerate(OP_CASES):
        n, C, hc, wc = cshape
        hs, ws = shw
        c = G.rand_feat(6100 + i, cshape, scale=2.0, offset=0.5)
        s = G.rand_feat(6200 + i, (n, C, hs, ws), scale=3.0, offset=1.0, relu=True)
        cfile = np.stack([file_mask(kind, hc * f, wc * f, 6300 + 10 * i + b, False)
                          for b in range(n)])
        sfile = np.stack([file_mask(kind, hs * f, ws * f, 6400 + 10 * i + b, True)
                          for b in range(n)])
        res, csegs, ssegs = [], [], []
        for b in range(n):
            cp = M.write_mask_png(os.path.join(tmp, f"op{i}_{b}_c.png"), cfile[b], mode)
            sp = M.write_mask_png(os.path.join(tmp, f"op{i}_{b}_s.png"), sfile[b], mode)
            res.append(nb.adaptive_instance_normalization_with_segment(
                G.t(c[b:b + 1]), G.t(s[b:b + 1]), cp, sp).numpy())
            cs, ss, _, _ = nb.get_segment_and_info(cp, sp, (wc, hc), (ws, hs))
            csegs.append(np.array(cs))
            ssegs.append(np.array(ss))
        out.update({f"op{i}_name": name, f"op{i}_mode": mode, f"op{i}_c": c, f"op{i}_s": s,
                    f"op{i}_cfile": cfile, f"op{i}_sfile": sfile,
                    f"op{i}_cseg": np.stack(csegs), f"op{i}_sseg": np.stack(ssegs),
                    f"op{i}_out": np.concatenate(res)})
    out["n_ops"] = len(OP_CASES)


def gen_nets(net, nb, tmp, out):
    # MultiScaleAdaINRPNet.test: constant stack, hidden 8, 5 blocks, N=2, 24x40; masks at
    # twice the image size
    cfg = dict(G.multiscale_config(8, 5, 0), use_mask=True)
    m = net.MultiScaleAdaINRPNet(cfg, copy.deepcopy(net.vgg))
    out["ms_seed"], out["ms_checksum"] = 61, G.synth_model_(m, 61)
    c, s = synth.image(6500, (2, 3, 24, 40)), synth.image(6501, (2, 3, 24, 40))
    cfile = np.stack([file_mask("blocks", 48, 80, 6510 + b, False) for b in range(2)])
    sfile = np.stack([file_mask("blocks", 48, 80, 6520 + b, True) for b in range(2)])
    out.update(ms_content=c, ms_style=s, ms_cfile=cfile, ms_sfile=sfile)
    for mode in ("L", "P"):
        cps = [M.write_mask_png(os.path.join(tmp, f"ms{mode}{b}_c.png"), cfile[b], mode)
               for b in range(2)]
        sps = [M.write_mask_png(os.path.join(tmp, f"ms{mode}{b}_s.png"), sfile[b], mode)
               for b in range(2)]
        out[f"ms_out_{mode}"] = m.test(G.t(c), G.t(s), c_mask_path=cps, s_mask_path=sps).numpy()
        segs = [nb.get_segment_and_info(cp, sp, (40, 24), (40, 24)) for cp, sp in zip(cps, sps)]
        out[f"ms_cseg_{mode}"] = np.stack([np.array(g[0]) for g in segs])
        out[f"ms_sseg_{mode}"] = np.stack([np.array(g[1]) for g in segs])

    # SourceNet.test: N=1, 64x48, masks at the image size go down to the 8x6 relu4_1 grid
    sn = net.SourceNet({"use_mask": True, "content_weight": 1.0, "style_weight": 10.0},
                       copy.deepcopy(net.vgg))
    out["src_seed"], out["src_checksum"] = 62, G.synth_model_(sn, 62)
    c, s = synth.image(6600, (1, 3, 64, 48)), synth.image(6601, (1, 3, 64, 48))
    cfile = np.zeros((1, 64, 48), dtype=np.uint8)
    # top / bottom halves, swapped in the style: at 8x6 a palette mask keeps 24 pixels per
    # label; a greyscale one keeps 12 and gets four invented border labels of 6 (not valid)
    cfile[0, :32], cfile[0, 32:] = 40, 200
    sfile = np.zeros((1, 64, 48), dtype=np.uint8)
    sfile[0, :32], sfile[0, 32:] = 200, 40
    out.update(src_content=c, src_style=s, src_cfile=cfile, src_sfile=sfile)
    for mode in ("L", "P"):
        cp = M.write_mask_png(os.path.join(tmp, f"src{mode}_c.png"), cfile[0], mode)
        sp = M.write_mask_png(os.path.join(tmp, f"src{mode}_s.png"), sfile[0], mode)
        out[f"src_out_{mode}"] = sn.test(G.t(c), G.t(s), c_mask_path=[cp],
                                         s_mask_path=[sp]).numpy()
        cs, ss, _, _ = nb.get_segment_and_info(cp, sp, (6, 8), (6, 8))
        out[f"src_cseg_{mode}"] = np.array(cs)[None]
        out[f"src_sseg_{mode}"] = np.array(ss)[None]


def main():
    torch.set_num_threads(8)
    torch.manual_seed(0)
    net = G._import_reference()
    nb = sys.modules["network.base"]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        gen_ops(nb, tmp, out)
        gen_nets(net, nb, tmp, out)
    helpers.save_golden("masked", **out)
    print("masked goldens written to", HERE)


if __name__ == "__main__":
    main()
