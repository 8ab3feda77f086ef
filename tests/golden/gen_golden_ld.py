"""Generate tests/golden/ld*.npz by running the REFERENCE's LDMSAdaINRPNet (`network:
ld_adain`, network/adain_rp.py:484-567) test() on CPU, with and without `use_mask`.

Runs only in the build container, like gen_golden.py, whose stub-and-import approach it reuses.
Nothing of the reference is copied: only inputs, seeds, weight checksums, the fp32 and float64
outputs, the reference's own fp32-against-float64 distance (`floor`), every level of
encode_rp_intermediate(content) in float64 with the fp32 run's distance to it, the state_dict
key list with shapes and, for the masked case, the mask files' arrays and the label maps the
reference resized them to.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_ld.py
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
import gen_golden_masked as GM  # noqa: E402  (file_mask)

import helpers  # noqa: E402  (tests/helpers.py, on sys.path through gen_golden)
import ld_ref as L  # noqa: E402  (tests/ld_ref.py: cases, config, key table)
import masked_ref as M  # noqa: E402  (tests/masked_ref.py: mask writers)
from rpst import synth  # noqa: E402


def main():
    torch.set_num_threads(8)
    torch.manual_seed(0)
    net = G._import_reference()
    nb = sys.modules["network.base"]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, (hid, layers, inc, shape, use_mask, seed) in enumerate(L.CASES):
            m = net.LDMSAdaINRPNet(L.config(hid, layers, inc, use_mask), copy.deepcopy(net.vgg))
            ck = G.synth_model_(m, seed)
            n, _, h, w = shape
            c, s = synth.image(8100 + 2 * i, shape), synth.image(8101 + 2 * i, shape)
            kw = {}
            if use_mask:  # masks at twice the image size, greyscale files
                cfile = np.stack([GM.file_mask("blocks", 2 * h, 2 * w, 8210 + b, False)
                                  for b in range(n)])
                sfile = np.stack([GM.file_mask("blocks", 2 * h, 2 * w, 8220 + b, True)
                                  for b in range(n)])
                cps = [M.write_mask_png(os.path.join(tmp, f"ld{i}_{b}_c.png"), cfile[b], "L")
                       for b in range(n)]
                sps = [M.write_mask_png(os.path.join(tmp, f"ld{i}_{b}_s.png"), sfile[b], "L")
                       for b in range(n)]
                kw = dict(c_mask_path=cps, s_mask_path=sps)
                segs = [nb.get_segment_and_info(cp, sp, (w, h), (w, h))
                        for cp, sp in zip(cps, sps)]
                out.update({f"net{i}_cfile": cfile, f"net{i}_sfile": sfile,
                            f"net{i}_cseg": np.stack([np.array(g[0]) for g in segs]),
                            f"net{i}_sseg": np.stack([np.array(g[1]) for g in segs])})
            y = m.test(G.t(c), G.t(s), **kw).numpy()
            m64 = copy.deepcopy(m).double()
            y64 = m64.test(G.t(c).double(), G.t(s).double(), **kw).numpy()
            with torch.no_grad():
                lv = [f.numpy() for f in m.encode_rp_intermediate(G.t(c))]
                lv64 = [f.numpy() for f in m64.encode_rp_intermediate(G.t(c).double())]
            names, shapes = L.key_table(m.state_dict())
            out.update({f"net{i}_hidden": hid, f"net{i}_layers": layers, f"net{i}_inception": inc,
                        f"net{i}_use_mask": use_mask, f"net{i}_seed": seed, f"net{i}_checksum": ck,
                        f"net{i}_content": c, f"net{i}_style": s, f"net{i}_out": y,
                        f"net{i}_out64": y64, f"net{i}_floor": helpers.rel_l2(y, y64),
                        f"net{i}_keys": names, f"net{i}_shapes": shapes})
            # the levels are kept in float64 only (the fp32 run's distance to them as a number):
            # both precisions of the 512-channel case would double the committed bytes
            for k, (a, a64) in enumerate(zip(lv, lv64)):
                out[f"net{i}_level{k}_64"] = a64
                out[f"net{i}_level{k}_floor"] = helpers.rel_l2(a, a64)
            print(f"ld {hid}x{layers} inc {inc} {shape} mask={use_mask}: "
                  f"floor {out[f'net{i}_floor']:.2e}")
    out["n_net"] = len(L.CASES)
    helpers.save_golden("ld", **out)
    print("ld_adain goldens written to", HERE)


if __name__ == "__main__":
    main()
