"""Generate tests/golden/ld4*.npz by running the REFERENCE's LDMSAdaINRPNet4 (`network:
ld_adain4`, network/adain_rp.py:711-819) test() and encode_rp_intermediate() on CPU, in fp32
and float64, with and without `use_mask`.

Runs only in the build container, like gen_golden_ld.py, whose stub-and-import approach it
reuses. Nothing of the reference is copied: only inputs, seeds, weight checksums, the fp32 and
float64 outputs, the reference's own fp32-against-float64 distance (`floor`), the state_dict
key list with shapes, for the masked case the mask files' arrays and the label maps the
reference resized them to, and, for the cases whose levels total under ld4_ref.LEVEL_BYTES,
every level of encode_rp_intermediate(content) in float64 with the fp32 run's distance to it
(the distance alone for the larger cases).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_ld4.py
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
import ld4_ref as L4  # noqa: E402  (tests/ld4_ref.py: cases, config, key table)
import masked_ref as M  # noqa: E402  (tests/masked_ref.py: mask writers)
from rpst import synth  # noqa: E402


def main():
    torch.set_num_threads(8)
    torch.manual_seed(0)
    net = G._import_reference()
    nb = sys.modules["network.base"]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, (hid, layers, inc, shape, sl, use_mask, seed) in enumerate(L4.CASES):
            m = net.LDMSAdaINRPNet4(L4.config(hid, layers, inc, sl, use_mask),
                                    copy.deepcopy(net.vgg))
            ck = G.synth_model_(m, seed)
            n, _, h, w = shape
            # the masked case shares the unmasked one's seed, and so its images
            c, s = synth.image(9100 + 2 * seed, shape), synth.image(9101 + 2 * seed, shape)
            kw = {}
            if use_mask:  # masks at twice the image size, greyscale files
                cfile = np.stack([GM.file_mask("blocks", 2 * h, 2 * w, 9210 + b, False)
                                  for b in range(n)])
                sfile = np.stack([GM.file_mask("blocks", 2 * h, 2 * w, 9220 + b, True)
                                  for b in range(n)])
                cps = [M.write_mask_png(os.path.join(tmp, f"ld4_{i}_{b}_c.png"), cfile[b], "L")
                       for b in range(n)]
                sps = [M.write_mask_png(os.path.join(tmp, f"ld4_{i}_{b}_s.png"), sfile[b], "L")
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
            names, shapes = L4.key_table(m.state_dict())
            out.update({f"net{i}_hidden": hid, f"net{i}_layers": layers, f"net{i}_inception": inc,
                        f"net{i}_stylized_layers": sl, f"net{i}_use_mask": use_mask,
                        f"net{i}_seed": seed, f"net{i}_checksum": ck, f"net{i}_content": c,
                        f"net{i}_style": s, f"net{i}_out": y, f"net{i}_out64": y64,
                        f"net{i}_floor": helpers.rel_l2(y, y64), f"net{i}_keys": names,
                        f"net{i}_shapes": shapes})
            keep = L4.level_bytes(hid, layers, shape) < L4.LEVEL_BYTES
            out[f"net{i}_has_levels"] = keep
            for k, (a, a64) in enumerate(zip(lv, lv64)):
                if keep:
                    out[f"net{i}_level{k}_64"] = a64
                out[f"net{i}_level{k}_floor"] = helpers.rel_l2(a, a64)
            print(f"ld4 {hid}x{layers} inc {inc} {shape} sl {sl} mask={use_mask}: floor "
                  f"{out[f'net{i}_floor']:.2e}, level floors "
                  f"{max(out[f'net{i}_level{k}_floor'] for k in range(layers)):.2e}, "
                  f"levels kept: {keep}")
    out["n_net"] = len(L4.CASES)
    helpers.save_golden("ld4", **out)
    print("ld_adain4 goldens written to", HERE)


if __name__ == "__main__":
    main()
