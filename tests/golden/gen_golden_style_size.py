"""Generate tests/golden/style_size.npz by running the REFERENCE's SAModel.test
(network/sanet.py:238-246) and WCTRPNet.test (network/wct_rp.py:139-147) on CPU with a style
image of another size than the content.

Runs only in the build container, like gen_golden_ld4.py, whose stub-and-import approach it
reuses. Nothing of the reference is copied: only inputs, seeds, weight checksums and outputs.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_style_size.py
"""
from __future__ import annotations

import copy
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (stubs, reference import, synth helpers)

import helpers  # noqa: E402  (tests/helpers.py, on sys.path through gen_golden)
from rpst import synth  # noqa: E402

# content / style shapes of tests/test_gpu_style_size.py's model tests
SA_SEED, SA_CONTENT, SA_STYLE = 74, (2, 3, 64, 48), (2, 3, 48, 80)
WCT_SEED, WCT_HIDDEN, WCT_BLOCKS, WCT_CONTENT, WCT_STYLE = 76, 16, 3, (2, 3, 24, 40), (2, 3, 33, 19)


def main():
    torch.set_num_threads(8)
    torch.manual_seed(0)
    net = G._import_reference()
    out = {}
    m = net.SAModel({}, copy.deepcopy(net.vgg), 0, 64)
    ck = G.synth_model_(m, SA_SEED)
    c, s = synth.image(9300, SA_CONTENT), synth.image(9301, SA_STYLE)
    y = m.test(G.t(c), G.t(s)).numpy()
    assert y.shape == c.shape
    out.update(sa_seed=SA_SEED, sa_checksum=ck, sa_content=c, sa_style=s, sa_out=y)
    w = net.WCTRPNet(G.rp_config(WCT_HIDDEN, WCT_BLOCKS), copy.deepcopy(net.vgg))
    ck = G.synth_model_(w, WCT_SEED)
    c, s = synth.image(9302, WCT_CONTENT), synth.image(9303, WCT_STYLE)
    y = w.test(G.t(c), G.t(s)).numpy()
    assert y.shape == c.shape
    out.update(wct_seed=WCT_SEED, wct_hidden=WCT_HIDDEN, wct_blocks=WCT_BLOCKS, wct_checksum=ck,
               wct_content=c, wct_style=s, wct_out=y)
    helpers.save_golden("style_size", **out)
    print("style-size goldens written to", HERE)


if __name__ == "__main__":
    main()
