"""LDMSAdaINRPNet (`network: ld_adain`) training, the parts that need no GPU: the restatement
of the loss graph (tests/ld_train_ref.py) in float64 against the reference's recorded float64
losses and gradients (tests/golden/grads_ld*.npz), the golden's own conditions, the C ABI of the
7x7 backward kernels (bindings and argument errors) and the driver's network list."""
import copy
import re

import numpy as np
import pytest
import torch

import ld_train_ref as LT
from helpers import GRAD_FLOOR_SAMPLES, rel_l2, state_dict_of, synth_

NEW_SYMBOLS = ("rpst_conv7_wgrad_workspace_size", "rpst_conv7_wgrad", "rpst_reflect_pad_backward")


def test_golden_cases_and_floor_cap(golden):
    g = golden("grads_ld")
    assert int(g["n"]) == len(LT.CASES) == 3 and GRAD_FLOOR_SAMPLES == 6
    for i, (hid, layers, inc, shape, seed, cw, sw, cseed, sseed) in enumerate(LT.CASES):
        assert (int(g[f"hidden{i}"]), int(g[f"layers{i}"]), int(g[f"inception{i}"]),
                tuple(g[f"content{i}"].shape), int(g[f"seed{i}"]), float(g[f"cw{i}"]),
                float(g[f"sw{i}"]), int(g[f"cseed{i}"]), int(g[f"sseed{i}"])) == \
            (hid, layers, inc, shape, seed, cw, sw, cseed, sseed)
        names = [str(n) for n in g[f"names{i}"]]
        assert names and all(n.startswith(("rp_enc", "rp_dec")) for n in names)
        for n in names:
            # every bar max(1e-4, 3 x floor) is the base 1e-4
            assert float(g[f"floor{i}:{n}"]) <= 3.3e-5, (i, n)
            assert g[f"grad{i}:{n}"].dtype == np.float32
            assert g[f"grad64_{i}:{n}"].dtype == np.float64


@pytest.mark.parametrize("i", range(len(LT.CASES)))
def test_restatement_matches_reference_float64(golden, i):
    """ld_train_ref.grads in float64 against the reference's float64 run: 1e-12 rel-L2 (the bar
    of tests/test_ld_cpu.py's float64 restatement) for the losses and every gradient."""
    import network as net
    from rpst import synth
    g = golden("grads_ld")
    m = net.LDMSAdaINRPNet(LT.golden_config(g, i), copy.deepcopy(net.vgg))
    assert np.array_equal(synth_(m, int(g[f"seed{i}"])), g[f"checksum{i}"])
    c, s = g[f"content{i}"], g[f"style{i}"]
    assert np.array_equal(c, synth.image(int(g[f"cseed{i}"]), c.shape))
    assert np.array_equal(s, synth.image(int(g[f"sseed{i}"]), s.shape))
    losses, grads = LT.grads(torch.from_numpy(c).double(), torch.from_numpy(s).double(),
                             state_dict_of(m), int(g[f"layers{i}"]), float(g[f"cw{i}"]),
                             float(g[f"sw{i}"]))
    for k in ("style_loss", "content_loss", "total_loss"):
        assert rel_l2(losses[k], g[f"{k}64_{i}"]) < 1e-12, (i, k)
    names = [str(n) for n in g[f"names{i}"]]
    assert sorted(names) == sorted(grads)
    worst = max(rel_l2(grads[n], g[f"grad64_{i}:{n}"]) for n in names)
    print(f"case {i}: restatement gradients vs float64 reference, worst {worst:.2e}")
    assert worst < 1e-12, (i, worst)


def test_new_symbols_bound_and_declared():
    import os

    from rpst import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                               "include", "rpst.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
        decl = re.search(r"\b" + name + r"\(([^;]*)\);", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_conv7_wgrad_abi_argument_errors():
    """rpst_conv7_wgrad / rpst_reflect_pad_backward / rpst_conv_weight_flip check their
    arguments before touching the device."""
    from rpst import _lib
    lib = _lib.load()
    need = lib.rpst_conv7_wgrad_workspace_size(2, 8, 8, 8, 8)
    assert need >= 4 * 8 * (8 * 49 + 1)
    assert lib.rpst_conv7_wgrad_workspace_size(0, 8, 8, 8, 8) == 0

    def wgrad(x=1, dy=1, dw=1, db=None, N=2, Cin=8, H=8, W=8, Cout=8, pad=1, ws=1, nbytes=need):
        return lib.rpst_conv7_wgrad(x, dy, dw, db, N, Cin, H, W, Cout, pad, ws, nbytes, None)

    def err():
        return lib.rpst_last_error().decode()

    assert wgrad(x=None) == -1 and "null pointer" in err()
    assert wgrad(dy=None) == -1 and "null pointer" in err()
    assert wgrad(dw=None) == -1 and "null pointer" in err()
    assert wgrad(Cin=0) == -1 and "bad shape" in err()
    assert wgrad(H=3) == -1 and "reflect" in err()
    assert wgrad(W=3) == -1 and "reflect" in err()
    assert wgrad(pad=2) == -1 and "bad pad" in err()
    assert wgrad(nbytes=need - 1) != 0 and "workspace" in err()
    assert wgrad(ws=None) != 0 and "workspace" in err()
    assert lib.rpst_reflect_pad_backward(None, 1, 4, 8, 8, 3, None) == -1 and "null pointer" in err()
    assert lib.rpst_reflect_pad_backward(1, 1, 0, 8, 8, 3, None) == -1 and "bad shape" in err()
    assert lib.rpst_reflect_pad_backward(1, 1, 4, 3, 8, 3, None) == -1 and "reflect" in err()
    # the flip admits 1, 3 and 7
    assert lib.rpst_conv_weight_flip(1, 1, 8, 8, 5, None) == -1 and "bad args" in err()
    assert lib.rpst_conv_weight_flip(None, 1, 8, 8, 7, None) == -1


def test_ld_adain_is_trainable():
    import train
    assert "ld_adain" in train.TRAINABLE
    from rpst import ops
    assert "ld" in ops.TRAIN_F4
