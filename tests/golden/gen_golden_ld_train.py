"""Generate tests/golden/grads_ld*.npz by running the REFERENCE's LDMSAdaINRPNet (`network:
ld_adain`, network/adain_rp.py:484-567) forward() + total_loss.backward() on the CPU.

Runs only in the build container, like gen_golden.py, whose stub-and-import approach it reuses.
Nothing of the reference is copied. Per case (tests/ld_train_ref.py: CASES) the reference runs
in fp32 and in float64 on the case's inputs and on GRAD_FLOOR_SAMPLES - 1 copies moved by one
fp32 ulp per element (helpers.ulp_perturbed); stored are the inputs, seeds and the weight
checksum, the fp32 and float64 losses and gradients of the unperturbed inputs, and per loss /
gradient tensor the floor: the RMS over the samples of rel-L2(fp32, float64).

Every gradient floor must be <= FLOOR_CAP, so that every test bar max(1e-4, 3 x floor) is the
base 1e-4: an ill-conditioned case would loosen its own test. A case that breaks the cap gets
another model seed, never a higher cap.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_ld_train.py
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (stubs, reference import, synth helpers)

sys.path.insert(0, G.REPO)  # oracle/, which tests/ld_train_ref.py composes
import helpers  # noqa: E402  (tests/helpers.py, on sys.path through gen_golden)
import ld_train_ref as LT  # noqa: E402  (tests/ld_train_ref.py: cases, config)
from rpst import synth  # noqa: E402

FLOOR_CAP = 3.3e-5


def _run(net, case, c, s, dt):
    hid, layers, inc, shape, seed, cw, sw, cseed, sseed = case
    m = net.LDMSAdaINRPNet(LT.config(hid, layers, inc, cw, sw), copy.deepcopy(net.vgg))
    ck = G.synth_model_(m, seed)
    m = m.to(dt)
    m.zero_grad()
    d, tot = m.forward(G.t(c).to(dt), G.t(s).to(dt))
    tot.backward()
    grads = {k: p.grad.detach().numpy() for k, p in m.named_parameters()
             if p.grad is not None and k.startswith("rp_")}
    return ck, {k: v.detach().numpy() for k, v in d.items()}, grads


def main():
    torch.set_num_threads(8)
    torch.manual_seed(0)
    net = G._import_reference()
    out = {}
    for i, case in enumerate(LT.CASES):
        hid, layers, inc, shape, seed, cw, sw, cseed, sseed = case
        c0, s0 = synth.image(cseed, shape), synth.image(sseed, shape)
        sq, lsq = {}, {}
        for smp in range(helpers.GRAD_FLOOR_SAMPLES):
            c, s = c0, s0
            if smp:
                c = helpers.ulp_perturbed(c0, 7000 + 2 * smp)
                s = helpers.ulp_perturbed(s0, 7001 + 2 * smp)
            ck, l32, g32 = _run(net, case, c, s, torch.float32)
            _, l64, g64 = _run(net, case, c, s, torch.float64)
            assert set(g32) == set(g64) and g32
            if smp == 0:
                out.update({f"hidden{i}": hid, f"layers{i}": layers, f"inception{i}": inc,
                            f"seed{i}": seed, f"checksum{i}": ck, f"cw{i}": cw, f"sw{i}": sw,
                            f"cseed{i}": cseed, f"sseed{i}": sseed, f"content{i}": c,
                            f"style{i}": s, f"names{i}": np.array(list(g32))})
                for k in l32:
                    out[f"{k}{i}"] = l32[k]
                    out[f"{k}64_{i}"] = l64[k]
                for k in g32:
                    assert g64[k].dtype == np.float64
                    out[f"grad{i}:{k}"] = g32[k]
                    out[f"grad64_{i}:{k}"] = g64[k]
            for k in l32:
                lsq[k] = lsq.get(k, 0.0) + helpers.rel_l2(l32[k], l64[k]) ** 2
            for k in g32:
                sq[k] = sq.get(k, 0.0) + helpers.rel_l2(g32[k], g64[k]) ** 2
        for k, v in lsq.items():
            out[f"lossfloor{i}:{k}"] = np.array(np.sqrt(v / helpers.GRAD_FLOOR_SAMPLES))
        worst = 0.0
        for k, v in sq.items():
            f = float(np.sqrt(v / helpers.GRAD_FLOOR_SAMPLES))
            out[f"floor{i}:{k}"] = np.array(f)
            worst = max(worst, f)
        print(f"grads_ld case {i} {case}: worst gradient floor {worst:.2e}", flush=True)
        assert worst <= FLOOR_CAP, (i, worst, "change the case's model seed, not the cap")
    out["n"] = len(LT.CASES)
    helpers.save_golden("grads_ld", **out)
    print("ld_adain training goldens written to", HERE)


if __name__ == "__main__":
    main()
