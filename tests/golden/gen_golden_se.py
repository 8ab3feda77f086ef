"""Generate tests/golden/se*.npz by running the REFERENCE's SE channel attention
(`attention: se`) on CPU: SEBottleneck (network/attention.py:25-66) alone, and
MultiScaleAdaINRPNet.test() with an SEBottleneck after every encoder block
(network/adain_rp.py:160-168), with and without `use_mask`.

Runs only in the build container, like gen_golden.py, whose stub-and-import approach it reuses.
Nothing of the reference is copied: only inputs, seeds, weight checksums, outputs, attention
maps, the reference's own fp32-against-float64 distance (`floor`) and the state_dict key list
with shapes are written.

A module case whose gates would not tell a kernel that ignores them from a correct one is
refused here: the seed moves on until the gates span (< 0.3, > 0.7), are not all equal and,
in a batch, differ by more than 0.1 between two images on some channel.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_se.py
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
import masked_ref as M  # noqa: E402  (tests/masked_ref.py: mask writers)
import se_ref as S  # noqa: E402  (tests/se_ref.py: inputs, weight rules, key table)
from rpst import synth  # noqa: E402

# (N, C, H, W), first seed tried
MODULE_CASES = [((2, 32, 24, 40), 7100), ((1, 48, 13, 9), 7200), ((1, 16, 17, 33), 7300)]
SEED_TRIES = 4000  # single images at unit scale rarely spread their gates that far
# (hidden, blocks, (N, 3, H, W), use_mask, model seed)
NET_CASES = [(32, 5, (2, 3, 24, 40), False, 71), (32, 5, (2, 3, 24, 40), True, 71),
             (48, 3, (1, 3, 20, 28), False, 72)]


def gates_discriminate(g):
    g = g.reshape(g.shape[0], -1)
    ok = g.min() < 0.3 and g.max() > 0.7 and not np.all(g == g.flat[0])
    if g.shape[0] > 1:
        ok = ok and max(np.abs(g[a] - g[b]).max() for a in range(g.shape[0])
                        for b in range(a)) > 0.1
    return bool(ok)


def gen_modules(att, out):
    for i, (shape, seed0) in enumerate(MODULE_CASES):
        n, C, h, w = shape
        x = S.module_input(7000 + i, shape)
        for seed in range(seed0, seed0 + SEED_TRIES):
            blk = att.SEBottleneck(C, C).eval()
            ck = S.synth_block_(blk, seed)
            with torch.no_grad():
                y = blk(G.t(x).clone()).numpy()
            g = blk.attention_map.numpy()
            if gates_discriminate(g):
                break
        else:
            raise AssertionError(f"module case {i}: no seed in {seed0}..{seed0 + SEED_TRIES - 1} gives "
                                 "gates that depend on the channel and the image")
        assert gates_discriminate(g), i
        with torch.no_grad():
            y64 = copy.deepcopy(blk).double()(G.t(x).double()).numpy()
        names, shapes = S.key_table(blk.state_dict())
        out.update({f"mod{i}_x": x, f"mod{i}_seed": seed, f"mod{i}_checksum": ck,
                    f"mod{i}_out": y, f"mod{i}_gate": g,
                    f"mod{i}_floor": helpers.rel_l2(y, y64),
                    f"mod{i}_keys": names, f"mod{i}_shapes": shapes})
        print(f"module {shape}: seed {seed} gates {g.min():.3f}..{g.max():.3f} "
              f"floor {out[f'mod{i}_floor']:.2e}")
    out["n_mod"] = len(MODULE_CASES)


def attention_maps(m):
    return [blk.attention_map.detach().numpy().copy() for blk in m.rp_shared_encoder]


def gen_nets(net, tmp, out):
    for i, (hid, blocks, shape, use_mask, seed) in enumerate(NET_CASES):
        cfg = dict(G.multiscale_config(hid, blocks, 0), attention="se", use_mask=use_mask)
        m = net.MultiScaleAdaINRPNet(cfg, copy.deepcopy(net.vgg))
        ck = G.synth_model_(m, seed)
        n, _, h, w = shape
        c, s = synth.image(7400 + 2 * i, shape), synth.image(7401 + 2 * i, shape)
        kw = {}
        if use_mask:  # masks at twice the image size, greyscale files
            cfile = np.stack([GM.file_mask("blocks", 2 * h, 2 * w, 7510 + b, False)
                              for b in range(n)])
            sfile = np.stack([GM.file_mask("blocks", 2 * h, 2 * w, 7520 + b, True)
                              for b in range(n)])
            kw = dict(
                c_mask_path=[M.write_mask_png(os.path.join(tmp, f"se{i}_{b}_c.png"), cfile[b], "L")
                             for b in range(n)],
                s_mask_path=[M.write_mask_png(os.path.join(tmp, f"se{i}_{b}_s.png"), sfile[b], "L")
                             for b in range(n)])
            out.update({f"net{i}_cfile": cfile, f"net{i}_sfile": sfile})
        y = m.test(G.t(c), G.t(s), **kw).numpy()
        maps = attention_maps(m)
        m64 = copy.deepcopy(m).double()
        y64 = m64.test(G.t(c).double(), G.t(s).double(), **kw).numpy()
        names, shapes = S.key_table(m.state_dict())
        out.update({f"net{i}_hidden": hid, f"net{i}_blocks": blocks, f"net{i}_use_mask": use_mask,
                    f"net{i}_seed": seed, f"net{i}_checksum": ck, f"net{i}_content": c,
                    f"net{i}_style": s, f"net{i}_out": y, f"net{i}_maps": np.stack(maps),
                    f"net{i}_floor": helpers.rel_l2(y, y64),
                    f"net{i}_maps_floor": helpers.rel_l2(np.stack(maps),
                                                         np.stack(attention_maps(m64))),
                    f"net{i}_keys": names, f"net{i}_shapes": shapes})
        g = np.stack(maps)
        print(f"net {hid}x{blocks} mask={use_mask}: gates {g.min():.3f}..{g.max():.3f} "
              f"floor {out[f'net{i}_floor']:.2e}")
    out["n_net"] = len(NET_CASES)


def main():
    torch.set_num_threads(8)
    torch.manual_seed(0)
    net = G._import_reference()
    att = sys.modules["network.attention"]
    out = {}
    gen_modules(att, out)
    with tempfile.TemporaryDirectory() as tmp:
        gen_nets(net, tmp, out)
    helpers.save_golden("se", **out)
    print("SE goldens written to", HERE)


if __name__ == "__main__":
    main()
