"""Restatement of LDMSAdaINRPNet.forward (`network: ld_adain`, the training loss graph) in the
caller's dtype, written from the formulas of tests/ld_ref.py (not from the reference's
modules), for the ld_adain training tests and their goldens (tests/golden/grads_ld*.npz).

    cfs, sfs = levels(content), levels(style)            ld_ref.levels: cat([small_i, big_i])
    y = dec_0(AdaIN(c_{L-1}, s_{L-1}))
    y = dec_j(y + AdaIN(y, s_{L-1-j}))                    j = 1 .. L-1
    losses   = style loss at VGG relu1_1..relu4_1 of y against the style's, content loss of
               y's relu4_1 against the content's (oracle.restate._vgg_losses)

Only the top level's content features reach the loss; the lower content levels feed it through
the level above them only. grads() differentiates total_loss w.r.t. every rp_enc* / rp_dec*
tensor with the VGG frozen.
"""

import torch

import ld_ref as L
from oracle import restate as R

# (hidden, levels, inception, shape, model seed, content weight, style weight,
#  content / style image seeds of rpst.synth.image)
CASES = [
    (4, 3, 0, (2, 3, 24, 40), 95, 1.0, 10.0, 9101, 9201),
    (8, 3, 1, (1, 3, 17, 33), 92, 1.0, 1.0, 9101, 9201),
    (4, 4, 0, (1, 3, 20, 28), 93, 1.0, 3.0, 9102, 9202),
]


def config(hidden, layers, inception=0, cw=1.0, sw=10.0):
    return dict(L.config(hidden, layers, inception), content_weight=cw, style_weight=sw)


def golden_config(g, i):
    """The config of case i of tests/golden/grads_ld*.npz."""
    return config(int(g[f"hidden{i}"]), int(g[f"layers{i}"]), int(g[f"inception{i}"]),
                  float(g[f"cw{i}"]), float(g[f"sw{i}"]))


def losses(content, style, sd, layers, content_weight, style_weight):
    """The loss dict of LDMSAdaINRPNet.forward in content's dtype (sd in the same dtype)."""
    cfs, sfs = L.levels(content, sd, layers), L.levels(style, sd, layers)
    y = L.block(L.adain(cfs[-1], sfs[-1]), sd, "rp_dec0.")
    for j, sf in enumerate(sfs[:-1][::-1]):
        y = L.block(y + L.adain(y, sf), sd, f"rp_dec{j + 1}.")
    with torch.no_grad():
        c4 = R.encode_with_intermediate(content, sd)[-1]
    return R._vgg_losses(y, style, c4, sd, content_weight, style_weight)


def grads(content, style, sd, layers, content_weight, style_weight):
    """(loss dict, {name: d total_loss / d tensor}) over the rp_enc* / rp_dec* entries of sd,
    everything in content's dtype."""
    dt = content.dtype
    sd = {k: (v.detach().to(dt) if v.is_floating_point() else v) for k, v in sd.items()}
    return R.grads_of(losses, sd, ("rp_enc", "rp_dec"), content, style, layers, content_weight,
                      style_weight)
