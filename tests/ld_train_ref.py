"""Restatement of LDMSAdaINRPNet.forward (`network: ld_adain`, the training loss graph) in the
caller's dtype, written from the formulas of tests/ld_ref.py (not from the reference's
modules), for the ld_adain training tests and their goldens (tests/golden/grads_ld*.npz).

    cfs, sfs = levels(content), levels(style)            ld_ref: cat([small_i, big_i])
    y = dec_0(AdaIN(c_{L-1}, s_{L-1}))
    y = dec_j(y + AdaIN(y, s_{L-1-j}))                    j = 1 .. L-1
    losses   = style loss at VGG relu1_1..relu4_1 of y against the style's, content loss of
               y's relu4_1 against the content's (oracle.restate._vgg_losses)

Only the top level's content features reach the loss; the lower content levels feed it through
the level above them only. grads() differentiates total_loss w.r.t. every rp_enc* / rp_dec*
tensor with the VGG frozen.
"""
import torch
import torch.nn.functional as F

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


def block(x, sd, prefix, pad_mode="reflect"):
    """A Conv2dBlock from its state_dict entries under `prefix`, in x's dtype: pad k // 2,
    conv, the 1x1 inception convs, LeakyReLU(0.2) once at the end."""
    y = L.conv_pad(x, sd[prefix + "conv.weight"], sd[prefix + "conv.bias"], pad_mode)
    j = 0
    while f"{prefix}inception.{j}.0.weight" in sd:
        y = F.conv2d(y, sd[f"{prefix}inception.{j}.0.weight"], sd[f"{prefix}inception.{j}.0.bias"])
        j += 1
    return torch.where(y > 0, y, 0.2 * y)


def levels(x, sd, layers):
    feats = []
    for i in range(layers):
        x = torch.cat([block(x, sd, f"rp_enc{i}_small_revf."),
                       block(x, sd, f"rp_enc{i}_big_revf.")], dim=1)
        feats.append(x)
    return feats


def losses(content, style, sd, layers, content_weight, style_weight):
    """The loss dict of LDMSAdaINRPNet.forward in content's dtype (sd in the same dtype)."""
    cfs, sfs = levels(content, sd, layers), levels(style, sd, layers)
    y = block(L.adain(cfs[-1], sfs[-1]), sd, "rp_dec0.")
    for j, sf in enumerate(sfs[:-1][::-1]):
        y = block(y + L.adain(y, sf), sd, f"rp_dec{j + 1}.")
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
