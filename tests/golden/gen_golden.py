"""Generate golden vectors by running the REFERENCE network/ package on CPU.

Runs only in the build container, where /root/reference exists. The reference is
imported read-only (PYTHONDONTWRITEBYTECODE) with four stub modules for imports it
makes but never calls on the hot path:
  numpy.lib.arraypad (base.py:2), torchvision (base.py:11,15, adain_rp.py:12),
  seaborn (adain_rp.py:6, sanet.py:8), maxflow (utils/mst.py:3).
Nothing from the reference is copied: only inputs, outputs and weight checksums are
written, as .npz files next to this script. Weights come from rpst.synth (the same
generator the tests and bench use), so only the seed and a checksum are stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden.py
"""
from __future__ import annotations

import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REPO, "rp-style-transfer_amd"))
from rpst import synth  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import helpers  # noqa: E402  (tests/helpers.py: grad_probe, shared with the tests)


def _install_stubs():
    arraypad = types.ModuleType("numpy.lib.arraypad")
    arraypad.pad = np.pad
    sys.modules["numpy.lib.arraypad"] = arraypad
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    tv.models.inception = types.ModuleType("torchvision.models.inception")
    tv.transforms = types.ModuleType("torchvision.transforms")
    tv.transforms.ToPILImage = object
    tv.utils = types.ModuleType("torchvision.utils")
    sys.modules.update({"torchvision": tv, "torchvision.models": tv.models,
                        "torchvision.models.inception": tv.models.inception,
                        "torchvision.transforms": tv.transforms,
                        "torchvision.utils": tv.utils})
    sys.modules["seaborn"] = types.ModuleType("seaborn")
    mf = types.ModuleType("maxflow")
    mf.fastmin = types.ModuleType("maxflow.fastmin")
    mf.fastmin.aexpansion_grid = None
    sys.modules["maxflow"] = mf
    sys.modules["maxflow.fastmin"] = mf.fastmin


def _import_reference():
    _install_stubs()
    sys.path.insert(0, REF)
    import network as net  # noqa: F401  (the reference package)
    return net


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def synth_model_(model, seed):
    synth.synth_module_(model, seed)
    sd = {k: v.numpy() for k, v in model.state_dict().items()}
    return np.array(synth.checksum(sd))


def rand_feat(seed, shape, scale=1.0, offset=0.0, relu=False):
    u = synth.uniform01(seed, "feat", int(np.prod(shape))).reshape(shape)
    x = (2.0 * u - 1.0) * scale + offset
    if relu:
        x = np.maximum(x, 0.0)
    return x.astype(np.float32)


def gen_stats(net):
    out = {}
    shapes = [(2, 8, 16, 16), (1, 256, 32, 32), (3, 5, 7, 9), (1, 4, 1, 3), (2, 16, 64, 64)]
    for i, shp in enumerate(shapes):
        c = rand_feat(100 + i, shp, scale=2.0, offset=0.5)
        s = rand_feat(200 + i, shp, scale=3.0, offset=(50.0 if i == 4 else 1.0), relu=(i % 2 == 1))
        cm, cs = net.calc_mean_std(t(c))
        o = net.adaptive_instance_normalization(t(c), t(s))
        out[f"c{i}"] = c
        out[f"s{i}"] = s
        out[f"cmean{i}"] = cm.numpy()
        out[f"cstd{i}"] = cs.numpy()
        out[f"adain{i}"] = o.numpy()
    helpers.save_golden("stats", n=len(shapes), **out)  # (over 1 MiB: stored in parts)


def rp_config(hidden, blocks=5):
    return {"rp_blocks": blocks, "hidden_dim": hidden, "content_weight": 1.0,
            "style_weight": 10.0, "resume": False, "use_mask": False}


def gen_adain_rp(net):
    out = {}
    cases = [(2, (2, 3, 32, 32), 11), (16, (1, 3, 16, 16), 12), (16, (2, 3, 20, 28), 13),
             (4, (1, 3, 9, 13), 14)]
    for i, (hid, shp, seed) in enumerate(cases):
        vgg = copy.deepcopy(net.vgg)
        m = net.AdaINRPNet(rp_config(hid), vgg)
        ck = synth_model_(m, seed)
        c = synth.image(1000 + i, shp)
        s = synth.image(2000 + i, shp)
        y = m.test(t(c), t(s))
        out[f"hidden{i}"] = hid
        out[f"seed{i}"] = seed
        out[f"checksum{i}"] = ck
        out[f"content{i}"] = c
        out[f"style{i}"] = s
        out[f"out{i}"] = y.numpy()
        if i == 0:
            # per-layer intermediates for the first case (encoder + AdaIN + decoder)
            with torch.no_grad():
                cf = m.rp_shared_encoder(t(c))
                sf = m.rp_shared_encoder(t(s))
                fu = net.adaptive_instance_normalization(cf, sf)
            out["enc_c0"] = cf.numpy()
            out["enc_s0"] = sf.numpy()
            out["fused0"] = fu.numpy()
    np.savez_compressed(os.path.join(HERE, "adain_rp.npz"), n=len(cases), **out)


def gen_forward(net):
    out = {}
    vgg = copy.deepcopy(net.vgg)
    m = net.AdaINRPNet(rp_config(4), vgg)
    out["checksum"] = synth_model_(m, 21)
    c = synth.image(3000, (2, 3, 32, 32))
    s = synth.image(3001, (2, 3, 32, 32))
    with torch.no_grad():
        d, tot = m.forward(t(c), t(s))
        feats = m.encode_with_intermediate(t(c))
    out.update(content=c, style=s, style_loss=d["style_loss"].numpy(),
               content_loss=d["content_loss"].numpy(), total_loss=tot.numpy())
    for i, f in enumerate(feats):
        out[f"relu{i + 1}_1"] = f.numpy()
    np.savez_compressed(os.path.join(HERE, "forward.npz"), **out)


def spd(seed, n, rank=None):
    rank = rank or n
    a = synth.uniform01(seed, "spd", n * rank).reshape(n, rank) * 2 - 1
    return a @ a.T / rank


def gen_wct(net):
    from network.wct_rp import matrix_inv_sqrt, matrix_sqrt
    out = {}
    mats = [spd(1, 32), spd(2, 32, rank=8), spd(3, 64) * 100.0]
    for i, a in enumerate(mats):
        out[f"A{i}"] = a
        out[f"sqrt{i}"] = matrix_sqrt(t(a)).numpy()
        out[f"isqrt{i}"] = matrix_inv_sqrt(t(a)).numpy()
    vgg = copy.deepcopy(net.vgg)
    m = net.WCTRPNet(rp_config(2), vgg)
    cases = [(16, 256), (64, 1024), (32, 100)]
    for i, (cdim, hw) in enumerate(cases):
        cf = rand_feat(300 + i, (cdim, hw), scale=2.0, offset=0.3, relu=True).astype(np.float64)
        sf = rand_feat(400 + i, (cdim, hw), scale=1.5, offset=0.5, relu=True).astype(np.float64)
        if i == 2:
            sf[3] = 0.0  # a dead style channel -> singular style covariance
        out[f"cF{i}"] = cf
        out[f"sF{i}"] = sf
        out[f"wc{i}"] = m.whiten_and_color(t(cf), t(sf)).numpy()
    ncase = 0
    for i, (hid, shp, seed) in enumerate([(2, (1, 3, 32, 32), 31), (4, (2, 3, 24, 24), 32)]):
        vgg = copy.deepcopy(net.vgg)
        m = net.WCTRPNet(rp_config(hid), vgg)
        ck = synth_model_(m, seed)
        c = synth.image(4000 + i, shp)
        s = synth.image(5000 + i, shp)
        y = m.test(t(c), t(s))
        out[f"net_hidden{i}"] = hid
        out[f"net_seed{i}"] = seed
        out[f"net_checksum{i}"] = ck
        out[f"net_content{i}"] = c
        out[f"net_style{i}"] = s
        out[f"net_out{i}"] = y.numpy()
        ncase += 1
    helpers.save_golden("wct", nmat=len(mats), ncase=len(cases), nnet=ncase, **out)


def gen_wct_large(net):
    """The WCT matrix functions and whiten_and_color at the widths WCTRPNet runs at
    (C = 256: the RP encoder's output; 512: VGG relu4_1) on features conditioned like real
    activations (synth.conditioned_features: the style covariance spans ~6 decades before
    the reference's +1e-4). Outputs are stored as products with fixed +-1 probe matrices
    (and the first 32 columns of the fused feature), which pins them without storing
    C x C / C x HW fp64 arrays; the inputs are regenerated from the seeds."""
    from network.wct_rp import matrix_inv_sqrt, matrix_sqrt
    m = net.WCTRPNet(rp_config(2), copy.deepcopy(net.vgg))
    out = {}
    cases = [(256, 4096, 900), (512, 2048, 901)]
    for i, (cdim, hw, seed) in enumerate(cases):
        cf = synth.conditioned_features(seed, cdim, hw, 1.5)
        sf = synth.conditioned_features(seed + 50, cdim, hw, 3.0)
        sm = sf - sf.mean(1, keepdims=True)
        a = sm @ sm.T / (hw - 1)  # the reference's style covariance (wct_rp.py:92-94)
        pm = 2.0 * synth.uniform01(seed, "probe", cdim * 8).reshape(cdim, 8) - 1.0
        ph = 2.0 * synth.uniform01(seed, "hwprobe", hw * 4).reshape(hw, 4) - 1.0
        wc = m.whiten_and_color(t(cf), t(sf)).numpy()
        out.update({f"C{i}": cdim, f"HW{i}": hw, f"seed{i}": seed,
                    f"sqrtP{i}": matrix_sqrt(t(a)).numpy() @ pm,
                    f"isqrtP{i}": matrix_inv_sqrt(t(a)).numpy() @ pm,
                    f"wcP{i}": wc @ ph, f"wcCols{i}": wc[:, :32].copy()})
    np.savez_compressed(os.path.join(HERE, "wct_large.npz"), ncase=len(cases), **out)


def wct_edge_inputs():
    """Inputs of gen_wct_edge (regenerated by the tests): the matrix functions on inputs the
    Newton-Schulz path must hand to the SVD form, and whiten_and_color at C = 512 with a dead
    style channel and a style covariance reaching ~1e4 (the fixed 1e-10 residual
    bar failed such valid inputs)."""
    from rpst import synth
    mats = {}
    q = np.linalg.qr(2.0 * synth.uniform01(71, "edge_q", 24 * 24).reshape(24, 24) - 1.0)[0]
    ev = np.linspace(-3.0, 5.0, 24)  # indefinite symmetric
    mats["indef"] = q @ np.diag(ev) @ q.T
    q2 = np.linalg.qr(2.0 * synth.uniform01(72, "edge_q", 20 * 20).reshape(20, 20) - 1.0)[0]
    ev2 = np.concatenate([[-1e-4 + 4e-6, -1e-4 + 2e-6], np.linspace(0.05, 2.0, 18)])
    mats["trunc"] = q2 @ np.diag(ev2) @ q2.T  # A + 1e-4 I has two singular values < 1e-5
    mats["nonsym"] = 2.0 * synth.uniform01(73, "edge_ns", 16 * 16).reshape(16, 16) - 1.0 + 3.0 * np.eye(16)
    cdim, hw = 512, 1536
    cf = synth.conditioned_features(950, cdim, hw, 1.5) * 4.0
    sf = synth.conditioned_features(951, cdim, hw, 3.0) * 80.0
    sf[7] = 0.0  # dead style channel: singular style covariance
    ph = 2.0 * synth.uniform01(950, "hwprobe", hw * 4).reshape(hw, 4) - 1.0
    return mats, cf, sf, ph


def gen_wct_edge(net):
    from network.wct_rp import matrix_inv_sqrt, matrix_sqrt
    mats, cf, sf, ph = wct_edge_inputs()
    out = {}
    for k, a in mats.items():
        out[f"sqrt_{k}"] = matrix_sqrt(t(a)).numpy()
        out[f"isqrt_{k}"] = matrix_inv_sqrt(t(a)).numpy()
    m = net.WCTRPNet(rp_config(2), copy.deepcopy(net.vgg))
    wc = m.whiten_and_color(t(cf), t(sf)).numpy()
    sm = sf - sf.mean(1, keepdims=True)
    out["style_cov_max_eig"] = np.linalg.eigvalsh(sm @ sm.T / (sf.shape[1] - 1)).max()
    out["wcP"] = wc @ ph
    out["wcCols"] = wc[:, :32].copy()
    np.savez_compressed(os.path.join(HERE, "wct_edge.npz"), **out)


def wct_original_inputs():
    """Inputs of gen_wct_original (regenerated by the tests): whiten_and_color(method=
    'original') (Li et al., wct_rp.py:96-101) on small ReLU features, one with a dead style
    channel (singular style covariance: matrix_sqrt's SVD form at the 1e-4 floor), and at
    C = 256 on conditioned features (stored as probe products)."""
    from rpst import synth
    cases = []
    for i, (cdim, hw) in enumerate([(16, 256), (64, 1024), (32, 100)]):
        cf = rand_feat(600 + i, (cdim, hw), scale=2.0, offset=0.3, relu=True).astype(np.float64)
        sf = rand_feat(700 + i, (cdim, hw), scale=1.5, offset=0.5, relu=True).astype(np.float64)
        if i == 2:
            sf[5] = 0.0
        cases.append((cf, sf, None))
    cdim, hw = 256, 2048
    cf = synth.conditioned_features(960, cdim, hw, 1.5)
    sf = synth.conditioned_features(961, cdim, hw, 3.0)
    ph = 2.0 * synth.uniform01(960, "hwprobe", hw * 4).reshape(hw, 4) - 1.0
    cases.append((cf, sf, ph))
    return cases


def gen_wct_original(net):
    m = net.WCTRPNet(rp_config(2), copy.deepcopy(net.vgg))
    out = {}
    for i, (cf, sf, ph) in enumerate(wct_original_inputs()):
        wc = m.whiten_and_color(t(cf), t(sf), method='original').numpy()
        if ph is None:
            out[f"wc{i}"] = wc
        else:
            out[f"wcP{i}"] = wc @ ph
            out[f"wcCols{i}"] = wc[:, :32].copy()
    np.savez_compressed(os.path.join(HERE, "wct_original.npz"), **out)


def gen_sanet(net):
    from network.sanet import SANet, Transform, mean_variance_norm
    out = {}
    # SANet module at reduced width (in_planes is a constructor argument, sanet.py:74)
    for i, (b, cdim, h, w) in enumerate([(2, 32, 8, 8), (1, 64, 5, 7)]):
        mod = SANet(cdim)
        ck = synth_model_(mod, 50 + i)
        c = rand_feat(500 + i, (b, cdim, h, w), scale=2.0, offset=0.5, relu=True)
        s = rand_feat(600 + i, (b, cdim, h, w), scale=2.0, offset=0.5, relu=True)
        with torch.no_grad():
            y = mod(t(c), t(s))
            mvn = mean_variance_norm(t(c))
        out.update({f"sa_c{i}": c, f"sa_s{i}": s, f"sa_out{i}": y.numpy(), f"sa_ck{i}": ck,
                    f"sa_mvn{i}": mvn.numpy(), f"sa_seed{i}": 50 + i})
    tr = Transform(32)
    ck = synth_model_(tr, 60)
    c4 = rand_feat(700, (2, 32, 8, 8), relu=True)
    s4 = rand_feat(701, (2, 32, 8, 8), relu=True)
    c5 = rand_feat(702, (2, 32, 4, 4), relu=True)
    s5 = rand_feat(703, (2, 32, 4, 4), relu=True)
    with torch.no_grad():
        y = tr(t(c4), t(s4), t(c5), t(s5))
    out.update(tr_c4=c4, tr_s4=s4, tr_c5=c5, tr_s5=s5, tr_out=y.numpy(), tr_ck=ck)
    # full SAModel.test (in_planes fixed at 512, sanet.py:207)
    cfg = {"content_weight": 1.0, "style_weight": 3.0, "l_identity1_weight": 50.0,
           "l_identity2_weight": 1.0}
    for i, shp in enumerate([(1, 3, 32, 32), (2, 3, 48, 64)]):
        vgg = copy.deepcopy(net.vgg)
        m = net.SAModel(cfg, vgg, 0, shp[-1])
        ck = synth_model_(m, 70 + i)
        c = synth.image(6000 + i, shp)
        s = synth.image(7000 + i, shp)
        y = m.test(t(c), t(s))
        out.update({f"model_content{i}": c, f"model_style{i}": s, f"model_out{i}": y.numpy(),
                    f"model_ck{i}": ck, f"model_seed{i}": 70 + i})
    np.savez_compressed(os.path.join(HERE, "sanet.npz"), **out)


def gen_adaptive(net):
    """AdaptiveSANet / AdaptiveTransform / AdaptiveSAModel, both AEA
    modules. AdaptiveSAModel.test() draws seaborn heatmaps after the forward pass, so its
    output is produced by the same calls test() makes (encode style, encode content,
    fuse, decoder; sanet.py:336-341) without the plotting."""
    from network.sanet import (AdaptiveSANet, AdaptiveTransform, AEALReluModule, AEAModule,
                               cal_affinity_matrix)
    out = {}
    # affinity and the AEA modules at the function level
    c = rand_feat(800, (2, 16, 6, 8), scale=2.0, offset=0.3, relu=True)
    s = rand_feat(801, (2, 16, 6, 8), scale=2.0, offset=0.3, relu=True)
    c[0, :, 0, 0] = 0.0  # an all-zero position: normalize's 1e-12 floor
    aff = cal_affinity_matrix(t(c), t(s))
    out.update(aff_c=c, aff_s=s, aff_out=aff.numpy())
    for mode, cls in (("aea", AEAModule), ("relu", AEALReluModule)):
        mod = cls(48)
        ck = synth_model_(mod, 90 if mode == "aea" else 91)
        fx = torch.softmax(t(rand_feat(802, (2, 48, 48), scale=4.0)), dim=-1)
        with torch.no_grad():
            y, cl = mod(aff, fx)
        out.update({f"aea_{mode}_fx": fx.numpy(), f"aea_{mode}_out": y.numpy(),
                    f"aea_{mode}_clamp": cl.numpy(), f"aea_{mode}_ck": ck})
    for mode in ("aea", "relu"):
        for i, (b, cdim, h, w) in enumerate([(2, 32, 8, 8), (1, 64, 5, 7)]):
            mod = AdaptiveSANet(cdim, h * w, mode)
            seed = 92 + 2 * i + (mode == "relu")
            ck = synth_model_(mod, seed)
            c = rand_feat(810 + i, (b, cdim, h, w), scale=2.0, offset=0.5, relu=True)
            s = rand_feat(820 + i, (b, cdim, h, w), scale=2.0, offset=0.5, relu=True)
            with torch.no_grad():
                y = mod(t(c), t(s))
            out.update({f"asa_{mode}_c{i}": c, f"asa_{mode}_s{i}": s,
                        f"asa_{mode}_out{i}": y.numpy(), f"asa_{mode}_ck{i}": ck,
                        f"asa_{mode}_claim{i}": mod.claim_value.numpy(),
                        f"asa_{mode}_seed{i}": seed})
        tr = AdaptiveTransform(32, 64, 16, mode)
        ck = synth_model_(tr, 98 + (mode == "relu"))
        c4 = rand_feat(830, (2, 32, 8, 8), relu=True)
        s4 = rand_feat(831, (2, 32, 8, 8), relu=True)
        c5 = rand_feat(832, (2, 32, 4, 4), relu=True)
        s5 = rand_feat(833, (2, 32, 4, 4), relu=True)
        with torch.no_grad():
            y = tr(t(c4), t(s4), t(c5), t(s5))
        out.update({f"atr_{mode}_c4": c4, f"atr_{mode}_s4": s4, f"atr_{mode}_c5": c5,
                    f"atr_{mode}_s5": s5, f"atr_{mode}_out": y.numpy(), f"atr_{mode}_ck": ck})
        cfg = {"content_weight": 1.0, "style_weight": 3.0, "l_identity1_weight": 50.0,
               "l_identity2_weight": 1.0, "ada_module": mode, "output": "/nonexistent"}
        m = net.AdaptiveSAModel(cfg, copy.deepcopy(net.vgg), 0, 64)
        ck = synth_model_(m, 100 + (mode == "relu"))
        cimg = synth.image(9100, (1, 3, 64, 64))
        simg = synth.image(9200, (1, 3, 64, 64))
        m.eval()
        with torch.no_grad():
            sf = m.encode_with_intermediate(t(simg))
            cf = m.encode_with_intermediate(t(cimg))
            y = m.decoder(m.fuse(cf, sf))
        out.update({f"model_{mode}_content": cimg, f"model_{mode}_style": simg,
                    f"model_{mode}_out": y.numpy(), f"model_{mode}_ck": ck,
                    f"model_{mode}_seed": 100 + (mode == "relu")})
    np.savez_compressed(os.path.join(HERE, "adaptive.npz"), **out)


def gen_vgg(net):
    out = {}
    vgg = copy.deepcopy(net.vgg)
    ck = synth_model_(vgg, 80)
    x = synth.image(8000, (1, 3, 40, 40))
    with torch.no_grad():
        feats = []
        h = t(x)
        for lo, hi in [(0, 4), (4, 11), (11, 18), (18, 31), (31, 44)]:
            h = vgg[lo:hi](h)
            feats.append(h.numpy())
    dec = copy.deepcopy(net.decoder)
    dck = synth_model_(dec, 81)
    z = rand_feat(900, (1, 512, 5, 6), relu=True)
    with torch.no_grad():
        d = dec(t(z))
    out.update(x=x, vgg_ck=ck, dec_ck=dck, z=z, dec_out=d.numpy())
    for i, f in enumerate(feats):
        out[f"relu{i + 1}_1"] = f
    np.savez_compressed(os.path.join(HERE, "vgg.npz"), **out)


def multiscale_config(hidden, blocks=5, inception=0):
    cfg = rp_config(hidden, blocks)
    cfg.update({"shuffle": False, "shuffle_layers": 1, "sort": False,
                "stylized_layers": blocks, "enc_stack_way": "constant",
                "inception_num": inception, "attention": "none"})
    return cfg


def gen_multiscale(net):
    """MultiScaleAdaINRPNet.test, constant stack."""
    out = {}
    cases = [(8, 5, 0, (2, 3, 24, 32), 41), (32, 5, 0, (1, 3, 16, 16), 42),
             (8, 3, 1, (1, 3, 9, 13), 43)]
    for i, (hid, blocks, inc, shp, seed) in enumerate(cases):
        m = net.MultiScaleAdaINRPNet(multiscale_config(hid, blocks, inc), copy.deepcopy(net.vgg))
        ck = synth_model_(m, seed)
        c = synth.image(4100 + i, shp)
        s = synth.image(4200 + i, shp)
        y = m.test(t(c), t(s))
        out.update({f"hidden{i}": hid, f"blocks{i}": blocks, f"inception{i}": inc,
                    f"seed{i}": seed, f"checksum{i}": ck, f"content{i}": c, f"style{i}": s,
                    f"out{i}": y.numpy()})
    np.savez_compressed(os.path.join(HERE, "multiscale.npz"), n=len(cases), **out)


def gen_deeper(net):
    """MultiScaleAdaINRPNet.test, 'deeper' stack (rp_deeper_conv_blocks encoder with 1x1
    inception convs, rp_shallower_conv_blocks decoder; adain_rp.py:152-156 as configured by
    config/rl/train_deeper_multiscale_rp_adain.yaml:31-33, hidden 16, inception 3)."""
    out = {}
    cases = [(4, 5, 3, (1, 3, 24, 32), 44), (16, 5, 3, (1, 3, 16, 16), 45),
             (8, 3, 1, (2, 3, 9, 13), 46)]
    for i, (hid, blocks, inc, shp, seed) in enumerate(cases):
        cfg = multiscale_config(hid, blocks, inc)
        cfg["enc_stack_way"] = "deeper"
        m = net.MultiScaleAdaINRPNet(cfg, copy.deepcopy(net.vgg))
        ck = synth_model_(m, seed)
        c = synth.image(4300 + i, shp)
        s = synth.image(4400 + i, shp)
        y = m.test(t(c), t(s))
        out.update({f"hidden{i}": hid, f"blocks{i}": blocks, f"inception{i}": inc,
                    f"seed{i}": seed, f"checksum{i}": ck, f"content{i}": c, f"style{i}": s,
                    f"out{i}": y.numpy()})
    np.savez_compressed(os.path.join(HERE, "deeper.npz"), n=len(cases), **out)


def gen_grads(net):
    """Reference training gradients: AdaINRPNet.forward + total_loss.backward()
    (adain_rp.py:110-138, train.py:186-189) on CPU; the RP encoder / decoder parameter
    gradients (the VGG is frozen, adain_rp.py:27-29) and the loss values."""
    out = {}
    cases = [(4, (2, 3, 32, 32), 24, 1.0, 10.0), (16, (1, 3, 128, 128), 25, 1.0, 1.0)]
    for i, (hid, shp, seed, cw, sw) in enumerate(cases):
        cfg = rp_config(hid)
        cfg.update(content_weight=cw, style_weight=sw)
        m = net.AdaINRPNet(cfg, copy.deepcopy(net.vgg))
        ck = synth_model_(m, seed)
        c = synth.image(3100 + i, shp)
        s = synth.image(3200 + i, shp)
        m.zero_grad()
        d, tot = m.forward(t(c), t(s))
        tot.backward()
        out.update({f"hidden{i}": hid, f"seed{i}": seed, f"checksum{i}": ck, f"cw{i}": cw,
                    f"sw{i}": sw, f"content{i}": c, f"style{i}": s,
                    f"style_loss{i}": d["style_loss"].detach().numpy(),
                    f"content_loss{i}": d["content_loss"].detach().numpy(),
                    f"total_loss{i}": tot.detach().numpy()})
        names = []
        for name, p in m.named_parameters():
            if p.requires_grad:
                assert p.grad is not None, name
                out[f"grad{i}:{name}"] = p.grad.numpy()
                names.append(name)
            else:
                assert p.grad is None, name
        out[f"names{i}"] = np.array(names)
    helpers.save_golden("grads", n=len(cases), **out)


def gen_grads_wct(net):
    """Reference WCTRPNet.forward + total_loss.backward() (wct_rp.py:168-194): fuse()
    detaches the encoder features, so only RP decoder gradients exist."""
    out = {}
    cases = [(4, (2, 3, 32, 32), 26, 1.0, 1.0), (8, (1, 3, 48, 40), 27, 1.0, 10.0)]
    for i, (hid, shp, seed, cw, sw) in enumerate(cases):
        cfg = rp_config(hid)
        cfg.update(content_weight=cw, style_weight=sw)
        m = net.WCTRPNet(cfg, copy.deepcopy(net.vgg))
        ck = synth_model_(m, seed)
        c = synth.image(3300 + i, shp)
        s = synth.image(3400 + i, shp)
        m.zero_grad()
        d, tot = m.forward(t(c), t(s))
        tot.backward()
        out.update({f"hidden{i}": hid, f"seed{i}": seed, f"checksum{i}": ck, f"cw{i}": cw,
                    f"sw{i}": sw, f"content{i}": c, f"style{i}": s,
                    f"style_loss{i}": d["style_loss"].detach().numpy(),
                    f"content_loss{i}": d["content_loss"].detach().numpy(),
                    f"total_loss{i}": tot.detach().numpy()})
        names = []
        for name, p in m.named_parameters():
            if p.grad is not None:
                out[f"grad{i}:{name}"] = p.grad.numpy()
                names.append(name)
        out[f"names{i}"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "grads_wct.npz"), n=len(cases), **out)


SAM_CFG = {"content_weight": 1.0, "style_weight": 3.0, "l_identity1_weight": 50.0,
           "l_identity2_weight": 1.0}


def gen_grads_sam(net):
    """Reference SAModel.forward + total_loss.backward() (sanet.py:248-275; trainable: the
    transform and the decoder): the five losses and probes of every parameter gradient."""
    out = {}
    cases = [((1, 3, 64, 64), 28), ((2, 3, 64, 48), 29)]
    for i, (shp, seed) in enumerate(cases):
        m = net.SAModel(dict(SAM_CFG), copy.deepcopy(net.vgg), 0, shp[-1])
        m.decoder = copy.deepcopy(m.decoder)  # the module-level decoder is shared
        ck = synth_model_(m, seed)
        c = synth.image(3500 + i, shp)
        s = synth.image(3600 + i, shp)
        m.zero_grad()
        d, tot = m.forward(t(c), t(s))
        tot.backward()
        out.update({f"seed{i}": seed, f"checksum{i}": ck, f"content{i}": c, f"style{i}": s})
        for k, v in d.items():
            out[f"{k}{i}"] = v.detach().numpy()
        names = []
        for name, p in m.named_parameters():
            if p.grad is not None:
                out[f"gprobe{i}:{name}"] = helpers.grad_probe(name, p.grad.numpy())
                names.append(name)
        out[f"names{i}"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "grads_sam.npz"), n=len(cases), **out)


def gen_grads_adaptive(net):
    """Reference AdaptiveSAModel.forward + total_loss.backward() (sanet.py:347-382, trained by
    train.py:118-119's dynamic_sanet branch) for both AEA modules: the losses and probes of
    every transform (incl. f_psi) and decoder gradient. The forward's claim-map extraction
    (random index, .cpu().numpy()) has no effect on the losses."""
    out = {}
    cases = [("aea", (1, 3, 64, 64), 38), ("relu", (2, 3, 64, 64), 39)]
    for i, (mode, shp, seed) in enumerate(cases):
        m = net.AdaptiveSAModel(dict(SAM_CFG, ada_module=mode), copy.deepcopy(net.vgg), 0,
                                shp[-1])
        m.decoder = copy.deepcopy(m.decoder)  # the module-level decoder is shared
        ck = synth_model_(m, seed)
        c = synth.image(3700 + i, shp)
        s = synth.image(3800 + i, shp)
        m.zero_grad()
        d, tot = m.forward(t(c), t(s))
        tot.backward()
        out.update({f"mode{i}": mode, f"seed{i}": seed, f"checksum{i}": ck, f"content{i}": c,
                    f"style{i}": s})
        for k, v in d.items():
            out[f"{k}{i}"] = v.detach().numpy()
        names = []
        for name, p in m.named_parameters():
            if p.grad is not None:
                out[f"gprobe{i}:{name}"] = helpers.grad_probe(name, p.grad.numpy())
                names.append(name)
        out[f"names{i}"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "grads_adaptive.npz"), n=len(cases), **out)


def gen_sourcenet(net):
    """SourceNet.test, classic AdaIN on VGG relu4_1."""
    out = {}
    cases = [((1, 3, 32, 32), 51), ((2, 3, 24, 40), 52)]
    for i, (shp, seed) in enumerate(cases):
        m = net.SourceNet({"use_mask": False, "content_weight": 1.0, "style_weight": 10.0},
                          copy.deepcopy(net.vgg))
        ck = synth_model_(m, seed)
        c = synth.image(5100 + i, shp)
        s = synth.image(5200 + i, shp)
        y = m.test(t(c), t(s))
        out.update({f"seed{i}": seed, f"checksum{i}": ck, f"content{i}": c, f"style{i}": s,
                    f"out{i}": y.numpy()})
    np.savez_compressed(os.path.join(HERE, "sourcenet.npz"), n=len(cases), **out)


def gen_grads_src(net):
    """Reference SourceNet.forward + total_loss.backward() (base.py:624-649; only the
    decoder trains): the losses and probes of every decoder gradient."""
    out = {}
    cases = [((1, 3, 32, 32), 53, 1.0, 10.0), ((2, 3, 40, 48), 54, 1.0, 1.0)]
    for i, (shp, seed, cw, sw) in enumerate(cases):
        m = net.SourceNet({"use_mask": False, "content_weight": cw, "style_weight": sw},
                          copy.deepcopy(net.vgg))
        m.decoder = copy.deepcopy(m.decoder)  # the module-level decoder is shared
        ck = synth_model_(m, seed)
        c = synth.image(5300 + i, shp)
        s = synth.image(5400 + i, shp)
        m.zero_grad()
        d, tot = m.forward(t(c), t(s))
        tot.backward()
        out.update({f"seed{i}": seed, f"checksum{i}": ck, f"cw{i}": cw, f"sw{i}": sw,
                    f"content{i}": c, f"style{i}": s})
        for k, v in d.items():
            out[f"{k}{i}"] = v.detach().numpy()
        names = []
        for name, p in m.named_parameters():
            if p.grad is not None:
                out[f"gprobe{i}:{name}"] = helpers.grad_probe(name, p.grad.numpy())
                names.append(name)
        out[f"names{i}"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "grads_src.npz"), n=len(cases), **out)


def gen_grads_ms(net):
    """Reference MultiScaleAdaINRPNet.forward + total_loss.backward() (adain_rp.py:321-345):
    the constant stack with one inception conv per encoder block, and the 'deeper' stack of
    config/rl/train_deeper_multiscale_rp_adain.yaml (3 inception convs): the losses and every
    RP encoder / decoder gradient."""
    out = {}
    cases = [(8, 5, 1, "constant", (2, 3, 32, 32), 55, 1.0, 10.0),
             (4, 5, 3, "deeper", (1, 3, 48, 40), 56, 1.0, 1.0)]
    for i, (hid, blocks, inc, way, shp, seed, cw, sw) in enumerate(cases):
        cfg = multiscale_config(hid, blocks, inc)
        cfg.update(enc_stack_way=way, content_weight=cw, style_weight=sw)
        m = net.MultiScaleAdaINRPNet(cfg, copy.deepcopy(net.vgg))
        ck = synth_model_(m, seed)
        c = synth.image(5500 + i, shp)
        s = synth.image(5600 + i, shp)
        m.zero_grad()
        d, tot = m.forward(t(c), t(s))
        tot.backward()
        out.update({f"hidden{i}": hid, f"blocks{i}": blocks, f"inception{i}": inc,
                    f"way{i}": way, f"seed{i}": seed, f"checksum{i}": ck, f"cw{i}": cw,
                    f"sw{i}": sw, f"content{i}": c, f"style{i}": s})
        for k, v in d.items():
            out[f"{k}{i}"] = v.detach().numpy()
        names = []
        for name, p in m.named_parameters():
            if p.grad is not None:
                out[f"grad{i}:{name}"] = p.grad.numpy()
                names.append(name)
        out[f"names{i}"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "grads_ms.npz"), n=len(cases), **out)


def _reference_model(net, family, g, i):
    """The reference model of case i of golden file `family` (grads*.npz), synth weights."""
    if family in ("grads", "grads_wct"):
        cfg = dict(rp_config(int(g[f"hidden{i}"])), content_weight=float(g[f"cw{i}"]),
                   style_weight=float(g[f"sw{i}"]))
        m = (net.AdaINRPNet if family == "grads" else net.WCTRPNet)(cfg, copy.deepcopy(net.vgg))
    elif family in ("grads_sam", "grads_adaptive"):
        cfg = dict(SAM_CFG)
        if family == "grads_adaptive":
            cfg["ada_module"] = str(g[f"mode{i}"])
        cls = net.SAModel if family == "grads_sam" else net.AdaptiveSAModel
        m = cls(cfg, copy.deepcopy(net.vgg), 0, g[f"content{i}"].shape[-1])
        m.decoder = copy.deepcopy(m.decoder)
    elif family == "grads_src":
        m = net.SourceNet({"use_mask": False, "content_weight": float(g[f"cw{i}"]),
                           "style_weight": float(g[f"sw{i}"])}, copy.deepcopy(net.vgg))
        m.decoder = copy.deepcopy(m.decoder)
    else:  # grads_ms
        cfg = multiscale_config(int(g[f"hidden{i}"]), int(g[f"blocks{i}"]), int(g[f"inception{i}"]))
        cfg.update(enc_stack_way=str(g[f"way{i}"]), content_weight=float(g[f"cw{i}"]),
                   style_weight=float(g[f"sw{i}"]))
        m = net.MultiScaleAdaINRPNet(cfg, copy.deepcopy(net.vgg))
    ck = synth_model_(m, int(g[f"seed{i}"]))
    assert np.array_equal(ck, g[f"checksum{i}"]), (family, i)
    return m


FLOOR_SAMPLES = helpers.GRAD_FLOOR_SAMPLES
_ulp_perturbed = helpers.ulp_perturbed


def gen_grad_floors(net):
    """The reference's own fp32 noise floor of every training-gradient golden (VERDICT r05
    item 4). Each case of grads / grads_wct / grads_sam / grads_src / grads_ms /
    grads_adaptive runs through the REFERENCE model in fp32 and in float64 (m.double(),
    float64 inputs) on FLOOR_SAMPLES inputs: the golden's own (its fp32 run reproduces the
    committed golden; checked) and FLOOR_SAMPLES - 1 copies moved by one fp32 ulp per
    element. Stored per gradient tensor: the floor, the RMS over the samples of the
    whole-tensor rel-L2(fp32, float64) -- one sample is rounding luck: on the ill-conditioned
    SANet f / g gradients (unscaled softmax logits spanning ~100 per row, ~1e3 x
    amplification of the frozen VGG features' rounding) single samples spread over an order
    of magnitude -- and the unperturbed float64 gradient's probe (helpers.grad_probe), which
    pins the oracle's float64 gradients to the reference's at test time. Per loss: the RMS
    rel-L2. (A probe difference is not a floor: a random rounding error of relative norm e
    moves a probe by only ~e / sqrt(n).) The GPU tests hold each gradient tensor to
    max(1e-4, 3 x its floor) in full-tensor rel-L2."""
    out = {}
    for family in ("grads", "grads_wct", "grads_sam", "grads_src", "grads_ms",
                   "grads_adaptive"):
        g = helpers.load_golden(family)
        for i in range(int(g["n"])):
            names = [str(n) for n in g[f"names{i}"]]
            sq, lsq = {}, {}
            for smp in range(FLOOR_SAMPLES):
                c, s = g[f"content{i}"], g[f"style{i}"]
                if smp:
                    c, s = _ulp_perturbed(c, 7000 + 2 * smp), _ulp_perturbed(s, 7001 + 2 * smp)
                res = {}
                for dt in (torch.float32, torch.float64):
                    m = _reference_model(net, family, g, i).to(dt)
                    if family == "grads_wct" and dt == torch.float64:
                        # fuse() returns .float() (wct_rp.py:166): widen it back
                        m.fuse = (lambda mm: lambda a, b: type(mm).fuse(mm, a, b).double())(m)
                    m.zero_grad()
                    d, tot = m.forward(t(c).to(dt), t(s).to(dt))
                    tot.backward()
                    res[dt] = ({k: v.detach() for k, v in d.items()},
                               {k: p.grad.detach() for k, p in m.named_parameters()
                                if p.grad is not None})
                (l32, g32), (l64, g64) = res[torch.float32], res[torch.float64]
                for k in l64:
                    if f"{k}{i}" in g:
                        if smp == 0:
                            assert helpers.rel_l2(l32[k], g[f"{k}{i}"]) == 0.0, (family, i, k)
                        lsq[k] = lsq.get(k, 0.0) + helpers.rel_l2(l32[k], l64[k]) ** 2
                for name in names:
                    if smp == 0:  # the fp32 run reproduces the golden
                        if f"grad{i}:{name}" in g:
                            assert helpers.rel_l2(g32[name], g[f"grad{i}:{name}"]) == 0.0
                        else:
                            assert np.array_equal(helpers.grad_probe(name, g32[name]),
                                                  g[f"gprobe{i}:{name}"])
                        out[f"{family}/{i}/p64:{name}"] = helpers.grad_probe(name, g64[name])
                        out[f"{family}/{i}/s0:{name}"] = np.array(helpers.rel_l2(g32[name], g64[name]))
                    sq[name] = sq.get(name, 0.0) + helpers.rel_l2(g32[name], g64[name]) ** 2
            for k, v in lsq.items():
                out[f"{family}/{i}/loss:{k}"] = np.array(np.sqrt(v / FLOOR_SAMPLES))
            for name in names:
                out[f"{family}/{i}:{name}"] = np.array(np.sqrt(sq[name] / FLOOR_SAMPLES))
            print(family, i, "worst floor", max(float(v) for k, v in out.items()
                                                if k.startswith(f"{family}/{i}:")
                                                and not k.endswith("g.bias")), flush=True)
    np.savez_compressed(os.path.join(HERE, "grad_floors.npz"), **out)


FSCALES = (1.0, 0.5, 0.3, 0.2, 0.15, 0.1)


def scan_adaptive_fscale(net):
    """python gen_golden.py fscale_scan: how live the AEA clamp of the reference
    AdaptiveSAModel ('aea', 64 x 64, seed 40, images 3702 / 3802) is, and what its f_psi
    gradients' fp32 floors are (gen_grad_floors' RMS over FLOOR_SAMPLES inputs), with the
    query convs transform.sanet4_1.f and sanet5_1.f scaled by each of FSCALES after the
    synthetic weights: the table behind the choice of a live grads_adaptive case
    (profiles/aea_live/fscale_scan.txt). Liveness (helpers.clamp_liveness) is of sanet4_1,
    from the float64 oracle on the same weights. Writes no golden."""
    sys.path.insert(0, REPO)
    from oracle import restate as R
    shp, seed = (1, 3, 64, 64), 40
    c0, s0 = synth.image(3702, shp), synth.image(3802, shp)
    print("fscale  live4_1  median max P   worst f_psi floor (RMS)   worst other floor")
    for fs in FSCALES:
        def model(dt):
            m = net.AdaptiveSAModel(dict(SAM_CFG, ada_module="aea"), copy.deepcopy(net.vgg), 0,
                                    shp[-1])
            m.decoder = copy.deepcopy(m.decoder)
            synth_model_(m, seed)
            with torch.no_grad():
                for sa in (m.transform.sanet4_1, m.transform.sanet5_1):
                    sa.f.weight *= fs
                    sa.f.bias *= fs
            return m.to(dt)
        sd = {k: v.detach().double() for k, v in model(torch.float32).state_dict().items()}
        with torch.no_grad():
            cf = R.encode_with_intermediate(t(c0).double(), sd, 5)[3]
            sf = R.encode_with_intermediate(t(s0).double(), sd, 5)[3]
            pre = "transform.sanet4_1."
            Fm = R.conv(R.mean_variance_norm(cf), sd, pre + "f", "none", False).flatten(2)
            Gm = R.conv(R.mean_variance_norm(sf), sd, pre + "g", "none", False).flatten(2)
            P = torch.softmax(torch.bmm(Fm.transpose(1, 2), Gm), -1)
            clamp = R.adaptive_sanet(cf, sf, sd, pre, "aea")[1]
        sq = {}
        for smp in range(FLOOR_SAMPLES):
            c, s = c0, s0
            if smp:
                c, s = _ulp_perturbed(c, 7000 + 2 * smp), _ulp_perturbed(s, 7001 + 2 * smp)
            res = {}
            for dt in (torch.float32, torch.float64):
                m = model(dt)
                m.zero_grad()
                m.forward(t(c).to(dt), t(s).to(dt))[1].backward()
                res[dt] = {k: p.grad.detach() for k, p in m.named_parameters()
                           if p.grad is not None}
            for k, g64 in res[torch.float64].items():
                sq[k] = sq.get(k, 0.0) + helpers.rel_l2(res[torch.float32][k], g64) ** 2
        fl = {k: float(np.sqrt(v / FLOOR_SAMPLES)) for k, v in sq.items()
              if not k.endswith("g.bias")}
        print(f"{fs:6.2f}  {helpers.clamp_liveness(P, clamp, 'aea'):7.3f}  "
              f"{float(P.amax(-1).median()):12.3f}   "
              f"{max(v for k, v in fl.items() if 'f_psi' in k):23.3e}   "
              f"{max(v for k, v in fl.items() if 'f_psi' not in k):17.3e}", flush=True)


def gen_keys(net):
    """state_dict key/shape lists of the reference models (checkpoint compatibility)."""
    import json
    vgg = copy.deepcopy(net.vgg)
    models = {
        "AdaINRPNet": net.AdaINRPNet(rp_config(16), vgg),
        "WCTRPNet": net.WCTRPNet(rp_config(16), vgg),
        "SAModel": net.SAModel({}, vgg, 0, 512),
        "MultiScaleAdaINRPNet": net.MultiScaleAdaINRPNet(multiscale_config(32, 5, 0), vgg),
        "MultiScaleAdaINRPNet_inception1": net.MultiScaleAdaINRPNet(
            multiscale_config(16, 4, 1), vgg),
        "SourceNet": net.SourceNet({"use_mask": False}, vgg),
        "AdaptiveSAModel_aea": net.AdaptiveSAModel({"ada_module": "aea"}, vgg, 0, 512),
        "AdaptiveSAModel_relu": net.AdaptiveSAModel({"ada_module": "relu"}, vgg, 0, 512),
        "vgg": net.vgg,
        "decoder": net.decoder,
    }
    out = {k: [[n, list(v.shape)] for n, v in m.state_dict().items()] for k, m in models.items()}
    with open(os.path.join(HERE, "keys.json"), "w") as f:
        json.dump(out, f, indent=0)


GENERATORS = {"keys": gen_keys, "stats": gen_stats, "adain_rp": gen_adain_rp,
              "forward": gen_forward, "wct": gen_wct, "sanet": gen_sanet, "vgg": gen_vgg,
              "multiscale": gen_multiscale, "sourcenet": gen_sourcenet,
              "adaptive": gen_adaptive, "deeper": gen_deeper, "grads": gen_grads,
              "grads_wct": gen_grads_wct, "wct_large": gen_wct_large,
              "grads_sam": gen_grads_sam, "grads_src": gen_grads_src,
              "grads_ms": gen_grads_ms, "wct_edge": gen_wct_edge,
              "grads_adaptive": gen_grads_adaptive, "wct_original": gen_wct_original,
              "grad_floors": gen_grad_floors}


def main():
    """python gen_golden.py [name ...]  (default: all; fscale_scan only by name)"""
    torch.set_num_threads(8)
    torch.manual_seed(0)
    net = _import_reference()
    for name in (sys.argv[1:] or list(GENERATORS)):
        dict(GENERATORS, fscale_scan=scan_adaptive_fscale)[name](net)
    print("goldens written to", HERE)


if __name__ == "__main__":
    main()
