"""SE channel attention (`attention: se`, reference network/attention.py:5-66 behind
network/base.py:177-198) on the GPU: the gate kernel and the gated conv epilogue against
float64, one SE block and MultiScaleAdaINRPNet.test() against the reference's recorded outputs
(tests/golden/se.npz, gen_golden_se.py), the fused path against the op-by-op one, the folded
weight cache, the inference-only errors, the stylize pipeline and the launch sequence.

Bars: 1e-5 rel-L2 per conv and per block (the project's per-conv bar), TOL_STATS for gates and
statistics, TOL_NET / TOL_NET_MAXABS end to end (tests/helpers.py)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import masked_ref as M
import se_ref as S
from helpers import (TOL_NET, TOL_STATS, check_net, check_pipeline, dataset_tree, dev, gen,
                     golden_net, mask_kw, multiscale_config, rel_l2, synth_, traced_launches,
                     unfused)

pytestmark = pytest.mark.gpu


# ---- the gate -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 16, 1), (3, 32, 2), (2, 48, 3), (2, 128, 8)])
def test_se_gate_vs_float64(cuda, shape):
    from rpst import ops
    n, c, r = shape
    m = gen(100, (n, c), 1.0, 0.5)
    w3 = gen(101, (c, c), (3.0 / c) ** 0.5)
    b3 = gen(102, (c,), 0.25)
    fa = gen(103, (r, c), 1.0 / c ** 0.5)
    fb = gen(104, (c, r), 1.0 / r ** 0.5)
    if n > 1:
        # the last image: p = w3 m + b3 all negative under non-negative squeeze weights, so
        # relu gives 0 and every gate of the row is exactly 0.5
        fa = fa.abs()
        target = -(gen(105, (c,)).abs().double() + 0.5)
        m[n - 1] = torch.linalg.solve(w3.double(), target - b3.double()).float()
        p = w3.double() @ m[n - 1].double() + b3.double()
        assert float(p.max()) < -0.1
    p = m.double() @ w3.double().t() + b3.double()
    ref = torch.sigmoid(torch.relu(p @ fa.double().t()) @ fb.double().t())
    gate = ops.se_gate(*(t.to(cuda) for t in (m, w3, b3, fa, fb)))
    assert tuple(gate.shape) == (n, c) and gate.dtype == torch.float32
    err = rel_l2(gate, ref)
    print(f"se_gate {shape}: rel-L2 {err:.3e}")
    assert err < TOL_STATS
    assert float((gate.cpu().double() - ref).abs().max()) < 1e-6
    if n > 1:
        assert torch.equal(gate[n - 1].cpu(), torch.full((c,), 0.5))
        assert not torch.equal(gate[0].cpu(), torch.full((c,), 0.5))
    # (N, C, 1, 1) statistics, as conv2d_stats returns them, are taken as they are
    again = ops.se_gate(m.to(cuda).view(n, c, 1, 1), *(t.to(cuda) for t in (w3, b3, fa, fb)))
    assert torch.equal(again, gate)


# ---- the gated conv -----------------------------------------------------------------------
@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", [(24, 40), (13, 9), (33, 17)])
@pytest.mark.parametrize("c", [16, 32, 48, 128])
def test_conv2d_gated_vs_float64(cuda, c, hw, n, stats):
    """out = relu(gate * (conv1x1(x) + b) + residual), gates holding exact 0 and 1, a residual
    with negative entries so the ReLU clips; with statistics, calc_mean_std of out. Image k of
    a batch equals the same image run alone, bit for bit."""
    from rpst import ops
    h, w = hw
    x = gen(110, (n, c, h, w))
    wt = gen(111, (c, c, 1, 1), (3.0 / c) ** 0.5)
    b = gen(112, (c,), 0.1)
    gate = gen(113, (n, c), 0.5, 0.5)
    gate[0, 0], gate[0, 1] = 0.0, 1.0
    res = gen(114, (n, c, h, w), 1.5, -0.25)
    u = F.conv2d(x.double(), wt.double(), b.double())
    ref = torch.relu(gate.double()[:, :, None, None] * u + res.double())
    xd, gd, rd, bd = x.to(cuda), gate.to(cuda), res.to(cuda), b.to(cuda)
    pk = ops.pack_conv_weight(wt.to(cuda))
    got = ops.conv2d_gated(xd, pk, bd, gd, rd, c, 1, stats=stats)
    out = got[0] if stats else got
    err = rel_l2(out, ref)
    print(f"conv2d_gated C{c} {h}x{w} N{n} stats={stats}: rel-L2 {err:.3e}")
    assert err < 1e-5
    assert (out == 0).any() and (out > 0).any()           # the final ReLU clips
    assert torch.equal(out[0, 0], torch.relu(rd[0, 0]))   # gate 0: the residual alone
    assert rel_l2(out[0, 1], torch.relu(u[0, 1] + res[0, 1].double())) < 1e-5  # gate 1
    if stats:
        mean, std = got[1], got[2]
        assert tuple(mean.shape) == tuple(std.shape) == (n, c, 1, 1)
        rm = ref.mean(dim=(2, 3), keepdim=True)
        rs = torch.sqrt(ref.var(dim=(2, 3), unbiased=True, keepdim=True) + 1e-5)
        em, es = rel_l2(mean, rm), rel_l2(std, rs)
        print(f"  mean {em:.3e} std {es:.3e}")
        assert em < TOL_STATS and es < TOL_STATS
        # the statistics form writes the same output as the plain form
        assert torch.equal(out, ops.conv2d_gated(xd, pk, bd, gd, rd, c, 1))
    for k in range(n if n > 1 else 0):
        one = ops.conv2d_gated(xd[k:k + 1], pk, bd, gd[k:k + 1], rd[k:k + 1], c, 1, stats=stats)
        if stats:
            assert torch.equal(one[1], mean[k:k + 1]) and torch.equal(one[2], std[k:k + 1]), k
            one = one[0]
        assert torch.equal(one, out[k:k + 1]), k


def test_conv2d_gated_rejects_what_is_not_built(cuda):
    from rpst import _lib, ops
    x = torch.zeros((1, 16, 8, 8), device=cuda)
    g = torch.zeros((1, 16), device=cuda)
    pk = ops.pack_conv_weight(torch.zeros((16, 16, 3, 3), device=cuda))
    with pytest.raises(_lib.RpstError, match="1x1"):
        ops.conv2d_gated(x, pk, None, g, x, 16, 3)
    with pytest.raises(ValueError, match="gate"):
        ops.conv2d_gated(x, pk, None, torch.zeros((2, 16), device=cuda), x, 16, 1)


# ---- one SE block ---------------------------------------------------------------------------
def _module(g, i, cuda):
    import network as net
    C = g[f"mod{i}_x"].shape[1]
    blk = net.SEBottleneck(C, C)
    assert np.array_equal(S.synth_block_(blk, int(g[f"mod{i}_seed"])), g[f"mod{i}_checksum"])
    sd = {k: v.clone() for k, v in blk.state_dict().items()}
    return blk.eval().to(cuda), sd


@pytest.mark.parametrize("i", [0, 1, 2])
def test_se_bottleneck_module_goldens(cuda, golden, i):
    from rpst import ops
    g = golden("se")
    blk, sd = _module(g, i, cuda)
    x = dev(g[f"mod{i}_x"], cuda)
    ref, ref_gate = S.se_block(g[f"mod{i}_x"], sd)
    with torch.no_grad():
        out, gate = ops.se_bottleneck(x, blk)
        out_s, gate_s, mean, std = ops.se_bottleneck(x, blk, stats=True)
        via_module = blk(x)
    n, C = x.shape[:2]
    assert tuple(gate.shape) == (n, C, 1, 1)
    e_out, e_ref = rel_l2(out, ref), rel_l2(out, g[f"mod{i}_out"])
    e_gate = rel_l2(gate, g[f"mod{i}_gate"])
    print(f"se_bottleneck {tuple(x.shape)}: out vs float64 {e_out:.3e} vs reference {e_ref:.3e} "
          f"gate {e_gate:.3e}")
    assert e_out < 1e-5 and e_ref < 1e-5
    assert e_gate < TOL_STATS and rel_l2(gate, ref_gate) < TOL_STATS
    assert torch.equal(out_s, out) and torch.equal(gate_s, gate)
    assert torch.equal(via_module, out) and torch.equal(blk.attention_map, gate)
    assert torch.equal(blk.se.attention_map, gate)
    rm = ref.mean(dim=(2, 3), keepdim=True)
    rs = torch.sqrt(ref.var(dim=(2, 3), unbiased=True, keepdim=True) + 1e-5)
    assert rel_l2(mean, rm) < TOL_STATS and rel_l2(std, rs) < TOL_STATS
    # x is the residual and must come back untouched
    assert torch.equal(x, dev(g[f"mod{i}_x"], cuda))


# ---- networks -------------------------------------------------------------------------------
def _net(g, i, cuda, seed=None):
    import network as net
    return golden_net(net.MultiScaleAdaINRPNet, S.golden_config(g, i), g, f"net{i}_", cuda, seed)


def _check_maps(m, g, i, n, what):
    ref = g[f"net{i}_maps"]
    assert len(m.rp_shared_encoder) == ref.shape[0]
    for k, blk in enumerate(m.rp_shared_encoder):
        am = blk.attention_map
        assert tuple(am.shape) == (n, int(g[f"net{i}_hidden"]), 1, 1), (what, k)
        err = rel_l2(am, ref[k])
        assert err < TOL_NET, (what, k, err)
    for blk in m.rp_decoder:
        assert blk.attention_block is None and blk.attention_map is None


@pytest.mark.parametrize("i", [0, 1, 2])
def test_multiscale_se_goldens(cuda, golden, tmp_path, i):
    """MultiScaleAdaINRPNet.test() with `attention: se` (case 1: with `use_mask: True`, the
    flagship YAML's pair) against the reference: the image, and every encoder block's
    attention_map = the style images' gates. Then the op-by-op path (FUSED_ADAIN off): within
    1e-5 of the fused one, and equal bit for bit to decode() on encode_rp_intermediate()."""
    import network.adain_rp as arp
    g = golden("se")
    m = _net(g, i, cuda)
    c, s = dev(g[f"net{i}_content"], cuda), dev(g[f"net{i}_style"], cuda)
    n = c.shape[0]
    kw = mask_kw(g, f"net{i}_", cuda, tmp_path)
    y = m.test(c, s, **kw)
    check_net(y, g[f"net{i}_out"], f"multiscale se case {i} fused")
    _check_maps(m, g, i, n, "fused")
    fused_maps = [blk.attention_map.clone() for blk in m.rp_shared_encoder]
    assert torch.equal(m.test(c, s, **kw), y)
    with unfused(arp, "FUSED_ADAIN"):
        plain = m.test(c, s, **kw)
    check_net(plain, g[f"net{i}_out"], f"multiscale se case {i} op-by-op")
    _check_maps(m, g, i, n, "op-by-op")
    assert rel_l2(y, plain) < 1e-5
    for a, blk in zip(fused_maps, m.rp_shared_encoder):
        assert rel_l2(a, blk.attention_map) < TOL_STATS
    m.eval()
    with torch.no_grad():
        cf, sf = m.encode_rp_intermediate(c), m.encode_rp_intermediate(s)
        dec = m.decode(cf, sf, use_mask=bool(g[f"net{i}_use_mask"]), **kw)
    assert torch.equal(dec, plain)


def test_flagship_options_construct_and_run(cuda):
    """The model options of config/rl/train_constant_multiscale_rp_adain.yaml: multi_adain,
    constant stack, hidden 32, 5 blocks, attention se, use_mask True."""
    import network as net
    from rpst import synth
    cfg = dict(multiscale_config(32, 5, 0), attention="se", use_mask=True)
    m = net.MultiScaleAdaINRPNet(cfg, copy.deepcopy(net.vgg))
    synth_(m, 4)
    m = m.to(cuda)
    c = torch.from_numpy(synth.image(1, (1, 3, 40, 72))).to(cuda)
    s = torch.from_numpy(synth.image(2, (1, 3, 40, 72))).to(cuda)
    seg = torch.from_numpy(M.blocks_mask(40, 72, [0, 60, 120], 3))[None].to(cuda)
    y = m.test(c, s, c_mask_path=seg, s_mask_path=seg)
    assert tuple(y.shape) == (1, 3, 40, 72) and bool(torch.isfinite(y).all())
    assert m.training  # test() leaves the model in training mode, as the reference does


def test_models_without_attention_unchanged(cuda):
    """attention 'none' never touches the SE path: no attention block, no attention map, and
    the fused and op-by-op paths agree as before."""
    import network as net
    import network.adain_rp as arp
    from rpst import synth
    m = net.MultiScaleAdaINRPNet(multiscale_config(16, 3, 0), copy.deepcopy(net.vgg))
    synth_(m, 9)
    m = m.to(cuda)
    assert not m._has_attention()
    c = torch.from_numpy(synth.image(41, (2, 3, 24, 40))).to(cuda)
    s = torch.from_numpy(synth.image(42, (2, 3, 24, 40))).to(cuda)
    y = m.test(c, s)
    with unfused(arp, "FUSED_ADAIN"):
        plain = m.test(c, s)
    assert rel_l2(y, plain) < 1e-5
    assert all(b.attention_map is None for b in m.rp_shared_encoder)


# ---- the folded-weight cache ----------------------------------------------------------------
def test_fold_cache_follows_load_state_dict_and_to(cuda, golden):
    from rpst import plan
    g = golden("se")
    m = _net(g, 2, cuda)
    c, s = dev(g["net2_content"], cuda), dev(g["net2_style"], cuda)
    y1 = m.test(c, s)
    blk = m.rp_shared_encoder[0].attention_block
    cached = plan.se_folded(blk)
    assert plan.se_folded(blk) is cached  # unchanged weights: the cached operands
    fresh = _net(g, 2, cuda, seed=73)
    m.load_state_dict(fresh.state_dict())
    assert plan.se_folded(blk) is not cached
    y2 = m.test(c, s)
    assert not torch.equal(y2, y1)
    assert torch.equal(y2, fresh.test(c, s))
    # a BatchNorm statistic alone changing refreshes the fold too
    before = plan.se_folded(blk)
    with torch.no_grad():
        blk.bn2.running_var.mul_(1.5)
    assert plan.se_folded(blk) is not before
    y3 = m.test(c, s)
    assert not torch.equal(y3, y2)
    # .to(): new storage, same values -> the same bits from freshly folded operands
    before = plan.se_folded(blk)
    m = m.cpu().to(cuda)
    assert plan.se_folded(m.rp_shared_encoder[0].attention_block) is not before
    assert torch.equal(m.test(c, s), y3)


# ---- inference only -------------------------------------------------------------------------
def test_se_training_paths_raise(cuda, golden):
    import network as net
    g = golden("se")
    m = _net(g, 2, cuda)
    c, s = dev(g["net2_content"], cuda), dev(g["net2_style"], cuda)
    assert torch.is_grad_enabled()
    with pytest.raises(NotImplementedError, match="inference only"):
        m(c, s)
    blk = net.SEBottleneck(16, 16).to(cuda)
    with pytest.raises(NotImplementedError, match="training-mode BatchNorm"):
        blk(torch.zeros((1, 16, 8, 8), device=cuda))
    cb = net.Conv2dBlock(3, 16, 3, 1, padding=1, attention="se").to(cuda)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="training-mode BatchNorm"):
        cb(c)
    with torch.no_grad():
        y = cb.eval()(c)
    assert tuple(y.shape) == (c.shape[0], 16) + tuple(c.shape[2:])
    assert tuple(cb.attention_map.shape) == (c.shape[0], 16, 1, 1)


# ---- launches -------------------------------------------------------------------------------
def test_se_block_launch_sequence(cuda, golden):
    """One SE block is four library calls -- conv1, conv2 with the statistics epilogue (its
    merge inside the call), the gate, the gated conv (with its merge when statistics are
    asked for) -- and nothing elementwise: the trace hook (rpst.ops.TRACE, which
    tools/per_layer.py reads) names every call the block makes."""
    from rpst import ops
    g = golden("se")
    blk, _ = _module(g, 0, cuda)
    x = dev(g["mod0_x"], cuda)
    for stats in (False, True):
        with torch.no_grad():
            ops.se_bottleneck(x, blk, stats=stats)  # warm: the fold and its packing are cached
            names, _ = traced_launches(lambda: ops.se_bottleneck(x, blk, stats=stats))
        kinds = [nm.split(" ")[0] for nm in names]
        assert kinds == ["conv1x1", "wino43x3", "se_gate", "gated1x1"], names
        assert all("32->32 24x40 N2" in nm for nm in (names[0], names[1], names[3])), names


# ---- pipeline -------------------------------------------------------------------------------
def test_pipeline_with_se_and_masks(cuda, tmp_path):
    """stylize.py with a YAML carrying `attention: se`, `use_mask: True` and
    --synthetic-weights: the outputs it writes are the direct test() call's. The pipeline
    resizes every image to (img_size, img_size), as the reference's does, so it runs at 40x40."""
    root = str(tmp_path / "data")
    # images 48 -> 40, masks 80 -> 40
    dataset_tree(root, 48, 80, ["L", "P"], rng_seed=12, mask_seed0=30)
    cfg = dict(multiscale_config(16, 3, 0), network="multi_adain", vgg="unused", use_mask=True,
               attention="se", img_size=40, test_dir=root, test_dataset="photoreal",
               batch_size=2, num_workers=2)
    m, _ = check_pipeline(cfg, tmp_path, cuda)
    assert m._has_attention()
