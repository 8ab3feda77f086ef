"""LDMSAdaINRPNet (`network: ld_adain`, reference network/adain_rp.py:484-567) on the GPU: the
7x7 reflect conv kernel (rpst_conv7) against float64 and its bit-level properties, a 7x7
Conv2dBlock, test() / encode_rp_intermediate against the reference's recorded outputs
(tests/golden/ld*.npz, gen_golden_ld.py), the fused path against the op-by-op one, the launch
sequence, save / resume, forward() and the stylize pipeline.

Bars: per conv max(1e-5, 3 x the rel-L2 distance of torch's CPU fp32 conv of the same inputs
to float64) -- 1e-5 is the project's per-conv bar; the second term is the reference
arithmetic's own fp32 distance at K = Cin * 49, which is longer than any K the 3x3 kernels
see. TOL_NET / TOL_NET_MAXABS end to end (tests/helpers.py)."""
import copy

import pytest
import torch
import torch.nn.functional as F

import ld_ref as L
from helpers import (TOL_NET, TOL_NET_MAXABS, check_pipeline, dataset_tree, dev, gen, golden_net,
                     mask_kw, max_abs_ratio, rel_l2, synth_, traced_launches, unfused)

pytestmark = pytest.mark.gpu

REFLECT, ZERO = 1, 0
NONE, RELU, LRELU = 0, 1, 2


def _act64(y, act):
    if act == RELU:
        return torch.relu(y)
    if act == LRELU:
        return torch.where(y > 0, y, 0.2 * y)
    return y


def _conv_inputs(shape):
    n, cin, h, w, cout = shape
    x = gen(11, (n, cin, h, w), 1.0, 0.25)
    wt = gen(12, (cout, cin, 7, 7), (3.0 / (cin * 49)) ** 0.5)
    b = gen(13, (cout,), 0.5)
    return x, wt, b


def _conv7(cuda, x, wt, b, pad, act, **kw):
    from rpst import ops
    return ops.conv2d_k7(x.to(cuda), ops.pack_conv7_weight(wt.to(cuda)),
                         None if b is None else b.to(cuda), wt.shape[0], pad=pad, act=act, **kw)


# ---- the kernel ---------------------------------------------------------------------------
# (N, Cin, H, W, Cout), [(pad, act, bias)]
CONV_CASES = [
    ((1, 8, 4, 4, 8), [(REFLECT, NONE, True), (ZERO, RELU, False)]),
    ((2, 32, 13, 9, 32), [(REFLECT, LRELU, True)]),
    ((1, 16, 9, 35, 16), [(REFLECT, RELU, False)]),
    ((1, 20, 17, 33, 24), [(REFLECT, LRELU, True), (ZERO, NONE, True)]),
    ((1, 16, 33, 70, 40), [(REFLECT, NONE, False), (ZERO, LRELU, True)]),
    ((3, 64, 24, 40, 64), [(REFLECT, LRELU, True)]),
    ((2, 128, 16, 20, 128), [(REFLECT, LRELU, True)]),
    ((1, 256, 8, 12, 256), [(REFLECT, RELU, True)]),
]


@pytest.mark.parametrize("shape,variants", CONV_CASES, ids=[str(c[0]) for c in CONV_CASES])
def test_conv7_vs_float64(cuda, shape, variants):
    x, wt, b = _conv_inputs(shape)
    for pad, act, bias in variants:
        mode = "reflect" if pad == REFLECT else "constant"
        bb = b if bias else None
        ref = _act64(L.conv_pad(x.double(), wt.double(), None if bb is None else bb.double(), mode),
                     act)
        cpu32 = _act64(L.conv_pad(x, wt, bb, mode), act)
        floor = rel_l2(cpu32, ref)
        bar = max(1e-5, 3 * floor)
        y = _conv7(cuda, x, wt, bb, pad, act)
        assert tuple(y.shape) == tuple(ref.shape) and y.dtype == torch.float32
        err = rel_l2(y, ref)
        print(f"conv7 {shape} pad {pad} act {act} bias {bias}: rel-L2 {err:.3e}  bar "
              f"max(1e-5, 3 x {floor:.3e}) = {bar:.3e}")
        assert err < bar, (shape, pad, act, bias, err, bar)


def test_conv7_zero_pad_accepts_tiny_images(cuda):
    """Zero padding has no minimum size: 1x1 and 2x3 images, where most taps fall outside."""
    for hw in ((1, 1), (2, 3)):
        x, wt, b = _conv_inputs((2, 8, hw[0], hw[1], 8))
        ref = L.conv_pad(x.double(), wt.double(), b.double(), "constant")
        assert rel_l2(_conv7(cuda, x, wt, b, ZERO, NONE), ref) < 1e-5


def test_conv7_batch_invariant_and_deterministic(cuda):
    """Image k of a batch has the bits of the same image run alone; two runs are identical."""
    x, wt, b = _conv_inputs((3, 20, 17, 33, 24))
    y = _conv7(cuda, x, wt, b, REFLECT, LRELU)
    assert torch.equal(y, _conv7(cuda, x, wt, b, REFLECT, LRELU))
    for k in range(3):
        assert torch.equal(y[k:k + 1], _conv7(cuda, x[k:k + 1], wt, b, REFLECT, LRELU)), k
    # the second input is read in place as the upper half of the batch
    x4 = torch.cat([x, x[:1]])
    y4 = _conv7(cuda, x4, wt, b, REFLECT, LRELU)
    assert torch.equal(y4, _conv7(cuda, x4[:2], wt, b, REFLECT, LRELU, x2=x4[2:].to(cuda)))
    assert torch.equal(y4[:3], y)


@pytest.mark.parametrize("shape", [(2, 16, 9, 35, 16), (1, 128, 16, 20, 128)])
def test_conv7_channel_offset_writes_its_half_only(cuda, shape):
    n, cin, h, w, cout = shape
    x, wt, b = _conv_inputs(shape)
    plain = _conv7(cuda, x, wt, b, REFLECT, LRELU)
    sentinel = -12345.5
    out = torch.full((n, 2 * cout, h, w), sentinel, device=cuda)
    res = _conv7(cuda, x, wt, b, REFLECT, LRELU, out=out, out_channel_offset=cout)
    assert res is out
    assert torch.equal(out[:, :cout], torch.full_like(plain, sentinel))
    assert torch.equal(out[:, cout:], plain)


def test_conv7_op_argument_checks(cuda):
    from rpst import _lib, ops
    x, wt, b = _conv_inputs((1, 8, 3, 8, 8))
    with pytest.raises(_lib.RpstError, match="reflect"):
        _conv7(cuda, x, wt, b, REFLECT, NONE)
    xg = torch.zeros((1, 8, 8, 8), device=cuda, requires_grad=True)
    pk = ops.pack_conv7_weight(wt.to(cuda))
    with pytest.raises(NotImplementedError, match="autograd"):
        ops.conv2d_k7(xg, pk, None, 8)
    with pytest.raises(NotImplementedError, match="autograd"):
        ops.pack_conv7_weight(torch.zeros((8, 8, 7, 7), device=cuda, requires_grad=True))
    with torch.no_grad():
        assert tuple(ops.conv2d_k7(xg, pk, None, 8).shape) == (1, 8, 8, 8)
    with pytest.raises(ValueError, match="out must"):
        ops.conv2d_k7(xg.detach(), pk, None, 8, out=torch.zeros((1, 8, 8, 9), device=cuda))
    with pytest.raises(ValueError, match="channel offset"):
        ops.conv2d_k7(xg.detach(), pk, None, 8, out_channel_offset=8)
    with pytest.raises(_lib.RpstError, match="channels"):
        ops.conv2d_k7(xg.detach(), pk, None, 8, out=torch.zeros((1, 12, 8, 8), device=cuda),
                      out_channel_offset=8)


@pytest.mark.parametrize("pad_type", ["reflect", "zero"])
def test_conv2d_block_7x7_with_inception(cuda, pad_type):
    import network as net
    blk = net.Conv2dBlock(16, 16, 7, 1, 3, inception_num=1, pad_type=pad_type)
    synth_(blk, 21)
    x = gen(22, (2, 16, 17, 33), 1.0, 0.1)
    sd = blk.state_dict()
    y64 = L.conv_pad(x.double(), sd["conv.weight"].double(), sd["conv.bias"].double(),
                     "reflect" if pad_type == "reflect" else "constant")
    y64 = F.conv2d(y64, sd["inception.0.0.weight"].double(), sd["inception.0.0.bias"].double())
    y64 = torch.where(y64 > 0, y64, 0.2 * y64)
    with torch.no_grad():
        y = blk.to(cuda)(x.to(cuda))
    err = rel_l2(y, y64)
    print(f"Conv2dBlock 7x7 {pad_type}: rel-L2 {err:.3e}")
    assert err < 1e-5


def test_plan_runs_7x7_steps(cuda):
    """plan.run / plan.conv route a pad-3 + 7x7 group to conv2d_k7 (one launch, cached
    packed weights); stats_last on a last 7x7 conv reduces the written output."""
    import torch.nn as nn

    from rpst import ops, plan
    torch.manual_seed(31)
    conv = nn.Conv2d(16, 24, 7).to(cuda)
    steps = plan.compile_layers([nn.ZeroPad2d(3), conv, nn.ReLU()])
    x = gen(32, (2, 16, 9, 35)).to(cuda)
    with torch.no_grad():
        direct = ops.conv2d_k7(x, ops.pack_conv7_weight(conv.weight), conv.bias, 24,
                               pad=ops.PAD_ZERO, act=ops.ACT_RELU)
        assert torch.equal(plan.run(steps, x), direct)
        assert torch.equal(plan.conv(steps[0], x), direct)
        assert plan.packed_weight(conv) is plan.packed_weight(conv)
        y, mean, std = plan.run(steps, x, stats_last=True)
        m2, s2 = ops.calc_mean_std(direct)
        assert torch.equal(y, direct) and torch.equal(mean, m2) and torch.equal(std, s2)
        # over [x; x2] a 7x7 first step reads two equal halves in place, else the concatenation
        assert torch.equal(plan.run(steps, x[:1], x2=x[1:]), direct)
        x3 = torch.cat([x, x[:1]])
        assert torch.equal(plan.run(steps, x3[:1], x2=x3[1:])[:2], direct)
        with pytest.raises(NotImplementedError, match="7x7"):
            plan.conv(steps[0], x, residual=direct)


# ---- the network --------------------------------------------------------------------------
def _net(g, i, cuda):
    import network as net
    return golden_net(net.LDMSAdaINRPNet, L.golden_config(g, i), g, f"net{i}_", cuda)


@pytest.mark.parametrize("i", range(len(L.CASES)))
def test_ld_test_matches_reference(cuda, golden, i, tmp_path):
    import network.adain_rp as arp
    g = golden("ld")
    m = _net(g, i, cuda)
    c, s = dev(g[f"net{i}_content"], cuda), dev(g[f"net{i}_style"], cuda)
    kw = mask_kw(g, f"net{i}_", cuda)
    y = m.test(c, s, **kw)
    assert m.training  # test() leaves the model in training mode, as the reference does
    ref = g[f"net{i}_out"]
    err, mx = rel_l2(y, ref), max_abs_ratio(y, ref)
    print(f"ld case {i}: rel-L2 {err:.3e} max-abs ratio {mx:.3e} (reference floor "
          f"{float(g[f'net{i}_floor']):.2e})")
    assert err < TOL_NET and mx < TOL_NET_MAXABS
    assert rel_l2(y, g[f"net{i}_out64"]) < TOL_NET
    assert torch.equal(y, m.test(c, s, **kw))
    if kw:  # from the mask files themselves (decoded and resized by rpst.imageio)
        yf = m.test(c, s, **mask_kw(g, f"net{i}_", cuda, tmp_path))
        assert rel_l2(yf, ref) < TOL_NET and max_abs_ratio(yf, ref) < TOL_NET_MAXABS
    with unfused(arp, "FUSED_ADAIN"):
        plain = m.test(c, s, **kw)
    assert rel_l2(plain, ref) < TOL_NET
    assert rel_l2(y, plain) < 1e-5
    m.eval()
    with torch.no_grad():
        dec = m.decode(m.encode_rp_intermediate(c), m.encode_rp_intermediate(s),
                       use_mask=bool(g[f"net{i}_use_mask"]), **kw)
    assert torch.equal(dec, plain)


@pytest.mark.parametrize("i", range(3))
def test_ld_encoder_levels_match_reference(cuda, golden, i):
    g = golden("ld")
    m = _net(g, i, cuda)
    with torch.no_grad():
        levels = m.encode_rp_intermediate(dev(g[f"net{i}_content"], cuda))
    assert len(levels) == int(g[f"net{i}_layers"])
    for k, lv in enumerate(levels):
        ref = g[f"net{i}_level{k}_64"]
        assert tuple(lv.shape) == tuple(ref.shape)
        err = rel_l2(lv, ref)
        print(f"ld case {i} level {k}: rel-L2 {err:.3e} (reference fp32 "
              f"{float(g[f'net{i}_level{k}_floor']):.2e})")
        assert err < TOL_NET, (i, k, err)


def test_ld_launch_sequence(cuda, golden):
    """The (16, 5) case: every 7x7 layer (32, 64, 128, 256 channels) is one conv7x7 launch
    over the [content; style] batch writing into the level tensor, and no level tensor comes
    from torch.cat."""
    g = golden("ld")
    m = _net(g, 2, cuda)
    c, s = dev(g["net2_content"], cuda), dev(g["net2_style"], cuda)
    m.test(c, s)  # warm: the packed weights are cached
    names, cats = traced_launches(lambda: m.test(c, s))
    k7 = [nm for nm in names if nm.startswith("conv7x7 ")]
    assert k7 == [f"conv7x7 {ch}->{ch} 16x20 N2" for ch in (32, 64, 128, 256)], names
    # the only concatenations are the AdaIN parameter vectors (1-D)
    assert all(len(shape) == 1 for shapes in cats for shape in shapes), cats


def test_ld_save_and_resume(cuda, golden, tmp_path):
    g = golden("ld")
    m = _net(g, 0, cuda)
    c, s = dev(g["net0_content"], cuda), dev(g["net0_style"], cuda)
    y = m.test(c, s)
    path = str(tmp_path / "1234.pth")
    m.save(path, 1234)
    assert set(torch.load(path, weights_only=True).keys()) == set(m.state_dict().keys())
    import network as net
    cfg = dict(L.config(4, 3), resume=True, checkpoint_path=path)
    m2 = net.LDMSAdaINRPNet(cfg, copy.deepcopy(net.vgg)).to(cuda)
    assert m2.begin == 1234
    assert torch.equal(m2.test(c, s), y)


def test_ld_forward_losses(cuda, golden):
    g = golden("ld")
    m = _net(g, 0, cuda)
    c, s = dev(g["net0_content"], cuda), dev(g["net0_style"], cuda)
    with torch.no_grad():
        losses, total = m(c, s)
    assert set(losses) == {"style_loss", "content_loss", "total_loss"}
    assert all(bool(torch.isfinite(v).all()) for v in losses.values())
    assert torch.equal(total, losses["total_loss"])
    assert torch.is_grad_enabled()
    # with autograd enabled forward() is rpst.autograd.ld_losses, bit for bit
    from rpst import autograd as A
    train_losses, train_total = m(c, s)
    assert set(train_losses) == {"style_loss", "content_loss", "total_loss"}
    assert all(bool(torch.isfinite(v).all()) for v in train_losses.values())
    assert train_total.requires_grad and train_losses["total_loss"].requires_grad
    ref_losses, ref_total = A.ld_losses(m, c, s)
    assert torch.equal(train_total, ref_total)
    for k, v in ref_losses.items():
        assert torch.equal(train_losses[k], v), k


# ---- pipeline -----------------------------------------------------------------------------
@pytest.mark.parametrize("use_mask", [False, True])
def test_pipeline_with_ld_adain(cuda, tmp_path, use_mask):
    """stylize.py with `network: ld_adain` and --synthetic-weights: the PNGs it writes are the
    direct test() call's through the pipeline's own uint8 conversion."""
    import network as net
    root = str(tmp_path / "data")
    # images 40 -> 32, masks 64 -> 32
    dataset_tree(root, 40, 64, ["L", "P"], rng_seed=12, mask_seed0=30, masks=use_mask)
    cfg = dict(L.config(4, 3, 0, use_mask), network="ld_adain", vgg="unused", img_size=32,
               test_dir=root, test_dataset="photoreal" if use_mask else "paired", batch_size=2,
               num_workers=2)
    m, _ = check_pipeline(cfg, tmp_path, cuda)
    assert isinstance(m, net.LDMSAdaINRPNet)
