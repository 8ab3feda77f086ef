"""LDMSAdaINRPNet (`network: ld_adain`) and the 7x7 conv, the parts that need no GPU: the
float64 restatement (tests/ld_ref.py) against the reference's recorded float64 outputs and
levels, the mirror's state_dict keys, the plan's 7x7 step, and what keeps raising."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import ld_ref as L
from helpers import golden_net, rel_l2


def _model(g, i):
    import network as net
    return golden_net(net.LDMSAdaINRPNet, L.golden_config(g, i), g, f"net{i}_")


def test_cases_recorded(golden):
    g = golden("ld")
    assert int(g["n_net"]) == len(L.CASES) == 4
    for i, (hid, layers, inc, shape, use_mask, seed) in enumerate(L.CASES):
        assert (int(g[f"net{i}_hidden"]), int(g[f"net{i}_layers"]), int(g[f"net{i}_inception"]),
                tuple(g[f"net{i}_content"].shape), bool(g[f"net{i}_use_mask"]),
                int(g[f"net{i}_seed"])) == (hid, layers, inc, shape, use_mask, seed)
        # the reference's own fp32 distance sits far inside TOL_NET
        assert float(g[f"net{i}_floor"]) < 1e-5, i


@pytest.mark.parametrize("i", range(len(L.CASES)))
def test_restatement_matches_reference_float64(golden, i):
    """ld_ref.test / ld_ref.encode against the reference's float64 run: 1e-12 rel-L2 for the
    output and for every level of encode_rp_intermediate(content)."""
    g = golden("ld")
    m = _model(g, i)  # (its checksum is the recorded one)
    sd = m.state_dict()
    layers = int(g[f"net{i}_layers"])
    segs = (g[f"net{i}_cseg"], g[f"net{i}_sseg"]) if bool(g[f"net{i}_use_mask"]) else (None, None)
    y = L.test(g[f"net{i}_content"], g[f"net{i}_style"], sd, layers, *segs)
    assert g[f"net{i}_out64"].dtype == np.float64
    err = rel_l2(y, g[f"net{i}_out64"])
    print(f"case {i}: restatement vs float64 reference {err:.2e}")
    assert err < 1e-12, (i, err)
    with torch.no_grad():
        levels = L.encode(g[f"net{i}_content"], sd, layers)
    for k, lv in enumerate(levels):
        assert tuple(lv.shape[1:2]) == (int(g[f"net{i}_hidden"]) * 2 ** (k + 1),)
        assert rel_l2(lv, g[f"net{i}_level{k}_64"]) < 1e-12, (i, k)


@pytest.mark.parametrize("i", range(len(L.CASES)))
def test_state_dict_keys_match_reference(golden, i):
    g = golden("ld")
    m = _model(g, i)
    names, shapes = L.key_table(m.state_dict())
    assert list(names) == list(g[f"net{i}_keys"])
    assert np.array_equal(shapes, g[f"net{i}_shapes"])


def test_big_branch_is_7x7():
    import network as net
    m = net.LDMSAdaINRPNet(L.config(4, 3), copy.deepcopy(net.vgg))
    assert m.rp_enc0_big_revf.conv.kernel_size == (3, 3)
    for i in (1, 2):
        big, small = getattr(m, f"rp_enc{i}_big_revf"), getattr(m, f"rp_enc{i}_small_revf")
        assert big.conv.kernel_size == (7, 7) and tuple(big.pad.padding) == (3, 3, 3, 3)
        assert small.conv.kernel_size == (3, 3)
        assert big.conv.in_channels == big.conv.out_channels == 4 * 2 ** i
    assert m.rp_shared_encoder is None and m.rp_decoder is None
    assert m.layer_num == 3 and m.encoder_out_dim == 16


def test_stylized_layers_below_layer_num_raises():
    import network as net
    cfg = L.config(4, 3)
    cfg["stylized_layers"] = 2
    with pytest.raises(ValueError, match="stylized_layers"):
        net.LDMSAdaINRPNet(cfg, copy.deepcopy(net.vgg))


def test_forward_with_grad_raises_before_any_kernel():
    import network as net
    """forward() with autograd enabled is the parent's dispatch to rpst.autograd.ld_losses:
    CPU tensors are refused before any kernel (no CPU fallback), sort / shuffle before that."""
    m = net.LDMSAdaINRPNet(L.config(4, 3), copy.deepcopy(net.vgg))
    x = torch.zeros(1, 3, 8, 8)
    assert torch.is_grad_enabled() and any(p.requires_grad for p in m.parameters())
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m(x, x)
    for key in ("sort", "shuffle"):
        cfg = L.config(4, 3)
        cfg[key] = True
        with pytest.raises(NotImplementedError, match="shuffle / sort"):
            net.LDMSAdaINRPNet(cfg, copy.deepcopy(net.vgg))(x, x)


def test_stylize_builds_ld_adain_and_refuses_the_later_ones():
    import network as net
    import stylize
    opt = dict(L.config(4, 3), network="ld_adain")
    assert isinstance(stylize.build_network(opt, synthetic_seed=1), net.LDMSAdaINRPNet)
    assert "ld_adain" not in stylize.OUT_OF_SCOPE and "ld_adain" in stylize.MASKED_NETWORKS
    assert stylize.mask_size("ld_adain", 24) == (24, 24)
    for kind in ("ld_adain2", "ld_adain3", "sel_multi_adain", "mrf", "spade"):
        with pytest.raises(NotImplementedError):
            stylize.build_network(dict(opt, network=kind), synthetic_seed=1)


def test_plan_accepts_pad3_7x7_and_rejects_the_rest():
    from rpst import ops, plan
    for pad_layer, mode in ((nn.ReflectionPad2d(3), ops.PAD_REFLECT), (nn.ZeroPad2d(3), ops.PAD_ZERO)):
        steps = plan.compile_layers([pad_layer, nn.Conv2d(8, 8, 7), nn.LeakyReLU(0.2)])
        assert len(steps) == 1 and isinstance(steps[0], plan.ConvStep)
        assert (steps[0].pad, steps[0].in_op, steps[0].relu) == (mode, ops.IN_NONE, ops.ACT_LRELU)
    import network as net
    blk = net.Conv2dBlock(8, 8, 7, 1, 3, inception_num=1)
    steps = plan.compile_layers(plan.block_layers(blk))
    assert [s.conv.kernel_size[0] for s in steps] == [7, 1] and steps[1].relu == ops.ACT_LRELU
    bad = [
        [nn.ReflectionPad2d(2), nn.Conv2d(8, 8, 5)],            # 5x5
        [nn.ReflectionPad2d(2), nn.Conv2d(8, 8, 7)],            # pad 2
        [nn.ReflectionPad2d(3), nn.Conv2d(8, 8, 7, stride=2)],  # stride 2
        [nn.ReflectionPad2d(3), nn.Conv2d(8, 8, 3)],            # pad 3 in front of a 3x3
        [nn.ReflectionPad2d(1), nn.Conv2d(8, 8, 7)],            # pad 1 in front of a 7x7
        [nn.ReflectionPad2d(3), nn.Conv2d(8, 8, 7, padding=3)],
        [nn.MaxPool2d(2, 2, ceil_mode=True), nn.ReflectionPad2d(3), nn.Conv2d(8, 8, 7)],
        [nn.Upsample(scale_factor=2, mode="nearest"), nn.ZeroPad2d(3), nn.Conv2d(8, 8, 7)],
    ]
    for layers in bad:
        with pytest.raises(NotImplementedError):
            plan.compile_layers(layers)


def test_plan_7x7_refuses_loader_operators():
    from rpst import ops, plan
    steps = plan.compile_layers([nn.ReflectionPad2d(3), nn.Conv2d(8, 8, 7)])
    x = torch.zeros(1, 8, 8, 8)
    with pytest.raises(NotImplementedError, match="7x7"):
        plan.run(steps, x, first_in_op=ops.IN_ADAIN, first_aux=torch.zeros(32))
    with pytest.raises(NotImplementedError, match="7x7"):
        plan.run(steps, x, first_mix=(torch.zeros(1, 8, 8), torch.zeros(1, 8)))


def test_ops_refuse_cpu_tensors_and_grad():
    from rpst import ops
    w = torch.zeros(8, 8, 7, 7)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.pack_conv7_weight(w)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.conv2d_k7(torch.zeros(1, 8, 8, 8), torch.zeros(8 * 49 * 32), None, 8)
    # pack_conv_weight keeps its 1x1 / 3x3 contract
    with pytest.raises((AssertionError, RuntimeError)):
        ops.pack_conv_weight(w)


def test_conv7_abi_argument_errors():
    """rpst_conv7 / rpst_conv7_pack check their arguments before touching the device."""
    from rpst import _lib
    lib = _lib.load()

    def conv7(inp=1, in2=None, wt=1, bias=None, out=1, N=2, Cin=8, H=8, W=8, Cout=8, pad=1, act=0,
              off=0, total=8):
        return lib.rpst_conv7(inp, in2, wt, bias, out, N, Cin, H, W, Cout, pad, act, off, total,
                              None)

    def err():
        return lib.rpst_last_error().decode()

    assert conv7(inp=None) == -1 and "null pointer" in err()
    assert conv7(wt=None) == -1 and "null pointer" in err()
    assert conv7(out=None) == -1 and "null pointer" in err()
    assert conv7(N=0) == -1 and "bad shape" in err()
    assert conv7(H=3) == -1 and "reflect" in err()
    assert conv7(W=3) == -1 and "reflect" in err()
    assert conv7(pad=2) == -1 and "bad pad" in err()
    assert conv7(act=3) == -1 and "activation" in err()
    assert conv7(off=1) == -1 and "channels" in err()
    assert conv7(off=-1, total=16) == -1 and "channels" in err()
    assert conv7(in2=1, N=3) == -1 and "even" in err()
    assert lib.rpst_conv7_pack(None, 1, 8, 8, None) == -1 and "null pointer" in err()
    assert lib.rpst_conv7_pack(1, 1, 0, 8, None) == -1 and "bad channels" in err()
    # the existing conv entries keep their contract
    assert lib.rpst_conv2d_packed_size(8, 8, 7) == 0 and lib.rpst_conv2d_packed_size(8, 8, 2) == 0
    assert lib.rpst_conv2d(1, None, 1, None, None, 1, 1, 8, 8, 8, 8, 5, 0, 0, 0, None) == -1
    assert "ksize" in err()


def test_conv7_packed_size_formula():
    """4 * ceil(Cin / 8) * 49 * 8 * Cout_pad bytes, Cout_pad = Cout rounded up to its tile
    (32 up to 32 channels, 64 up to 64, else 128)."""
    from rpst import _lib
    lib = _lib.load()
    assert lib.rpst_conv7_packed_size(24, 20) == 4 * 3 * 49 * 8 * 32
    assert lib.rpst_conv7_packed_size(256, 256) == 4 * 32 * 49 * 8 * 256
    assert lib.rpst_conv7_packed_size(40, 16) == 4 * 2 * 49 * 8 * 64
    assert lib.rpst_conv7_packed_size(0, 8) == 0 and lib.rpst_conv7_packed_size(8, -1) == 0
