"""Host side of the opt-in bf16 inference path: what plan.lower(precision="bf16") sends to
rpst_conv2d_bf16, the `precision` config key of the models, and the CPU emulation
(tests/bf16_ref.py) against the float64 oracle. No GPU: lower() is host-only, and the library's
rpst_conv2d_bf16_supports is a host function.

The emulation's brackets below are what this file's own case reads (AdaINRPNet rp_blocks 5,
hidden 16, synthetic weights seed 31, uniform [0, 1) images, N = 2, the five layers of 64 or
more output channels rounded): at 24^2 / 48^2 the emulation sits 1.92e-2 / 2.00e-2 rel-L2 and
2.2 % / 1.8 % of max|ref| from the float64 oracle with either accumulation, and its fp32 and
float64 accumulations sit 2.2e-3 / 2.7e-3 apart: rounding decisions diverge through the stack,
which is why the GPU test holds the kernel to twice the emulation's distance from the oracle and
not to the emulation itself.
"""
import copy

import pytest
import torch
import torch.nn as nn

import bf16_ref as B
from helpers import (gen, golden_net, max_abs_ratio, multiscale_config, rel_l2, rp_config,
                     state_dict_of)
from oracle import restate as R


def _ops(launches):
    return [rec.op for rec in launches]


@pytest.fixture(scope="module")
def model():
    import network as net
    return golden_net(net.AdaINRPNet, rp_config(16), None, "", seed=31)


def test_supports_rule_is_host_only_and_measured():
    """Capability (3x3, Cin % 16, Cout >= 16, zero / reflect, no operator or AdaIN) and the
    measured rule (profiles/bf16: every layer of at most 32 output channels lost to its fp32
    kernel at 512^2)."""
    from rpst import ops
    yes = [(64, 32), (128, 64), (256, 128), (128, 256), (64, 128), (64, 16), (512, 256)]
    no = [(32, 16), (32, 64), (16, 32), (16, 3), (3, 16), (64, 24), (8, 32), (64, 272), (63, 32)]
    for cout, cin in yes:
        for pad in (ops.PAD_ZERO, ops.PAD_REFLECT):
            for in_op in (ops.IN_NONE, ops.IN_ADAIN):
                assert ops.conv2d_bf16_supports(cout, cin, 3, pad, in_op), (cout, cin, pad, in_op)
    for cout, cin in no:
        assert not ops.conv2d_bf16_supports(cout, cin), (cout, cin)
    for in_op in (ops.IN_MAXPOOL2, ops.IN_UPSAMPLE2, ops.IN_ADD_UPSAMPLE2, ops.IN_ADD_ADAIN):
        assert not ops.conv2d_bf16_supports(128, 64, 3, ops.PAD_ZERO, in_op)
    assert not ops.conv2d_bf16_supports(128, 64, 1) and not ops.conv2d_bf16_supports(128, 64, 7)
    assert not ops.conv2d_bf16_supports(128, 64, 3, 2)


def test_lowering_of_the_adain_rp_stacks(model):
    from rpst import ops, plan
    enc, dec = plan.of(model.rp_shared_encoder), plan.of(model.rp_decoder)
    shape = (2, 3, 24, 24)
    fp32 = plan.lower(enc, shape, shape, stats_last=True)
    assert _ops(fp32) == ["conv2d_pair", "conv2d", "conv2d", "conv2d", "conv2d_stats"]
    assert plan.lower(enc, shape, shape, stats_last=True, precision="fp32") == fp32
    low = plan.lower(enc, shape, shape, stats_last=True, precision="bf16")
    # 3->16 (paired, fp32), 16->32 (fp32: the measured rule), 32->64, 64->128, 128->256
    assert _ops(low) == ["conv2d_pair", "conv2d", "conv2d_bf16", "conv2d_bf16", "conv2d_bf16"]
    assert [rec.takes for rec in low] == [("x2",), (), (), (), ("store_n",)]
    for a, b in zip(low, fp32):  # nothing but the op changes
        assert (a.step, a.in_op, a.pooled, a.takes) == (b.step, b.in_op, b.pooled, b.takes)
        c = a.step.conv
        assert (a.op == "conv2d_bf16") == ops.conv2d_bf16_supports(
            c.out_channels, c.in_channels, 3, a.step.pad, a.in_op)

    dshape = (2, 256, 24, 24)
    fp32 = plan.lower(dec, dshape, first_in_op=ops.IN_ADAIN)
    assert _ops(fp32) == ["conv2d"] * 5 and fp32[0].takes == ("aux",)
    assert plan.lower(dec, dshape, first_in_op=ops.IN_ADAIN, precision="fp32") == fp32
    low = plan.lower(dec, dshape, first_in_op=ops.IN_ADAIN, precision="bf16")
    # 256->128 (AdaIN loader), 128->64, then 64->32, 32->16, 16->3 on fp32
    assert _ops(low) == ["conv2d_bf16", "conv2d_bf16", "conv2d", "conv2d", "conv2d"]
    assert low[0].takes == ("aux",) and low[0].in_op == ops.IN_ADAIN
    assert all(rec.takes == () for rec in low[1:])


def test_lowering_pair_stats_and_what_stays():
    from rpst import ops, plan
    seq = nn.Sequential(nn.Conv2d(32, 64, 3, padding=1), nn.ReLU(),
                        nn.ReflectionPad2d(1), nn.Conv2d(64, 128, 3), nn.LeakyReLU(0.2),
                        nn.Conv2d(128, 128, 1),
                        nn.Upsample(scale_factor=2, mode="nearest"),
                        nn.ReflectionPad2d(1), nn.Conv2d(128, 64, 3),
                        nn.ReflectionPad2d(3), nn.Conv2d(64, 64, 7),
                        nn.MaxPool2d((2, 2), (2, 2), (0, 0), ceil_mode=True),
                        nn.Conv2d(64, 64, 3, padding=1))
    steps = plan.compile_layers(seq.children())
    shape = (1, 32, 20, 20)
    fp32 = plan.lower(steps, shape, (2, 32, 20, 20), stats_last=True)
    low = plan.lower(steps, shape, (2, 32, 20, 20), stats_last=True, precision="bf16")
    assert len(low) == len(fp32)
    for a, b in zip(low, fp32):
        assert (a.step, a.in_op, a.pooled, a.takes) == (b.step, b.in_op, b.pooled, b.takes)
    changed = [(b.op, a.op) for a, b in zip(low, fp32) if a.op != b.op]
    # the paired first conv, the reflect-padded LeakyReLU conv, and (when the pool before it
    # ran as a pass of its own) the last conv with its statistics; the 1x1, the upsampling
    # and the 7x7 conv keep their kernels
    assert changed[:2] == [("conv2d_pair", "conv2d_bf16"), ("conv2d", "conv2d_bf16")]
    assert low[0].takes == ("x2",)
    assert all(a.op == b.op for a, b in zip(low, fp32)
               if b.op in ("conv2d_k7", "maxpool2x2_ceil", "upsample_nearest2x", "conv2d_pool")
               or (b.step is not None and (b.step.conv.kernel_size[0] != 3
                                           or b.in_op not in (ops.IN_NONE, ops.IN_ADAIN))))
    last = low[-1]
    if last.op == "conv2d_bf16":
        assert last.takes == ("store_n",) and last.in_op == ops.IN_NONE
    # a single statistics conv over a pair is not paired (as on fp32): the cat stays
    one = plan.compile_layers([nn.Conv2d(32, 64, 3, padding=1)])
    low = plan.lower(one, shape, shape, stats_last=True, precision="bf16")
    assert _ops(low) == ["cat", "conv2d_bf16"] and low[1].takes == ("store_n",)


def test_precision_is_validated():
    import network as net
    from rpst import plan
    vgg = net.vgg
    with pytest.raises(ValueError, match="precision"):
        plan.lower([], (1, 3, 8, 8), precision="fp16")
    with pytest.raises(ValueError, match="precision"):
        net.AdaINRPNet(dict(rp_config(4), precision="fp16"), copy.deepcopy(vgg))
    assert net.AdaINRPNet(rp_config(4), copy.deepcopy(vgg)).precision == "fp32"
    assert net.AdaINRPNet(dict(rp_config(4), precision="fp32"), copy.deepcopy(vgg)).precision == "fp32"
    assert net.AdaINRPNet(dict(rp_config(4), precision="bf16"), copy.deepcopy(vgg)).precision == "bf16"
    for build in (lambda: net.MultiScaleAdaINRPNet(dict(multiscale_config(8), precision="bf16"),
                                                   copy.deepcopy(vgg)),
                  lambda: net.WCTRPNet(dict(rp_config(4), precision="bf16"), copy.deepcopy(vgg)),
                  lambda: net.SourceNet({"precision": "bf16"}, copy.deepcopy(vgg)),
                  lambda: net.SAModel({"precision": "bf16"}, copy.deepcopy(vgg), 0, 64),
                  lambda: net.AdaptiveSAModel({"precision": "bf16"}, copy.deepcopy(vgg), 0, 64)):
        with pytest.raises(NotImplementedError, match="bf16"):
            build()
    with pytest.raises(ValueError, match="precision"):
        net.WCTRPNet(dict(rp_config(4), precision="half"), copy.deepcopy(vgg))
    # the other families still build without the key and with "fp32"
    net.MultiScaleAdaINRPNet(dict(multiscale_config(8), precision="fp32"), copy.deepcopy(vgg))


def test_wrappers_refuse_cpu_tensors():
    from rpst import ops
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.pack_conv_weight_bf16(torch.zeros(64, 32, 3, 3))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.conv2d_bf16(torch.zeros(1, 32, 4, 4), torch.zeros(8, dtype=torch.bfloat16), None, 64)


def test_round_bf16_is_nearest_even():
    x = torch.tensor([1.0, 1.00390625, 1.01171875, 1.0 + 2 ** -8 + 2 ** -20, -1.0 - 2 ** -8 - 2 ** -20])
    # 1 + 2^-8 is a tie between 1 and 1 + 2^-7 (even: 1); 1 + 3 * 2^-8 a tie going up to even
    assert B.round_bf16(x).tolist() == [1.0, 1.0, 1.015625, 1.0078125, -1.0078125]


@pytest.mark.parametrize("size", [24, 48])
def test_emulation_brackets(model, size):
    from rpst import ops
    content, style = gen(40 + size, (2, 3, size, size), 0.5, 0.5), gen(41 + size, (2, 3, size, size), 0.5, 0.5)
    sd = state_dict_of(model)
    oracle = R.adain_rp_test(content.double(), style.double(),
                             {k: v.double() for k, v in sd.items()}, 5)

    def eligible(cout, cin):
        return ops.conv2d_bf16_supports(cout, cin)

    e64 = B.adain_rp_test_bf16(content, style, sd, 5, eligible)
    e32 = B.adain_rp_test_bf16(content, style, sd, 5, eligible, acc=torch.float32)
    plain = B.adain_rp_test_bf16(content, style, sd, 5, lambda cout, cin: False)
    d64, d32, apart = rel_l2(e64, oracle), rel_l2(e32, oracle), rel_l2(e32, e64)
    m64, m32 = max_abs_ratio(e64, oracle), max_abs_ratio(e32, oracle)
    print(f"bf16 emulation {size}^2: to oracle {d64:.3e} (float64 sums) {d32:.3e} (fp32 sums), "
          f"max-abs {m64:.3e} {m32:.3e}; fp32 vs float64 sums {apart:.3e}")
    assert rel_l2(plain, oracle) < 1e-6  # with no layer rounded the emulation is the oracle
    assert 1.5e-2 < d64 < 2.5e-2 and 1.5e-2 < d32 < 2.5e-2, (d64, d32)
    assert 1.2e-2 < m64 < 3e-2 and 1.2e-2 < m32 < 3e-2, (m64, m32)
    assert 1.5e-3 < apart < 3.5e-3, apart
