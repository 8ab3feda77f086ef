"""GPU parity of the opt-in bf16 conv (rpst_conv2d_bf16) and of AdaINRPNet.test() under
precision "bf16", against the CPU emulation of its arithmetic contract (tests/bf16_ref.py).

Single layers take inputs and weights that are already bf16 values, so no rounding decision
can differ between the kernel and the emulation; what is left is fp32 against float64
accumulation of exact products, which reads 0.75-1.05e-7 rel-L2 on the CPU at (16->32),
(128->64), (256->128). The bar is the fp32 convs' own, 1e-5 (tests/test_gpu_kernels.py); an
fp32 kernel on unrounded operands misses this reference by 2.3e-3, so a silent fallback fails.
Under RPST_IN_ADAIN the affine makes values that are no bf16 values and a 1-ulp difference in
it flips a rounding now and then: the bar there is max(1e-5, 3 d), d the distance between the
emulation with the affine in fp32 and in float64 (printed; std_c >= 0.1 keeps d below 1e-4).
End to end the rounding decisions diverge through ten layers: the emulation is no tight
reference, so the GPU result is held to twice the emulation's own distance from the float64
oracle (rel-L2 and max-abs), both sides computed here.
"""
import functools

import pytest
import torch

import bf16_ref as B
from helpers import gen, golden_net, max_abs_ratio, rel_l2, rp_config, state_dict_of
from oracle import restate as R

pytestmark = pytest.mark.gpu

TOL_OUT = 1e-5
TOL_STAT = 1e-6
EPS = 1e-5
ZERO, REFLECT = 0, 1
PADS = {ZERO: "zero", REFLECT: "reflect"}


@functools.lru_cache(maxsize=None)
def _problem(seed, n, cin, h, w, cout, bias=True):
    """bf16-valued input and weights (fp32 tensors), fp32 bias; formed once, never modified."""
    x = B.round_bf16(gen(seed, (n, cin, h, w), 1.0, 0.2))
    wt = B.round_bf16(gen(seed + 1, (cout, cin, 3, 3), (2.0 / (cin * 9)) ** 0.5))
    b = gen(seed + 2, (cout,), 0.05) if bias else None
    return x, wt, b


def _run(cuda, x, wt, b, pad=ZERO, act=0, **kw):
    from rpst import ops
    packed = ops.pack_conv_weight_bf16(wt.to(cuda))
    kw = {k: (v.to(cuda) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    return ops.conv2d_bf16(x.to(cuda), packed, None if b is None else b.to(cuda), wt.shape[0],
                           pad=pad, relu=act, **kw)


# (N, Cin, Cout, H, W), pad, activation, bias: every shape with both pads where reflect is
# defined, the three activations and bias / no bias spread over them
LAYERS = [
    ((2, 16, 32, 20, 37), ZERO, 0, True), ((2, 16, 32, 20, 37), REFLECT, 1, False),
    ((3, 48, 16, 9, 33), ZERO, 2, False), ((3, 48, 16, 9, 33), REFLECT, 0, True),
    ((1, 128, 256, 7, 5), ZERO, 1, True), ((1, 128, 256, 7, 5), REFLECT, 2, True),
    ((2, 256, 128, 33, 64), ZERO, 2, True), ((2, 256, 128, 33, 64), REFLECT, 1, False),
    ((1, 32, 32, 1, 1), ZERO, 0, False), ((1, 32, 32, 1, 1), ZERO, 1, True),
    ((1, 32, 32, 2, 3), REFLECT, 2, True), ((1, 32, 32, 2, 3), ZERO, 0, True),
]


@pytest.mark.parametrize("shape,pad,act,bias", LAYERS)
def test_layer_vs_emulation(cuda, shape, pad, act, bias):
    n, cin, cout, h, w = shape
    x, wt, b = _problem(100 + cin + cout, n, cin, h, w, cout, bias)
    ref = B.conv_bf16(x, wt, b, PADS[pad], act)
    out = _run(cuda, x, wt, b, pad, act)
    assert out.dtype == torch.float32 and out.shape == ref.shape
    err = rel_l2(out, ref)
    print(f"bf16 conv {shape} pad {pad} act {act}: rel-L2 {err:.3e}")
    assert err < TOL_OUT, err


def test_pair_input_equals_concatenation(cuda):
    x, wt, b = _problem(7, 3, 32, 11, 37, 64)
    whole = _run(cuda, x, wt, b, REFLECT, 1)
    pair = _run(cuda, x[:1], wt, b, REFLECT, 1, x2=x[1:])
    assert torch.equal(whole, pair)


@pytest.mark.parametrize("cin,cout", [(32, 64), (128, 256)])
def test_batch_invariance(cuda, cin, cout):
    x, wt, b = _problem(9, 3, cin, 10, 35, cout)
    whole = _run(cuda, x, wt, b, ZERO, 2)
    for i in range(3):
        assert torch.equal(whole[i:i + 1], _run(cuda, x[i:i + 1], wt, b, ZERO, 2)), i


@pytest.mark.parametrize("shape", [(3, 32, 48, 21, 37), (3, 128, 256, 19, 40), (3, 16, 16, 3, 2)])
def test_statistics_and_store_n(cuda, shape):
    n, cin, cout, h, w = shape
    x, wt, b = _problem(11, n, cin, h, w, cout)
    out, mean, std = _run(cuda, x, wt, b, ZERO, 1, stats=True)
    assert torch.equal(out, _run(cuda, x, wt, b, ZERO, 1))
    m64, s64 = R.calc_mean_std(out.double().cpu(), EPS)
    em, es = rel_l2(mean, m64), rel_l2(std, s64)
    print(f"bf16 conv stats {shape}: mean {em:.3e} std {es:.3e}")
    assert em < TOL_STAT and es < TOL_STAT, (em, es)
    out1, mean1, std1 = _run(cuda, x, wt, b, ZERO, 1, stats=True, store_n=1)
    assert torch.equal(out1[:1], out[:1])
    assert torch.equal(mean1, mean) and torch.equal(std1, std)


@functools.lru_cache(maxsize=None)
def _adain_case():
    """A (2, 256, 61, 75) input, statistics with std_c in [0.6, 1.0] (so the affine's values
    span one decade: no single rounding flip dominates the L2 distance) and the affine formed
    in fp32 and in float64. 2.3 M values: some 75 of them round differently between the two
    forms, enough for d to be a stable figure (at 150 k values it is 5 flips, and d then
    depends on how large those five values happen to be)."""
    n, cin, h, w = 2, 256, 61, 75
    x = gen(13, (n, cin, h, w), 1.0, 0.2)
    mc, sc = gen(15, (n, cin, 1, 1), 0.3, 0.2), gen(16, (n, cin, 1, 1), 0.2, 0.8)
    ms, ss = gen(17, (n, cin, 1, 1), 0.5), gen(18, (n, cin, 1, 1), 0.2, 0.8)
    assert float(sc.min()) >= 0.1
    return (x, (mc, sc, ms, ss), B.adain_affine(x, mc, sc, ms, ss, torch.float32),
            B.adain_affine(x, mc, sc, ms, ss, torch.float64))


@pytest.mark.parametrize("cout,pad", [(16, REFLECT), (48, ZERO), (128, REFLECT)])
def test_adain_loader(cuda, cout, pad):
    """One case per output-channel tile (32, 64, 128), each with the AdaIN loader."""
    from rpst import ops
    x, stats, a32, a64 = _adain_case()
    wt = B.round_bf16(gen(19, (cout, x.shape[1], 3, 3), (2.0 / (x.shape[1] * 9)) ** 0.5))
    b = gen(20, (cout,), 0.05)
    ref32, ref64 = (B.conv_bf16(a, wt, b, PADS[pad], 1) for a in (a32, a64))
    d = rel_l2(ref32, ref64)
    aux = ops.adain_params(*(t.to(cuda) for t in stats))
    out = _run(cuda, x, wt, b, pad, 1, in_op=ops.IN_ADAIN, aux=aux)
    err = rel_l2(out, ref64)
    print(f"bf16 conv AdaIN loader 256->{cout} pad {pad}: rel-L2 {err:.3e}, d = {d:.3e}")
    assert d < 1e-4, d
    assert err < max(TOL_OUT, 3 * d), (err, d)


def test_refusals(cuda):
    from rpst import _lib, ops
    lib = _lib.load()
    einval = _lib.constants("EINVAL")[0]
    buf = torch.zeros(1 << 16, device=cuda)

    def call(cin, cout, in_op, aux=None):
        p = buf.data_ptr()  # input, packed weights and output: disjoint thirds of buf
        return lib.rpst_conv2d_bf16(p, None, 0, aux, p + (64 << 10), None, p + (128 << 10), 1,
                                    cin, 4, 4, cout, ZERO, in_op, 0, None, None, EPS, 1, None, 0,
                                    None)

    assert call(32, 32, ops.IN_NONE) == 0  # the frame itself is a valid call
    torch.cuda.synchronize()
    for cin, cout, k, in_op in [(24, 32, 3, ops.IN_NONE), (32, 8, 3, ops.IN_NONE),
                                (32, 32, 1, ops.IN_NONE), (32, 32, 3, ops.IN_UPSAMPLE2)]:
        assert not ops.conv2d_bf16_supports(cout, cin, k, ZERO, in_op), (cin, cout, k, in_op)
        if k == 3:  # (the entry point is 3x3 only: it has no ksize to get wrong)
            assert call(cin, cout, in_op) == einval, (cin, cout, in_op)
            assert b"conv2d_bf16" in lib.rpst_last_error()
    assert lib.rpst_conv2d_bf16_packed_size(32, 24) == 0 == lib.rpst_conv2d_bf16_packed_size(8, 32)
    with pytest.raises(ValueError, match="conv2d_bf16"):
        ops.pack_conv_weight_bf16(torch.zeros(32, 32, 1, 1, device=cuda))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.conv2d_bf16(torch.zeros(1, 32, 4, 4), buf.bfloat16(), None, 32)
    with pytest.raises(NotImplementedError, match="autograd"):
        ops.conv2d_bf16(torch.zeros(1, 32, 4, 4, device=cuda, requires_grad=True),
                        buf.bfloat16(), None, 32)


# ---- end to end ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _net_case(size):
    """AdaINRPNet (rp_blocks 5, hidden 16, synthetic weights), N = 2 inputs of size^2, the
    float64 oracle and the bf16 emulation (float64 accumulation): CPU, formed once."""
    import network as net
    from rpst import ops
    model = golden_net(net.AdaINRPNet, rp_config(16), None, "", seed=31)
    content, style = gen(40 + size, (2, 3, size, size), 0.5, 0.5), gen(41 + size, (2, 3, size, size), 0.5, 0.5)
    sd = state_dict_of(model)
    oracle = R.adain_rp_test(content.double(), style.double(), {k: v.double() for k, v in sd.items()}, 5)
    emu = B.adain_rp_test_bf16(content, style, sd, 5, lambda co, ci: ops.conv2d_bf16_supports(co, ci))
    return model, content, style, oracle, emu


@pytest.mark.parametrize("size", [24, 48])
def test_adain_rp_bf16_vs_oracle(cuda, size):
    import copy
    cpu_model, content, style, oracle, emu = _net_case(size)
    model = copy.deepcopy(cpu_model).to(cuda)
    c, s = content.to(cuda), style.to(cuda)
    assert model.precision == "fp32"
    y32 = model.test(c, s)
    model.precision = "bf16"
    y16 = model.test(c, s)
    model.precision = "fp32"
    assert torch.equal(model.test(c, s), y32)  # the fp32 path is untouched by a bf16 call
    e_gpu, e_emu = rel_l2(y16, oracle), rel_l2(emu, oracle)
    m_gpu, m_emu = max_abs_ratio(y16, oracle), max_abs_ratio(emu, oracle)
    moved = rel_l2(y16, y32)
    print(f"AdaINRPNet bf16 {size}^2: rel-L2 gpu {e_gpu:.3e} emulation {e_emu:.3e}; max-abs gpu "
          f"{m_gpu:.3e} emulation {m_emu:.3e}; bf16 vs fp32 on the GPU {moved:.3e}")
    assert e_gpu <= 2 * e_emu, (e_gpu, e_emu)
    assert m_gpu <= 2 * m_emu, (m_gpu, m_emu)
    assert moved >= 1e-3, moved  # the bf16 kernels ran


def test_adain_rp_bf16_cache_follows_load_state_dict(cuda):
    import copy

    import network as net
    cpu_model, content, style, _, _ = _net_case(24)
    model = copy.deepcopy(cpu_model).to(cuda)
    model.precision = "bf16"
    c, s = content.to(cuda), style.to(cuda)
    y_a = model.test(c, s)
    other = golden_net(net.AdaINRPNet, rp_config(16), None, "", seed=32)
    model.load_state_dict(other.state_dict())
    y_b = model.test(c, s)
    assert rel_l2(y_b, y_a) > 1e-2
    model.load_state_dict(cpu_model.state_dict())
    assert torch.equal(model.test(c, s), y_a)
