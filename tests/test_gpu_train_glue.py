"""The small kernels of the training path, each on its own against float64 torch autograd on
the CPU (tests/train_glue_ref.py), at the shapes where a per-plane or grid-stride kernel can
go wrong and the whole-model gradient tests never look: their images leave SAModel's
transform planes of 4 to 60 pixels, one pass of every `i += 256` loop with three of four
waves idle. Here: planes under one wave, of exactly one stride (256), one element past it,
several strides, and the production plane (64 x 64); sq_diff_mean on both sides of the grid's
1024 x 256 elements; the float4 body and scalar tail of the ReLU backward.

Bars: 1e-6 where the kernel sums in fp64 and rounds once (mean_variance_norm backward, the
loss seed, sq_diff_mean, the upsample backward's four-term sum): CPU float32 autograd of the
same formulas reads 4e-8 to 1.1e-7 on these inputs, and HW written for HW - 1 moves the
result by 4.5e-6 at the least (tests/test_train_glue_cpu.py), which the project's usual 1e-5
would let through at HW = 4096. AdaIN backward keeps its kernel bar, 1e-5. The elementwise
kernels are compared bit for bit."""
import pytest
import torch

import train_glue_ref as T
from helpers import gen, rel_l2

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", T.MVN_SHAPES)
def test_mean_variance_norm_backward(cuda, shape, accumulate):
    """rpst_mean_variance_norm_backward from the GPU's own y and std, as the SAModel step
    calls it; accumulate = 1 adds into a prefilled dx."""
    from rpst import _lib, ops
    x, dy, pre = T.mvn_inputs(shape)
    ref = T.mvn_backward_ref(x, dy)
    xg = x.to(cuda)
    y = ops.mean_variance_norm(xg)
    std = ops.calc_mean_std(xg)[1].reshape(-1).contiguous()
    dx = pre.to(cuda) if accumulate else torch.empty_like(xg)
    dyg = dy.to(cuda)
    _lib.call("rpst_mean_variance_norm_backward", y.data_ptr(), dyg.data_ptr(), std.data_ptr(),
              dx.data_ptr(), shape[0] * shape[1], shape[2] * shape[3], accumulate,
              ops._stream(xg))
    want = pre.double() + ref if accumulate else ref
    e = rel_l2(dx, want)
    print(f"mvn backward {shape} accumulate {accumulate}: rel-L2 {e:.3e} (bar {T.MVN_BAR:.0e})")
    assert e < T.MVN_BAR, (shape, accumulate, e)


@pytest.mark.parametrize("shape", T.ADAIN_SHAPES)
def test_adain_backward_wrapper(cuda, shape):
    """autograd._adain_backward(g, autograd._adain_state(cf, sf)): the wrapper that sizes the
    workspace and carves [d content; d style] out of one stacked tensor."""
    from rpst import autograd as A
    c, s, g = T.adain_inputs(shape)
    dc_ref, ds_ref = T.adain_backward_ref(c, s, g)
    d = A._adain_backward(g.to(cuda), A._adain_state(c.to(cuda), s.to(cuda)))
    n = shape[0]
    assert tuple(d.shape) == (2 * n,) + tuple(shape[1:])
    for got, ref, name in ((d[:n], dc_ref, "d content"), (d[n:], ds_ref, "d style")):
        e = rel_l2(got, ref)
        print(f"adain backward wrapper {shape} {name}: rel-L2 {e:.3e} (bar 1e-05)")
        assert e < 1e-5, (shape, name, e)


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("wts", T.SEED_WTS)
@pytest.mark.parametrize("content", [False, True])
@pytest.mark.parametrize("shape", T.SEED_SHAPES)
def test_loss_seed(cuda, shape, content, wts, acc):
    """autograd._seed (rpst_style_content_loss_grad): w_s d style_loss(F, T) + w_c d mse(F, Fc)
    with the weights read from the device, the statistics from autograd._stats; content False
    passes no target (the style term alone), acc adds into a prefilled out."""
    from rpst import autograd as A
    F, Tt, Fc, pre = T.seed_inputs(shape)
    Fc = Fc if content else None
    ref = T.seed_ref(F, Tt, Fc, wts)
    Fg, Tg = F.to(cuda), Tt.to(cuda)
    out = pre.to(cuda) if acc else torch.empty_like(Fg)
    A._seed(Fg, None if Fc is None else Fc.to(cuda), A._stats(Fg, Tg),
            torch.tensor(wts, dtype=torch.float32, device=cuda), out, acc)
    want = pre.double() + ref if acc else ref
    e = rel_l2(out, want)
    print(f"loss seed {shape} content {content} wts {wts} acc {acc}: rel-L2 {e:.3e} "
          f"(bar {T.SEED_BAR:.0e})")
    assert e < T.SEED_BAR, (shape, content, wts, acc, e)


@pytest.mark.parametrize("n", T.SQ_DIFF_NS)
def test_sq_diff_mean(cuda, n):
    """autograd.sq_diff_mean: an fp64 sum rounded once, on both sides of the 1024 x 256
    elements the grid covers in one pass; a - a is exactly 0; a second call is bit-equal."""
    from rpst import autograd as A
    a, b = T.sq_diff_inputs(n)
    ref = T.sq_diff_ref(a, b)
    ag, bg = a.to(cuda), b.to(cuda)
    got = A.sq_diff_mean(ag, bg)
    assert got.shape == () and got.dtype == torch.float32
    e = abs(float(got.double()) - ref) / ref
    print(f"sq_diff_mean n = {n}: relative error {e:.3e} (bar {T.SQ_DIFF_BAR:.0e})")
    assert e <= T.SQ_DIFF_BAR, (n, e)
    assert float(A.sq_diff_mean(ag, ag)) == 0.0
    assert torch.equal(A.sq_diff_mean(ag, bg), got)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4099])
def test_relu_backward_kernels_bitwise(cuda, n):
    """relu_backward and act_backward(., ., ACT_LRELU): the float4 body and the scalar tail
    (chosen by i + 3 < n) with +0.0, -0.0 and negative y among the outputs they threshold
    by: g where y > 0, else 0 / 0.2 g, bit for bit."""
    from rpst import autograd as A
    from rpst import ops
    g = gen(21, (n,))
    y = gen(22, (n,))
    y[0::5] = 0.0
    y[2::5] = -0.0
    gg, yg = g.to(cuda), y.to(cuda)
    relu = A.relu_backward(gg, yg).cpu()
    assert torch.equal(relu, torch.where(y > 0, g, torch.zeros(n)))
    assert torch.equal(A.act_backward(gg, yg, ops.ACT_RELU).cpu(), relu)
    lrelu = A.act_backward(gg, yg, ops.ACT_LRELU).cpu()
    assert torch.equal(lrelu, torch.where(y > 0, g, g * 0.2))
    assert A.act_backward(gg, yg, ops.ACT_NONE) is gg


@pytest.mark.parametrize("shape", T.UPSAMPLE_G_SHAPES)
def test_upsample_backward(cuda, shape):
    """autograd._upsample_backward: each output is a fixed-order sum of four floats."""
    from rpst import autograd as A
    g = gen(23, shape)
    ref = T.upsample_backward_ref(g)
    dx = A._upsample_backward(g.to(cuda))
    assert tuple(dx.shape) == tuple(ref.shape)
    e = rel_l2(dx, ref)
    print(f"upsample backward {shape}: rel-L2 {e:.3e} (bar 1e-06)")
    assert e < 1e-6, (shape, e)
