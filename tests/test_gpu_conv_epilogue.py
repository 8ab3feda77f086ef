"""GPU parity of the F(4x4) kernels' epilogue context (rpst_wino4q.hip, rpst_wino4.hip).

The position-quarter kernel derives what its epilogue needs besides the tile (tile origin,
ragged row and column counts, store flags, the image's output descriptor, the statistics
partial's address, per-lane row offsets) once per block into LDS and reads it back per
channel; the channel's plane offset is a running value. A record that is stale, shared between
tile rows or images, or a running offset that is off by a plane shows as a wrong output or
wrong statistics, never as a fault. The shapes are the smallest that make each field matter:
ragged last row band and column tile with a skipped image, three images in one launch, the
non-buffer store path (W % 4 != 0) with the border-class bias table, a ragged co tile, the
pooled store. Each runs on the quarter kernel and on the 32-channel kernel where it takes it.

Bars: the output against an fp64 torch convolution on the CPU at rel-L2 1e-5 (the single-conv
bar of test_conv2d_vs_torch); mean and std per (n, c) against torch.var_mean of that fp64
output at rel-L2 1e-6 (test_conv2d_stats_equal_calc_mean_std's bar).
"""
import functools

import pytest
import torch

from helpers import gen, rel_l2
from oracle import restate as R
from test_gpu_kernels import _conv_ref

pytestmark = pytest.mark.gpu

TOL_OUT = 1e-5
TOL_STAT = 1e-6
EPS = 1e-5


@pytest.fixture
def kernel(request, monkeypatch):
    """F(4x4) forced; quarter = 2 (the position-quarter kernel on every shape it supports)
    or 0 (the 32-channel kernel) through the calling thread's switch."""
    from rpst import _lib
    monkeypatch.setenv("RPST_CONV_ALGO", "winograd4")
    lib = _lib.load()
    old = lib.rpst_conv2d_set_quarter(request.param)
    yield request.param
    lib.rpst_conv2d_set_quarter(old)


BOTH = pytest.mark.parametrize("kernel", [2, 0], indirect=True, ids=["quarter", "w32"])
W32 = pytest.mark.parametrize("kernel", [0], indirect=True, ids=["w32"])


def _takes(kernel, cout, cin, h, w, in_op=0):
    from rpst import _lib
    lib = _lib.load()
    assert lib.rpst_conv2d_algorithm(cout, cin, h, w, 3, in_op) == 2  # F(4x4)
    assert lib.rpst_conv2d_quarter(cout, cin, h, w, 3, in_op) == int(kernel == 2)


@functools.lru_cache(maxsize=None)
def _problem(seed, n, cin, h, w, cout, pad, in_op, act):
    """Inputs and the fp64 reference of one case (formed once, shared, never modified);
    act: 0 none, 1 ReLU, 2 LeakyReLU(0.2)."""
    x = gen(seed, (n, cin, h, w), 1.0, 0.2)
    wt = gen(seed + 1, (cout, cin, 3, 3), (2.0 / (cin * 9)) ** 0.5)
    b = gen(seed + 2, (cout,), 0.05)
    ref = _conv_ref(x.double(), wt.double(), b.double(), pad, in_op, act == 1)
    if act == 2:
        ref = torch.nn.functional.leaky_relu(ref, 0.2)
    return x, wt, b, ref


def _stats_ref(ref):
    var, mean = torch.var_mean(ref, dim=(2, 3), unbiased=True, keepdim=True)
    return mean, (var + EPS).sqrt()


def _check_stats(what, mean, std, ref):
    m2, s2 = _stats_ref(ref)
    em, es = rel_l2(mean, m2), rel_l2(std, s2)
    print(f"{what}: mean {em:.3e} std {es:.3e}")
    assert em < TOL_STAT and es < TOL_STAT, (em, es)


@BOTH
def test_ragged_tiles_stats_skipped_image(cuda, kernel):
    """(2, 128, 13, 72) -> 256, zero padding, statistics, store_n = 1: two column tiles and two
    row bands whose last ones are ragged, four co tiles, image 1 in the statistics only and
    its output memory untouched (sentinel, through the C ABI)."""
    from rpst import _lib, ops
    n, cin, h, w, cout = 2, 128, 13, 72, 256
    _takes(kernel, cout, cin, h, w)
    x, wt, b, ref = _problem(80, n, cin, h, w, cout, 0, 0, 1)
    x, b, p = x.to(cuda), b.to(cuda), ops.pack_conv_weight(wt.to(cuda))
    lib = _lib.load()
    nbytes = lib.rpst_conv2d_stats_workspace_size(n, cin, h, w, cout, 3, ops.IN_NONE)
    ws_t = torch.empty(nbytes, device=cuda, dtype=torch.uint8)
    sentinel = -12345.0
    out = torch.full((n, cout, h, w), sentinel, device=cuda)
    mean = torch.empty((n, cout, 1, 1), device=cuda)
    std = torch.empty_like(mean)
    _lib.call("rpst_conv2d_stats_store", x.data_ptr(), None, p.data_ptr(), b.data_ptr(), None,
              out.data_ptr(), n, cin, h, w, cout, 3, ops.PAD_ZERO, ops.IN_NONE, ops.ACT_RELU,
              mean.data_ptr(), std.data_ptr(), EPS, 1, ws_t.data_ptr(), nbytes,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    err = rel_l2(out[:1], ref[:1])
    print(f"ragged stats kernel {kernel}: out {err:.3e}")
    assert err < TOL_OUT, err
    assert (out[1:] == sentinel).all()
    _check_stats(f"ragged stats kernel {kernel}", mean, std, ref)


@BOTH
def test_three_images_reflect(cuda, kernel):
    """(3, 128, 16, 128) -> 64, reflect padding, no statistics: the blocks of three images
    in one launch, each with its own record."""
    from rpst import ops
    n, cin, h, w, cout = 3, 128, 16, 128, 64
    _takes(kernel, cout, cin, h, w)
    x, wt, b, ref = _problem(83, n, cin, h, w, cout, 1, 0, 1)
    out = ops.conv2d(x.to(cuda), ops.pack_conv_weight(wt.to(cuda)), b.to(cuda), cout, 3,
                     pad=ops.PAD_REFLECT, relu=True)
    for i in range(n):
        err = rel_l2(out[i:i + 1], ref[i:i + 1])
        print(f"three images kernel {kernel} image {i}: {err:.3e}")
        assert err < TOL_OUT, (i, err)


@functools.lru_cache(maxsize=None)
def _folded_problem():
    n, cin, h, w, cout = 1, 256, 9, 70, 128
    c = gen(86, (n, cin, h, w), 2.0, 0.5).clamp_min(0)
    s = gen(87, (n, cin, h, w), 1.0, 1.0).clamp_min(0)
    wt = gen(88, (cout, cin, 3, 3), 0.08)
    b = gen(89, (cout,), 0.05)
    ref = _conv_ref(R.adain(c, s).double(), wt.double(), b.double(), 0, 0, True)
    return c, s, wt, b, ref


@BOTH
def test_folded_adain_border_classes_unaligned_width(cuda, kernel):
    """(1, 256, 9, 70) -> 128 with AdaIN folded into per-image weights, zero padding: the
    border-class bias table on every edge tile, and W % 4 != 0, so the plain store path with
    its per-element column masks."""
    from rpst import ops
    n, cin, h, w, cout = 1, 256, 9, 70, 128
    _takes(kernel, cout, cin, h, w)
    c, s, wt, b, ref = _folded_problem()
    mc, sc = R.calc_mean_std(c)
    ms, ss = R.calc_mean_std(s)
    aux = ops.adain_params(mc, sc, ms, ss).to(cuda)
    out = ops.conv2d(c.to(cuda), ops.pack_conv_weight(wt.to(cuda)), b.to(cuda), cout, 3,
                     pad=ops.PAD_ZERO, in_op=ops.IN_ADAIN, aux=aux, relu=True, fold=True)
    err = rel_l2(out, ref)
    print(f"folded kernel {kernel}: {err:.3e}")
    assert err < TOL_OUT, err


@BOTH
def test_ragged_co_tile_leaky_relu(cuda, kernel):
    """(1, 128, 8, 64) -> 96, LeakyReLU: Cout is no multiple of either kernel's co tile, so
    the running channel offset passes the last real channel under the channel masks."""
    from rpst import ops
    n, cin, h, w, cout = 1, 128, 8, 64, 96
    _takes(kernel, cout, cin, h, w)
    x, wt, b, ref = _problem(90, n, cin, h, w, cout, 0, 0, 2)
    out = ops.conv2d(x.to(cuda), ops.pack_conv_weight(wt.to(cuda)), b.to(cuda), cout, 3,
                     pad=ops.PAD_ZERO, relu=ops.ACT_LRELU)
    err = rel_l2(out, ref)
    print(f"lrelu kernel {kernel}: {err:.3e}")
    assert err < TOL_OUT, err
    assert (out < 0).any()  # the negative branch is live


@W32
@pytest.mark.parametrize("shape", [(1, 64, 20, 130, 128), (2, 16, 7, 66, 32)])
def test_w32_stats(cuda, kernel, shape):
    """The 32-channel kernel's statistics epilogue: four co tiles over an interior and a
    ragged column tile, and the 8-row block with two images."""
    from rpst import ops
    n, cin, h, w, cout = shape
    _takes(kernel, cout, cin, h, w)
    x, wt, b, ref = _problem(93 + cin, n, cin, h, w, cout, 0, 0, 1)
    out, mean, std = ops.conv2d_stats(x.to(cuda), ops.pack_conv_weight(wt.to(cuda)), b.to(cuda),
                                      cout, 3, relu=True)
    err = rel_l2(out, ref)
    print(f"w32 stats {shape}: out {err:.3e}")
    assert err < TOL_OUT, err
    _check_stats(f"w32 stats {shape}", mean, std, ref)


@BOTH
def test_pooled_output(cuda, kernel):
    """(1, 128, 11, 35) upsampled -> 96 with the 2x2 ceil-mode max pool in the epilogue
    (pool_out): the smallest pooled shape of test_conv2d_pool_matches_conv_then_pool that both
    kernels take, here against the pooled fp64 convolution."""
    from rpst import ops
    n, cin, hs, ws, cout = 1, 128, 11, 35, 96
    _takes(kernel, cout, cin, hs, ws, ops.IN_UPSAMPLE2)
    x, wt, b, ref = _problem(96, n, cin, hs, ws, cout, 1, ops.IN_UPSAMPLE2, 0)
    ref = torch.nn.functional.max_pool2d(ref, 2, 2, 0, ceil_mode=True)
    x = x.to(cuda)
    assert ops.conv2d_pool_fuses(x, cout, 3, ops.IN_UPSAMPLE2)
    out = ops.conv2d_pool(x, ops.pack_conv_weight(wt.to(cuda)), b.to(cuda), cout, 3,
                          pad=ops.PAD_REFLECT, in_op=ops.IN_UPSAMPLE2, relu=False)
    assert out.shape == ref.shape
    err = rel_l2(out, ref)
    print(f"pooled kernel {kernel}: {err:.3e}")
    assert err < TOL_OUT, err
