"""GPU parity of the F(4x4) kernels' LDS-DMA ring addressing (rpst_wino4q.hip, rpst_wino4.hip).

A wave copies contiguous 1-KiB pieces of a step's weight slice from one M0 and one scalar
offset, the piece in the instruction offset, and the step-uniform values (soffsets, live
tests, descriptors) are formed once per step. A wrong target leaves a stage partly stale or
partly overwritten, which shows as a wrong result, never as a fault. The shapes are the
smallest that take each addressing path: one ring turn per co tile (every look-ahead issue
of the last turn dead), ragged and multiple co tiles (the post-epilogue wait path), a tile
that is both x edges, interior 16-B blocks, the 4-B patch path (W % 4 != 0), the upsample
loader, the statistics epilogue with a store head and the per-image folded weights.

Bar: rel-L2 1e-5 against an fp64 reference, the single-conv bar of test_conv2d_vs_torch
(F(4x4) measures about 2e-6 at Cin = 128).
"""
import functools

import pytest
import torch

from helpers import gen, rel_l2
from oracle import restate as R
from test_gpu_kernels import _conv_ref

pytestmark = pytest.mark.gpu

# (Cin, Cout, H, W) of the source, N = 2
QUARTER_CASES = [
    (16, 64, 8, 64),      # K4 = 4: one ring turn per co tile; one tile that is both x edges
    (48, 80, 12, 128),    # ragged co tile; two column tiles, both edge tiles
    (128, 192, 16, 192),  # three co tiles (post-epilogue wait twice); interior block at x0 = 64
    (144, 64, 9, 70),     # W % 4 != 0: the 4-B patch path; K4 = 36
]
W32_CASES = [(16, 32, 8, 64), (32, 16, 20, 70), (64, 128, 16, 192), (8, 32, 8, 64)]  # last: NR = 2
N = 2


def _algo(monkeypatch, quarter):
    monkeypatch.setenv("RPST_CONV_ALGO", "winograd4")
    monkeypatch.setenv("RPST_W4Q", "2" if quarter else "0")


@functools.lru_cache(maxsize=None)
def _problem(cin, cout, h, w, pad, in_op):
    """Inputs and the fp64 reference of one case (formed once, shared, never modified)."""
    x = gen(70, (N, cin, h, w), 1.0, 0.2)
    wt = gen(71, (cout, cin, 3, 3), (2.0 / (cin * 9)) ** 0.5)
    b = gen(72, (cout,), 0.05)
    ref = _conv_ref(x.double(), wt.double(), b.double(), pad, in_op, True)
    return x, wt, b, ref


def _run(cuda, cin, cout, h, w, pad, in_op, quarter):
    from rpst import _lib, ops
    x, wt, b, ref = _problem(cin, cout, h, w, pad, in_op)
    assert _lib.load().rpst_conv2d_algorithm(cout, cin, h, w, 3, in_op) == 2  # F(4x4)
    assert _lib.load().rpst_conv2d_quarter(cout, cin, h, w, 3, in_op) == int(quarter)
    out = ops.conv2d(x.to(cuda), ops.pack_conv_weight(wt.to(cuda)), b.to(cuda), cout, 3, pad=pad,
                     in_op=in_op, relu=True)
    assert out.shape == ref.shape
    return out, ref


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("case", QUARTER_CASES)
def test_quarter_ring(cuda, monkeypatch, case, pad):
    _algo(monkeypatch, True)
    out, ref = _run(cuda, *case, pad, 0, True)
    err = rel_l2(out, ref)
    print(f"quarter {case} pad {pad}: rel-L2 {err:.3e}")
    assert err < 1e-5, err


@pytest.mark.parametrize("pad", [0, 1])
def test_quarter_ring_upsample(cuda, monkeypatch, pad):
    from rpst import ops
    _algo(monkeypatch, True)
    out, ref = _run(cuda, 128, 64, 6, 40, pad, ops.IN_UPSAMPLE2, True)
    err = rel_l2(out, ref)
    print(f"quarter upsample pad {pad}: rel-L2 {err:.3e}")
    assert err < 1e-5, err


@pytest.mark.parametrize("pad", [0, 1])
def test_quarter_ring_stats_store_head(cuda, monkeypatch, pad):
    """Statistics epilogue with store_n = 1: the stored image against fp64, every image's
    statistics against those of the fp64 result."""
    from rpst import ops
    _algo(monkeypatch, True)
    cin, cout, h, w = 128, 64, 8, 64
    x, wt, b, ref = _problem(cin, cout, h, w, pad, 0)
    out, mean, std = ops.conv2d_stats(x.to(cuda), ops.pack_conv_weight(wt.to(cuda)), b.to(cuda),
                                      cout, 3, pad=pad, relu=True, store_n=1)
    err = rel_l2(out[:1], ref[:1])
    m2, s2 = R.calc_mean_std(ref)
    em, es = rel_l2(mean, m2), rel_l2(std, s2)
    print(f"quarter stats pad {pad}: out {err:.3e} mean {em:.3e} std {es:.3e}")
    assert err < 1e-5, err
    assert em < 1e-5 and es < 1e-5, (em, es)


@pytest.mark.parametrize("pad", [0, 1])
def test_quarter_ring_folded_adain(cuda, monkeypatch, pad):
    """256 -> 128 with AdaIN folded into per-image weights at N = 2: image 1's slices start one
    weight image further on (the per-image stride in the scalar offset)."""
    from rpst import _lib, ops
    _algo(monkeypatch, True)
    cin, cout, h, w = 256, 128, 9, 72
    c = gen(60, (N, cin, h, w), 2.0, 0.5).clamp_min(0)
    s = gen(61, (N, cin, h, w), 1.0, 1.0).clamp_min(0)
    wt = gen(62, (cout, cin, 3, 3), 0.08)
    b = gen(63, (cout,), 0.05)
    mc, sc = R.calc_mean_std(c)
    ms, ss = R.calc_mean_std(s)
    aux = ops.adain_params(mc, sc, ms, ss).to(cuda)
    assert _lib.load().rpst_conv2d_quarter(cout, cin, h, w, 3, 0) == 1
    out = ops.conv2d(c.to(cuda), ops.pack_conv_weight(wt.to(cuda)), b.to(cuda), cout, 3, pad=pad,
                     in_op=ops.IN_ADAIN, aux=aux, relu=True, fold=True)
    ref = _conv_ref(R.adain(c, s).double(), wt.double(), b.double(), pad, 0, True)
    err = rel_l2(out, ref)
    print(f"quarter folded pad {pad}: rel-L2 {err:.3e}")
    assert err < 1e-5, err


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("case", W32_CASES)
def test_w32_ring(cuda, monkeypatch, case, pad):
    _algo(monkeypatch, False)
    out, ref = _run(cuda, *case, pad, 0, False)
    err = rel_l2(out, ref)
    print(f"w32 {case} pad {pad}: rel-L2 {err:.3e}")
    assert err < 1e-5, err


def test_w32_ring_adain_loader(cuda, monkeypatch):
    from rpst import ops
    _algo(monkeypatch, False)
    cin, cout, h, w = 32, 16, 20, 70
    c = gen(60, (N, cin, h, w), 2.0, 0.5).clamp_min(0)
    s = gen(61, (N, cin, h, w), 1.0, 1.0).clamp_min(0)
    wt = gen(62, (cout, cin, 3, 3), 0.08)
    b = gen(63, (cout,), 0.05)
    mc, sc = R.calc_mean_std(c)
    ms, ss = R.calc_mean_std(s)
    aux = ops.adain_params(mc, sc, ms, ss).to(cuda)
    out = ops.conv2d(c.to(cuda), ops.pack_conv_weight(wt.to(cuda)), b.to(cuda), cout, 3, pad=0,
                     in_op=ops.IN_ADAIN, aux=aux, relu=True, fold=False)
    ref = _conv_ref(R.adain(c, s).double(), wt.double(), b.double(), 0, 0, True)
    err = rel_l2(out, ref)
    print(f"w32 adain loader: rel-L2 {err:.3e}")
    assert err < 1e-5, err


def test_quarter_ring_not_stale(cuda, monkeypatch):
    """A piece that is never copied would leave another launch's weights in the stage: the
    three-co-tile case, the one-turn case, then the first again, bit for bit."""
    _algo(monkeypatch, True)
    first, ref = _run(cuda, *QUARTER_CASES[2], 0, 0, True)
    _run(cuda, *QUARTER_CASES[0], 0, 0, True)
    again, _ = _run(cuda, *QUARTER_CASES[2], 0, 0, True)
    assert rel_l2(first, ref) < 1e-5
    assert torch.equal(first, again)
