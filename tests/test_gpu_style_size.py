"""A style image of another size than the content: the rectangular SANet attention core
(HWq queries, HWk keys), the WCT with two pixel counts, and the modules / models built on them,
against float64, the CPU oracle (which reads each side's own size) and the equal-size entries."""
import contextlib
import copy

import pytest
import torch

from helpers import (TOL_NET, TOL_NET_MAXABS, TOL_WCT, gen, max_abs_ratio, rel_l2, rp_config,
                     state_dict_of, synth_, unfused)
from oracle import restate as R

pytestmark = pytest.mark.gpu

FLASH_C = (64, 128, 256, 512)


def _attn_ref(F, G, H, dtype=torch.float64):
    """O = H softmax(F^T G)^T (sanet.py:86-94) with G and H of their own size -> F's shape."""
    B, C = F.shape[:2]
    S = torch.bmm(F.reshape(B, C, -1).to(dtype).permute(0, 2, 1), G.reshape(B, C, -1).to(dtype))
    O = torch.bmm(H.reshape(B, C, -1).to(dtype), torch.softmax(S, -1).permute(0, 2, 1))
    return O.view(F.shape)


def _flash_rule(C, hwq, hwk):
    """include/rpst.h, rpst_sanet_attention_qk: flash for C in {64, 128, 256, 512} and
    HWk % 4 == 0; HWq needs no alignment."""
    return C in FLASH_C and hwk % 4 == 0


def _attn_bar(F, G, H, ref, err, what):
    """1e-5 (test_sanet_attention_flash_shapes' bar); where a case reads above it,
    max(1e-5, 3 x the error of CPU fp32 torch on the same inputs): test_gpu_ld.py's rule."""
    bar = 1e-5
    if err >= bar:
        floor = rel_l2(_attn_ref(F, G, H, torch.float32), ref)
        bar = max(1e-5, 3 * floor)
        print(f"{what}: rel-L2 {err:.3e}, CPU fp32 floor {floor:.3e}, bar {bar:.3e}")
    else:
        print(f"{what}: rel-L2 {err:.3e}, bar {bar:.3e}")
    return bar


def _qk(B, C, q, k, seeds=(31, 32, 33), scale=0.6):
    return (gen(seeds[0], (B, C) + q, scale), gen(seeds[1], (B, C) + k, scale),
            gen(seeds[2], (B, C) + k, 1.0))


ATTN_CASES = [
    # fewer than 64 queries; 180 keys ragged against the 16-key block
    pytest.param(2, 64, (5, 4), (12, 15), True, id="c64-20q-180k"),
    # fewer keys than one key block; a ragged last query block
    pytest.param(2, 128, (9, 20), (3, 4), True, id="c128-180q-12k"),
    pytest.param(3, 256, (8, 8), (5, 4), True, id="c256-64q-20k"),
    pytest.param(2, 512, (16, 17), (8, 9), True, id="c512-272q-72k"),
    # odd query count: flash (rpst.h: HWq needs no alignment)
    pytest.param(2, 64, (7, 9), (8, 8), True, id="c64-63q-64k"),
    # materialised: C is no flash width
    pytest.param(2, 40, (6, 6), (5, 7), False, id="c40-materialised"),
    # materialised: key count not a multiple of 4
    pytest.param(2, 64, (6, 6), (5, 7), False, id="c64-35k-materialised"),
]


@pytest.mark.parametrize("B,C,q,k,flash", ATTN_CASES)
def test_attention_qk_vs_float64(cuda, B, C, q, k, flash):
    """The rectangular core on both orders (HWq > HWk, HWq < HWk), B >= 2 so that a plane stride
    taken from the wrong count shows, every flash width and both materialised reasons; which
    path ran is the workspace query's answer (0 bytes: flash), checked against rpst.h's rule.
    Two calls give identical bits."""
    from rpst import _lib, ops
    hwq, hwk = q[0] * q[1], k[0] * k[1]
    ws = _lib.load().rpst_sanet_attention_qk_workspace_size_c(B, C, hwq, hwk)
    assert (ws == 0) == flash == _flash_rule(C, hwq, hwk)
    if not flash:
        assert ws == 4 * (B * hwq * hwk + 2 * B * hwq)
    F, G, H = _qk(B, C, q, k)
    ref = _attn_ref(F, G, H)
    out = ops.sanet_attention(F.to(cuda), G.to(cuda), H.to(cuda))
    assert out.shape == F.shape
    err = rel_l2(out, ref)
    assert err < _attn_bar(F, G, H, ref, err, f"attention {(B, C, q, k)}")
    assert torch.equal(out, ops.sanet_attention(F.to(cuda), G.to(cuda), H.to(cuda)))


def test_attention_qk_large_logits(cuda):
    """|S| max > 60 (inputs as test_sanet_attention_large_logits builds them): the max
    subtraction of the online softmax over 180 keys for 180 queries of another image size."""
    from rpst import ops
    B, C, q, k = 2, 128, (9, 20), (12, 15)
    F, G, H = gen(5, (B, C) + q, 2.5), gen(6, (B, C) + k, 2.5), gen(7, (B, C) + k, 1.0)
    S = torch.bmm(F.view(B, C, -1).permute(0, 2, 1).double(), G.view(B, C, -1).double())
    assert S.abs().max() > 60
    ref = _attn_ref(F, G, H)
    out = ops.sanet_attention(F.to(cuda), G.to(cuda), H.to(cuda))
    err = rel_l2(out, ref)
    assert err < _attn_bar(F, G, H, ref, err,
                           f"large logits |S| max {float(S.abs().max()):.1f}")


@pytest.mark.parametrize("B,C,q,k", [(2, 64, (9, 20), (7, 12)), (2, 256, (5, 8), (12, 15))])
def test_attention_qk_ragged_tail_nan_after_tensor(cuda, B, C, q, k):
    """HWk % 16 != 0 and HWq % 64 != 0: the last key block of the last channel row of the last
    image reaches past G and H, whose descriptors now end at the key plane (C x HWk), and the
    last query block past F. Each tensor sits at the front of its own NaN-filled buffer; the
    output is finite and within the bar."""
    from rpst import ops
    assert (k[0] * k[1]) % 16 != 0 and (k[0] * k[1]) % 4 == 0 and (q[0] * q[1]) % 64 != 0

    def at_front_of_nan(x):
        buf = torch.full((x.numel() + 4096,), float("nan"), device=cuda)
        v = buf[:x.numel()].view(x.shape)
        v.copy_(x)
        return v
    F, G, H = _qk(B, C, q, k, seeds=(51, 52, 53))
    out = ops.sanet_attention(*(at_front_of_nan(x.to(cuda)) for x in (F, G, H)))
    assert torch.isfinite(out).all()
    ref = _attn_ref(F, G, H)
    err = rel_l2(out, ref)
    assert err < _attn_bar(F, G, H, ref, err, f"nan guard {(B, C, q, k)}")


# ---- equal sizes are untouched -------------------------------------------------------------
def _call_qk(F, G, H):
    from rpst import _lib
    B, C = F.shape[:2]
    hwq, hwk = F.shape[2] * F.shape[3], G.shape[2] * G.shape[3]
    out = torch.empty_like(F)
    nbytes = _lib.load().rpst_sanet_attention_qk_workspace_size_c(B, C, hwq, hwk)
    ws = _lib.scratch(nbytes, F)
    _lib.call("rpst_sanet_attention_qk", F.data_ptr(), G.data_ptr(), H.data_ptr(),
              out.data_ptr(), B, C, hwq, hwk, ws.data_ptr(), nbytes,
              torch.cuda.current_stream().cuda_stream)
    return out


def _call_square(F, G, H):
    from rpst import _lib
    B, C, h, w = F.shape
    out = torch.empty_like(F)
    nbytes = _lib.load().rpst_sanet_attention_workspace_size_c(B, C, h * w)
    assert nbytes == _lib.load().rpst_sanet_attention_qk_workspace_size_c(B, C, h * w, h * w)
    ws = _lib.scratch(nbytes, F)
    _lib.call("rpst_sanet_attention", F.data_ptr(), G.data_ptr(), H.data_ptr(), out.data_ptr(),
              B, C, h * w, ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    return out


@pytest.mark.parametrize("shape", [(2, 128, 9, 20), (1, 40, 15, 17)])
def test_attention_equal_sizes_one_body(cuda, shape):
    """ops.sanet_attention at equal sizes, the one-count entry and the rectangular entry with
    HWq = HWk give the same bits (flash and materialised)."""
    from rpst import ops
    F, G, H = (gen(s, shape, 0.6).to(cuda) for s in (31, 32, 33))
    a = ops.sanet_attention(F, G, H)
    assert torch.equal(a, _call_qk(F, G, H)) and torch.equal(a, _call_square(F, G, H))


def test_wct_fuse_equal_sizes_one_body(cuda):
    """rpst_wct_fuse and rpst_wct_fuse_cs with HWc = HWs: the same bits, the same workspace."""
    from rpst import _lib, ops
    lib = _lib.load()
    n, C, h, w = 2, 32, 10, 13
    c = gen(11, (n, C, h, w), 2.0, 0.3, relu=True).to(cuda)
    s = gen(12, (n, C, h, w), 1.5, 0.5, relu=True).to(cuda)
    nbytes = lib.rpst_wct_workspace_size(n, C, h * w)
    assert nbytes == lib.rpst_wct_workspace_size_cs(n, C, h * w, h * w)
    outs = []
    for name, counts in (("rpst_wct_fuse", (h * w,)), ("rpst_wct_fuse_cs", (h * w, h * w))):
        out = torch.empty_like(c)
        ws = _lib.scratch(nbytes, c)
        _lib.call(name, c.data_ptr(), s.data_ptr(), out.data_ptr(), n, C, *counts, None,
                  ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], ops.wct_fuse(c, s))


# ---- WCT against the oracle ----------------------------------------------------------------
# cov_syrk_kernel's split-K (rpst_wct_mat.hip, cov_layout): kper = HW / kCovSplits (8) rounded
# up to whole kCovBK = 32 stages, ksplit = ceil(HW / kper). 64 pixels: 2 splits of 32; 272
# pixels: 5 splits of 64 -- past the 8 x 32 = 256 boundary where kper doubles.
WCT_CASES = [
    pytest.param(16, (12, 20), (9, 8), id="c16-240x72px"),
    pytest.param(32, (10, 13), (16, 24), id="c32-130x384px"),
    pytest.param(16, (8, 8), (16, 17), id="c16-splitk-2of32-vs-5of64"),
    # C > 256: the tiled fp64 SYRK (gemm_f64_kernel) instead of cov_syrk_kernel
    pytest.param(264, (33, 32), (40, 30), id="c264-tiled-1056x1200px"),
]


def _wct_inputs(C, hc, hs):
    return (gen(11, (2, C) + hc, 2.0, 0.3, relu=True), gen(12, (2, C) + hs, 1.5, 0.5, relu=True))


@pytest.mark.parametrize("C,hc,hs", WCT_CASES)
def test_wct_fuse_and_params_vs_oracle(cuda, C, hc, hs):
    """ops.wct_fuse and T cF + c from ops.wct_params against the oracle, n = 2 distinct images,
    both pixel counts >= 4 C. Smallest eigenvalue over both images of (Cc + 1e-4 I, Cs + 1e-4 I,
    Mid's argument Sc Cs Sc + 1e-4 I) in the oracle, against its 1e-5 truncation:
      c16-240x72px      1.313, 1.075e-1, 1.674e-1
      c32-130x384px     1.157, 2.259e-1, 3.215e-1
      c16-splitk        1.161, 2.509e-1, 3.650e-1
      c264-tiled        1.146, 1.278e-1, 1.888e-1
    (test_style_size_cpu.py::test_wct_cases_are_conditioned keeps them above 1e-2).
    status is 0 for every image, and rpst_wct_status_cs reads the same workspace."""
    from rpst import ops
    c, s = _wct_inputs(C, hc, hs)
    ref = R.wct_fuse(c, s)
    out, st = ops.wct_fuse(c.to(cuda), s.to(cuda), status=True)
    assert out.shape == c.shape and st.tolist() == [0, 0]
    err = rel_l2(out, ref)
    T, off, res, st2 = ops.wct_params(c.to(cuda), s.to(cuda), status=True)
    assert st2.tolist() == [0, 0]
    prod = (torch.bmm(T, c.to(cuda).double().flatten(2)) + off[:, :, None]).view(c.shape)
    errp = rel_l2(prod, ref)
    print(f"wct {C, hc, hs}: fuse rel-L2 {err:.3e}, T cF + c rel-L2 {errp:.3e}, bar {TOL_WCT}")
    assert err < TOL_WCT and errp < TOL_WCT
    # each image alone gives the same bits: the split-K is a function of its side's own count
    solo = ops.wct_fuse(c[1:].to(cuda), s[1:].to(cuda))
    assert torch.equal(solo[0], out[1])


def test_wct_params_with_means(cuda):
    """means (2n, C), content rows first, each side's over its own pixels: the same matrices
    as without (the epilogue means of the fused WCTRPNet.test)."""
    from rpst import ops
    c, s = (x.to(cuda) for x in _wct_inputs(32, (10, 13), (16, 24)))
    means = torch.cat([c.mean((2, 3)), s.mean((2, 3))], 0)
    T0, o0, _ = ops.wct_params(c, s)
    T1, o1, _ = ops.wct_params(c, s, means=means)
    assert rel_l2(T1, T0) < 1e-9 and rel_l2(o1, o0) < 1e-9


# ---- modules and models --------------------------------------------------------------------
@pytest.mark.parametrize("B,C,q,k", [(2, 64, (12, 10), (9, 14)), (3, 48, (7, 9), (5, 6))])
def test_sanet_module_vs_oracle(cuda, B, C, q, k):
    import network as net
    mod = net.SANet(C)
    synth_(mod, 3)
    sd = state_dict_of(mod)
    c = gen(1, (B, C) + q, 2.0, 0.5, relu=True)
    s = gen(2, (B, C) + k, 2.0, 0.5, relu=True)
    ref = R.sanet(c, s, sd, "")
    with torch.no_grad():
        out = mod.to(cuda)(c.to(cuda), s.to(cuda))
    assert out.shape == c.shape
    assert rel_l2(out, ref) < 1e-5, rel_l2(out, ref)


def test_transform_vs_oracle(cuda):
    import network as net
    tr = net.Transform(64)
    synth_(tr, 60)
    sd = state_dict_of(tr)
    xs = [gen(70 + i, (2, 64) + hw, 2.0, 0.5, relu=True)
          for i, hw in enumerate([(16, 12), (12, 20), (8, 6), (6, 10)])]  # c4, s4, c5, s5
    ref = R.transform(*xs, sd, "")
    with torch.no_grad():
        out = tr.to(cuda)(*(x.to(cuda) for x in xs))
    assert rel_l2(out, ref) < 1e-5, rel_l2(out, ref)


@pytest.fixture(scope="module")
def samodel_case(cuda):
    """SAModel.test at content (2, 3, 64, 48), style (2, 3, 48, 80): the smallest sizes whose
    relu4_1 map is even on both axes. -> (model on the GPU, content, style, oracle output)."""
    import network as net
    from rpst import synth
    m = net.SAModel({}, copy.deepcopy(net.vgg), 0, 64)
    synth_(m, 4)
    sd = state_dict_of(m)
    c = torch.from_numpy(synth.image(3, (2, 3, 64, 48)))
    s = torch.from_numpy(synth.image(4, (2, 3, 48, 80)))
    return m.to(cuda), c, s, R.samodel_test(c, s, sd)


def test_samodel_test_vs_oracle(cuda, samodel_case):
    m, c, s, ref = samodel_case
    out = m.test(c.to(cuda), s.to(cuda))
    assert out.shape == ref.shape
    print(f"SAModel.test: rel-L2 {rel_l2(out, ref):.3e}, max-abs {max_abs_ratio(out, ref):.3e}")
    assert rel_l2(out, ref) < TOL_NET and max_abs_ratio(out, ref) < TOL_NET_MAXABS


def test_samodel_batch_independence(cuda, samodel_case):
    """Image 1 of the different-size batch of 2 has the bits of the same pair run alone."""
    m, c, s, _ = samodel_case
    both = m.test(c.to(cuda), s.to(cuda))
    solo = m.test(c[1:].to(cuda), s[1:].to(cuda))
    assert torch.equal(both[1], solo[0])


@pytest.fixture(scope="module")
def wct_case(cuda):
    """WCTRPNet (hidden 16, rp_blocks 3) at content (2, 3, 24, 40), style (2, 3, 33, 19)."""
    import network as net
    from rpst import synth
    m = net.WCTRPNet(rp_config(16, 3), copy.deepcopy(net.vgg))
    synth_(m, 6)
    sd = state_dict_of(m)
    c = torch.from_numpy(synth.image(5, (2, 3, 24, 40)))
    s = torch.from_numpy(synth.image(6, (2, 3, 33, 19)))
    return m.to(cuda), c, s, R.wct_rp_test(c, s, sd, 3)


def test_wct_rp_test_vs_oracle(cuda, wct_case):
    """Fused (epilogue means of each side's own encoder run, rpst_conv2d_mix) and op by op
    (FUSED_WCT off: encode_both twice, fuse, decoder): both against the oracle, and each other."""
    import network.wct_rp as wct_mod
    m, c, s, ref = wct_case
    assert wct_mod.FUSED_WCT
    fused = m.test(c.to(cuda), s.to(cuda))
    with unfused(wct_mod, "FUSED_WCT"):
        plain = m.test(c.to(cuda), s.to(cuda))
    m.check()
    assert fused.shape == ref.shape
    print(f"WCTRPNet.test: fused {rel_l2(fused, ref):.3e}, op by op {rel_l2(plain, ref):.3e}, "
          f"between {rel_l2(fused, plain):.3e}")
    assert rel_l2(fused, ref) < TOL_NET and rel_l2(plain, ref) < TOL_NET
    assert rel_l2(fused, plain) < 1e-5
    # fuse() on features of two sizes
    cf, sf = gen(11, (2, 16, 12, 20), 2.0, 0.3, relu=True), gen(12, (2, 16, 9, 8), 1.5, 0.5, relu=True)
    assert rel_l2(m.fuse(cf.to(cuda), sf.to(cuda)), R.wct_fuse(cf, sf)) < TOL_WCT
    m.check()


def test_wct_rp_batch_independence(cuda, wct_case):
    import network.wct_rp as wct_mod
    m, c, s, _ = wct_case
    for fused in (True, False):
        with contextlib.nullcontext() if fused else unfused(wct_mod, "FUSED_WCT"):
            both = m.test(c.to(cuda), s.to(cuda))
            solo = m.test(c[1:].to(cuda), s[1:].to(cuda))
        assert torch.equal(both[1], solo[0]), fused
    m.check()


def test_models_vs_reference_golden(cuda, golden):
    """The same two models against the reference's own outputs (tests/golden/style_size.npz,
    gen_golden_style_size.py), at the same bars."""
    import network as net
    from helpers import t
    g = golden("style_size")
    m = net.SAModel({}, copy.deepcopy(net.vgg), 0, 64)
    assert (synth_(m, int(g["sa_seed"])) == g["sa_checksum"]).all()
    out = m.to(cuda).test(t(g["sa_content"]).to(cuda), t(g["sa_style"]).to(cuda))
    assert rel_l2(out, g["sa_out"]) < TOL_NET and max_abs_ratio(out, g["sa_out"]) < TOL_NET_MAXABS
    w = net.WCTRPNet(rp_config(int(g["wct_hidden"]), int(g["wct_blocks"])), copy.deepcopy(net.vgg))
    assert (synth_(w, int(g["wct_seed"])) == g["wct_checksum"]).all()
    out = w.to(cuda).test(t(g["wct_content"]).to(cuda), t(g["wct_style"]).to(cuda))
    w.check()
    assert rel_l2(out, g["wct_out"]) < TOL_NET


# ---- what still refuses --------------------------------------------------------------------
def test_mismatched_batch_or_channels_raise(cuda):
    from rpst import ops
    F = gen(1, (2, 64, 4, 5)).to(cuda)
    for bad in ((3, 64, 6, 6), (2, 32, 6, 6)):
        G = gen(2, bad).to(cuda)
        with pytest.raises(ValueError, match=r"\(2, 64, 4, 5\).*" + str(bad).replace("(", r"\(").replace(")", r"\)")):
            ops.sanet_attention(F, G, G)
        with pytest.raises(ValueError, match=r"\(2, 64, 4, 5\)"):
            ops.wct_fuse(F, G)
        with pytest.raises(ValueError, match=r"\(2, 64, 4, 5\)"):
            ops.wct_params(F, G)
    with pytest.raises(ValueError, match="one shape"):
        ops.sanet_attention(F, gen(2, (2, 64, 6, 6)).to(cuda), gen(3, (2, 64, 6, 7)).to(cuda))


def test_square_only_paths_still_refuse(cuda):
    """AdaptiveSANet (f_psi's width is tied to img_size), adaptive_instance_normalization
    (base.py:411), whiten_and_color's fp64 matrices and the training steps stay equal-size."""
    import network as net
    from rpst import autograd, ops
    c = gen(1, (2, 64, 4, 4), 1.0, 0.2, relu=True).to(cuda)
    s = gen(2, (2, 64, 4, 5), 1.0, 0.2, relu=True).to(cuda)
    mod = net.AEAModule(16).to(cuda)
    with torch.no_grad(), pytest.raises(AssertionError):
        ops.adaptive_attention(c, s, s, c, s, mod.f_psi, mod.mode, 50.0, 0.4, 0.5)
    ada = net.AdaptiveSANet(64, 16).to(cuda)
    with torch.no_grad(), pytest.raises(AssertionError):
        ada(c, s)
    with pytest.raises(AssertionError):
        ops.adaptive_instance_normalization(c, s)
    w = net.WCTRPNet(rp_config(4, 3), copy.deepcopy(net.vgg)).to(cuda)
    with pytest.raises(ValueError, match=r"\(8, 40\).*\(8, 30\)"):
        w.whiten_and_color(torch.zeros(8, 40, dtype=torch.float64, device=cuda),
                           torch.zeros(8, 30, dtype=torch.float64, device=cuda))
    ic, is_ = torch.zeros(1, 3, 32, 32, device=cuda), torch.zeros(1, 3, 32, 48, device=cuda)
    with pytest.raises(ValueError, match="one shape"):
        autograd.wct_rp_losses(w, ic, is_)
    sa = net.SAModel({}, copy.deepcopy(net.vgg), 0, 32).to(cuda)
    with pytest.raises(ValueError, match="one shape"):
        autograd.samodel_losses(sa, ic, is_)
