"""GPU parity for the AdaptiveSANet family (network/sanet.py:12-18,
26-71, 100-160, 278-345) through the C ABI: the cosine affinity GEMM, the AEA clamp MLP
(GEMM with a LeakyReLU epilogue + head kernel), the clamped attention formed while S is
staged into the second GEMM, and the AdaptiveSAModel end to end — against goldens produced
by the reference and against the CPU oracle / float64 restatements at larger sizes.

Tolerances: kernels and modules rel-L2 <= 1e-5; networks rel-L2 <= 1e-4 and max-abs <=
5e-4*max|ref| (tests/helpers.py). The AEA clamp (sigmoid slope 50 on a peaked softmax)
is ill-conditioned end to end: with synthetic weights the reference's own fp32 output is
1.8e-4 (rel-L2) away from the same model in float64 (AdaptiveSAModel 'aea' at 64x64).
Network tests therefore compare against the float64 oracle with the tolerance
max(TOL_NET, 3 x the fp32 reference's own distance to it) — `_cond_tol`."""
import copy

import pytest
import torch
import torch.nn.functional as Fn

from helpers import (TOL_NET, TOL_NET_MAXABS, flat_or_live, gen, max_abs_ratio, rel_l2,
                     state_dict_of, synth_, t)
from oracle import restate as R

pytestmark = pytest.mark.gpu
MODES = ("aea", "relu")


def test_affinity_golden(cuda, golden):
    import network as net
    g = golden("adaptive")
    out = net.cal_affinity_matrix(t(g["aff_c"]).to(cuda), t(g["aff_s"]).to(cuda))
    assert rel_l2(out, g["aff_out"]) < 1e-6


@pytest.mark.parametrize("shape", [(1, 512, 64, 64), (2, 512, 32, 32), (3, 20, 7, 9)])
def test_affinity_vs_fp64(cuda, shape):
    from rpst import ops
    c = gen(1, shape, 2.0, 0.3, relu=True)
    s = gen(2, shape, 2.0, 0.3, relu=True)
    ref = R.cal_affinity_matrix(c.double(), s.double())
    assert rel_l2(ops.cosine_affinity(c.to(cuda), s.to(cuda)), ref) < 1e-6


@pytest.mark.parametrize("mode", MODES)
def test_aea_modules_golden(cuda, golden, mode):
    import network as net
    g = golden("adaptive")
    mod = (net.AEAModule if mode == "aea" else net.AEALReluModule)(48)
    synth_(mod, 90 if mode == "aea" else 91)
    with torch.no_grad():
        y, cl = mod.to(cuda)(t(g["aff_out"]).to(cuda), t(g[f"aea_{mode}_fx"]).to(cuda))
    assert rel_l2(cl, g[f"aea_{mode}_clamp"]) < 1e-6
    assert rel_l2(y, g[f"aea_{mode}_out"]) < 1e-5


@pytest.mark.parametrize("mode", MODES)
def test_adaptive_sanet_golden(cuda, golden, mode):
    import network as net
    g = golden("adaptive")
    for i in range(2):
        c = t(g[f"asa_{mode}_c{i}"])
        mod = net.AdaptiveSANet(c.shape[1], c.shape[2] * c.shape[3], mode)
        synth_(mod, int(g[f"asa_{mode}_seed{i}"]))
        mod = mod.to(cuda)
        with torch.no_grad():
            out = mod(c.to(cuda), t(g[f"asa_{mode}_s{i}"]).to(cuda))
        assert rel_l2(out, g[f"asa_{mode}_out{i}"]) < 1e-5, (mode, i)
        assert rel_l2(mod.claim_value, g[f"asa_{mode}_claim{i}"]) < 1e-6


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hw2", [(12, 16), (9, 20)])
def test_adaptive_attention_peaked(cuda, mode, hw2):
    """Logits in the hundreds: the softmax is peaked, so P crosses the clamp and both AEA
    branches (sigmoid slope 50, relu + second softmax) carry weight. float64 reference.
    C = 64 runs the two-pass flash kernels (no S); HW = 180 leaves a ragged last key block
    (keys past HW weigh nothing). Without keep_claims the output is the same bits."""
    import network as net
    from rpst import ops
    B, C = 2, 64
    h, w = hw2
    hw = h * w
    mod = net.AEAModule(hw) if mode == "aea" else net.AEALReluModule(hw)
    synth_(mod, 7)
    sd = {k: v.double() for k, v in state_dict_of(mod).items()}
    F = gen(5, (B, C, h, w), 3.0)
    G = gen(6, (B, C, h, w), 3.0)
    H = gen(7, (B, C, h, w), 1.0)
    c = gen(8, (B, C, h, w), 1.0, 0.2, relu=True)
    s = gen(9, (B, C, h, w), 1.0, 0.2, relu=True)
    S = torch.bmm(F.view(B, C, -1).permute(0, 2, 1).double(), G.view(B, C, -1).double())
    assert S.abs().max() > 100
    P = torch.softmax(S, -1)
    Q, clamp = R.aea(R.cal_affinity_matrix(c.double(), s.double()), P, sd, "", mode)
    if mode == "aea":
        assert (Q > 0.5).any()  # the sigmoid branch is exercised
    ref = torch.bmm(H.view(B, C, -1).double(), Q.permute(0, 2, 1)).view(B, C, h, w)
    mod = mod.to(cuda)
    with torch.no_grad():
        out, cl, before, after = ops.adaptive_attention(
            F.to(cuda), G.to(cuda), H.to(cuda), c.to(cuda), s.to(cuda), mod.f_psi, mod.mode,
            50.0, 0.4, 0.5, keep_claims=True)
    assert rel_l2(cl, clamp) < 1e-6
    assert rel_l2(before, P) < 1e-5
    assert rel_l2(after, Q) < 1e-5
    assert rel_l2(out, ref) < 1e-5
    with torch.no_grad():
        out2, cl2, b2, a2 = ops.adaptive_attention(
            F.to(cuda), G.to(cuda), H.to(cuda), c.to(cuda), s.to(cuda), mod.f_psi, mod.mode,
            50.0, 0.4, 0.5, keep_claims=False)
    assert b2 is None and a2 is None
    assert torch.equal(out2, out) and torch.equal(cl2, cl)


@pytest.mark.parametrize("mode", MODES)
def test_adaptive_attention_relu4_1_at_1024(cuda, mode):
    """AdaptiveSANet at relu4_1 of a 1024x1024 image (C = 512, HW =
    128 x 128 = 16384) on the two-pass flash path: the workspace holds no B x HW x HW term (S
    alone would be 1 GiB per image) and the output matches a float64 reference formed in
    query chunks on the GPU (torch, S of 2048 queries at a time)."""
    import network as net
    from rpst import _lib, ops
    B, C, h, w = 1, 512, 128, 128
    hw = h * w
    mod = net.AEAModule(hw) if mode == "aea" else net.AEALReluModule(hw)
    synth_(mod, 31)
    hid = mod.f_psi[0].out_features
    nbytes = _lib.load().rpst_adaptive_attention_workspace_size(B, C, hw, hid)
    # T = sn W1^T (+ its 4 K-chunk partials), Z = cn^T T (f_psi's hidden layer: HW x HW/16
    # by the reference's design), the normalised features and 7 per-query vectors -- no
    # B x HW x HW term (S: 1 GiB)
    assert nbytes == 4 * (5 * B * C * hid + B * hw * hid + 2 * B * C * hw + 7 * B * hw), nbytes
    g = torch.Generator(device=cuda).manual_seed(5)
    F, G, H = ((torch.rand((B, C, h, w), device=cuda, generator=g) * 2 - 1) * sc
               for sc in (0.3, 0.3, 1.0))
    c, s = (torch.rand((B, C, h, w), device=cuda, generator=g) for _ in range(2))
    mod = mod.to(cuda)
    with torch.no_grad():
        out, cl, _, _ = ops.adaptive_attention(F, G, H, c, s, mod.f_psi, mod.mode, 50.0, 0.4,
                                               0.5)
    sd = {k: v.double().to(cuda) for k, v in state_dict_of(mod).items()}
    F64, G64, H64 = (x.double().view(B, C, hw) for x in (F, G, H))
    cn = torch.nn.functional.normalize(c.double().view(B, C, hw), dim=1)
    sn = torch.nn.functional.normalize(s.double().view(B, C, hw), dim=1)
    ref = torch.empty((B, C, hw), dtype=torch.float64, device=cuda)
    ref_cl = torch.empty((B, hw, 1), dtype=torch.float64, device=cuda)
    for q0 in range(0, hw, 2048):
        qs = slice(q0, q0 + 2048)
        P = torch.softmax(torch.bmm(F64[:, :, qs].transpose(1, 2), G64), -1)
        A = torch.bmm(cn[:, :, qs].transpose(1, 2), sn)
        Q, clamp = R.aea(A, P, sd, "", mode)
        ref[:, :, qs] = torch.bmm(H64, Q.transpose(1, 2))
        ref_cl[:, qs] = clamp.view(B, -1, 1)
    assert rel_l2(cl, ref_cl) < 1e-6
    assert rel_l2(out, ref.view(B, C, h, w)) < 1e-5


@pytest.mark.parametrize("mode,shape,inputs", flat_or_live(
    [(f"shape{i}-{mode}", (mode, shape)) for mode in MODES
     for i, shape in enumerate([(2, 512, 32, 32), (2, 48, 8, 10)])]))
def test_factored_clamp_production_shape(cuda, mode, shape, inputs):
    """The factored AEA clamp (Z = cn^T (sn W1^T), dW1 = (cn du)^T sn: the B x HW x HW
    affinity never formed) at a production shape (C = 512, HW = 1024, hid = 64) and at a
    ragged hidden width (HW = 80 -> hid = 5), forward clamp and backward dW1 / db1 / dW2 / db2
    against the float64 two-GEMM form (affinity formed, torch autograd).
    flat: F and G uniform x 0.2, so P ~ 1 / HW and the clamp is dead: 'aea' has Q < 1e-13 and
    f_psi gradients of norm ~1e-12 (held to 1e-4); with 'relu' no entry of P passes its clamp
    and dF, dG and the f_psi gradients are exactly zero on both sides, asserted as such.
    live: F and G from helpers.peaked_attention_inputs (helpers.aea_live_case), the four f_psi
    gradients and dF, dG, dH under the conditions and bars of helpers.aea_live_bars."""
    import network as net
    from rpst import ops
    from helpers import (aea_attention_grads, aea_backward_abi, aea_live_case, check_aea_grads,
                         clamp_liveness)
    B, C, h, w = shape
    what = f"factored clamp {mode} {shape} {inputs}"
    if inputs == "live":
        case = aea_live_case(mode, shape)
        mod, clamp, O, g64 = copy.deepcopy(case.mod), case.clamp, case.out, case.g64
        host = (case.F, case.G, case.H, case.c, case.s, case.dO)
    else:
        mod = net.AEAModule(h * w) if mode == "aea" else net.AEALReluModule(h * w)
        synth_(mod, 11)
        host = (gen(21, shape, 0.2), gen(22, shape, 0.2), gen(23, shape, 1.0),
                gen(24, shape, 1.0, 0.2, relu=True), gen(25, shape, 1.0, 0.2, relu=True),
                gen(26, shape, 1.0))
        O, clamp, P, Q, g64 = aea_attention_grads(*host, state_dict_of(mod), mode, torch.float64)
        assert clamp_liveness(P, clamp, mode) == 0.0
    assert mod.f_psi[0].out_features == h * w // 16
    mod = mod.to(cuda)
    args = [x.to(cuda) for x in host]
    with torch.no_grad():
        out, cl, _, _ = ops.adaptive_attention(*args[:5], mod.f_psi, mod.mode, 50.0, 0.4, 0.5,
                                               keep_claims=True)
    assert rel_l2(cl, clamp) < 1e-6, rel_l2(cl, clamp)
    assert rel_l2(out, O) < 1e-5
    got, _ = aea_backward_abi(mod, *args)
    if inputs == "live":
        check_aea_grads(got, g64, case.bars, what)
        return
    fpsi = [k for k in g64 if k.startswith("f_psi")]
    if mode == "relu":  # relu never active: zero on both sides, exactly
        for k in ["dF", "dG"] + fpsi:
            assert not g64[k].any() and not got[k].any(), k
    else:
        assert Q.max() < 1e-13
        check_aea_grads(got, {k: g64[k] for k in fpsi}, dict.fromkeys(fpsi, 1e-4), what)


@pytest.mark.parametrize("mode", MODES)
def test_adaptive_transform_golden(cuda, golden, mode):
    import network as net
    g = golden("adaptive")
    tr = net.AdaptiveTransform(32, 64, 16, mode)
    synth_(tr, 98 + (mode == "relu"))
    with torch.no_grad():
        out = tr.to(cuda)(*(t(g[f"atr_{mode}_{k}"]).to(cuda) for k in ("c4", "s4", "c5", "s5")))
    assert rel_l2(out, g[f"atr_{mode}_out"]) < 1e-5


def _cond_tol(ref32, ref64):
    """Network tolerance against the float64 oracle: the fp32 reference's own error there
    (the problem's conditioning) x 5, at least TOL_NET. The factor: the VGG convs run as
    Winograd F(4x4,3x3), whose fp32 rounding is ~2.8x the direct convolution's per layer
    (1.1e-6 vs 4e-7 rel-L2, tests/test_gpu_fullsize.py); measured 3.5x on the 'aea' model
    (sigmoid slope 50 on a peaked softmax), 2.4x with F(2x2)."""
    return max(TOL_NET, 5.0 * rel_l2(ref32, ref64))


@pytest.mark.parametrize("mode", MODES)
def test_adaptive_samodel_golden(cuda, golden, mode):
    import network as net
    g = golden("adaptive")
    m = net.AdaptiveSAModel({"ada_module": mode}, copy.deepcopy(net.vgg), 0, 64)
    synth_(m, int(g[f"model_{mode}_seed"]))
    sd64 = {k: v.double() for k, v in state_dict_of(m).items()}
    c, s = t(g[f"model_{mode}_content"]), t(g[f"model_{mode}_style"])
    out = m.to(cuda).test(c.to(cuda), s.to(cuda))
    ref = g[f"model_{mode}_out"]
    ref64 = R.adaptive_samodel_test(c.double(), s.double(), sd64, mode)
    tol = _cond_tol(ref, ref64)
    assert rel_l2(out, ref64) < tol, (rel_l2(out, ref64), tol)
    if mode == "relu":  # well conditioned: the plain network bar against the reference
        assert rel_l2(out, ref) < TOL_NET, rel_l2(out, ref)
        assert max_abs_ratio(out, ref) < TOL_NET_MAXABS


@pytest.mark.parametrize("mode,size,batch", [("relu", 256, 2), ("aea", 128, 3)])
def test_adaptive_samodel_vs_oracle(cuda, mode, size, batch):
    import network as net
    from rpst import synth
    m = net.AdaptiveSAModel({"ada_module": mode}, copy.deepcopy(net.vgg), 0, size)
    synth_(m, 11)
    sd = state_dict_of(m)
    c = torch.from_numpy(synth.image(21, (batch, 3, size, size)))
    s = torch.from_numpy(synth.image(22, (batch, 3, size, size)))
    ref = R.adaptive_samodel_test(c, s, sd, mode)
    ref64 = R.adaptive_samodel_test(c.double(), s.double(),
                                    {k: v.double() for k, v in sd.items()}, mode)
    out = m.to(cuda).test(c.to(cuda), s.to(cuda))
    tol = _cond_tol(ref, ref64)
    assert rel_l2(out, ref64) < tol, (rel_l2(out, ref64), tol)
    # claim values of the last call are kept like the reference's attribute
    assert m.transform.sanet5_1.claim_value.shape == (batch, (size // 16) ** 2, 1)


def test_adaptive_requires_matching_spatial_dims(cuda):
    import network as net
    mod = net.AdaptiveSANet(16, 64, "relu").to(cuda)
    x = torch.rand(1, 16, 4, 4, device=cuda)
    with torch.no_grad(), pytest.raises(AssertionError):
        mod(x, x)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C,hw2,scale", [(512, (16, 16), 1.0), (64, (12, 16), 3.0)])
def test_adaptive_forward_matches_backward_statistics(cuda, mode, C, hw2, scale):
    """the training forward runs the two flash passes (P normalised by row
    statistics summed in the flash kernel's key order), while rpst_adaptive_attention_backward
    recomputes S and its row statistics with gemm_f32_kernel + rowstats_kernel -- the form the
    keep_claims maps are made with. The output implied by that form, H Q_gemm^T, agrees with
    the flash output to within 3x the flash output's own fp32 distance to float64, so the
    gradients are taken at the point the forward reported (bound: max(3 e, 1e-6))."""
    import network as net
    from rpst import ops
    B = 2
    h, w = hw2
    hw = h * w
    mod = net.AEAModule(hw) if mode == "aea" else net.AEALReluModule(hw)
    synth_(mod, 17)
    sd = {k: v.double() for k, v in state_dict_of(mod).items()}
    F = gen(15, (B, C, h, w), scale)
    G = gen(16, (B, C, h, w), scale)
    H = gen(17, (B, C, h, w), 1.0)
    c = gen(18, (B, C, h, w), 1.0, 0.2, relu=True)
    s = gen(19, (B, C, h, w), 1.0, 0.2, relu=True)
    S = torch.bmm(F.view(B, C, -1).permute(0, 2, 1).double(), G.view(B, C, -1).double())
    Q, _ = R.aea(R.cal_affinity_matrix(c.double(), s.double()), torch.softmax(S, -1), sd, "",
                 mode)
    ref64 = torch.bmm(H.view(B, C, -1).double(), Q.permute(0, 2, 1)).view(B, C, h, w)
    mod = mod.to(cuda)
    with torch.no_grad():
        out, _, _, after = ops.adaptive_attention(
            F.to(cuda), G.to(cuda), H.to(cuda), c.to(cuda), s.to(cuda), mod.f_psi, mod.mode,
            50.0, 0.4, 0.5, keep_claims=True)
    implied = torch.bmm(H.view(B, C, -1).double().to(cuda),
                        after.double().permute(0, 2, 1)).view(B, C, h, w)
    e = rel_l2(out, ref64)
    mismatch = rel_l2(out, implied)
    assert e < 1e-5, e
    assert mismatch <= max(3 * e, 1e-6), (mismatch, e)
