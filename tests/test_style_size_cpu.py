"""A style of another size than the content: the argument checks that need no GPU (the C
entries refuse before any launch, the ops refuse CPU tensors and wrong shape combinations)
and the conditioning of the GPU tests' WCT inputs."""
import ctypes

import pytest
import torch

from oracle import restate as R


def _lib_and_err():
    from rpst import _lib
    lib = _lib.load()
    return lib, (lambda: lib.rpst_last_error().decode())


def test_attention_qk_argument_errors():
    """rpst_sanet_attention_qk: RPST_EINVAL for a null pointer or a count < 1, RPST_EWORKSPACE
    (include/rpst.h: the code of every entry for it) for a short workspace on the materialised
    path, all before any launch."""
    from rpst import _lib
    lib, err = _lib_and_err()
    EINVAL, EWORKSPACE = _lib.constants("EINVAL", "EWORKSPACE")

    def attn(F=1, G=1, H=1, O=1, B=2, C=40, q=36, k=35, ws=1, nbytes=1 << 30):
        return lib.rpst_sanet_attention_qk(F, G, H, O, B, C, q, k, ws, nbytes, None)

    assert attn(G=None) == EINVAL and "null pointer" in err()
    assert attn(q=0) == EINVAL and "bad shape" in err() and "HW=0/35" in err()
    assert attn(k=0) == EINVAL and "bad shape" in err() and "HW=36/0" in err()
    assert attn(k=-4) == EINVAL and attn(B=0) == EINVAL and attn(C=0) == EINVAL
    need = lib.rpst_sanet_attention_qk_workspace_size_c(2, 40, 36, 35)
    assert need == 4 * (2 * 36 * 35 + 2 * 2 * 36)
    assert attn(nbytes=need - 1) == EWORKSPACE and "workspace" in err()
    assert attn(ws=None) == EWORKSPACE and "workspace" in err()
    # C = 64 with 35 keys is materialised too (16-byte key rows); 36 keys with any query count
    # is flash and asks for nothing
    assert attn(C=64, nbytes=16) == EWORKSPACE
    assert lib.rpst_sanet_attention_qk_workspace_size_c(2, 64, 35, 36) == 0
    assert lib.rpst_sanet_attention_qk_workspace_size_c(2, 64, 36, 35) > 0
    assert lib.rpst_sanet_attention_qk_workspace_size_c(2, 64, 0, 36) == 0
    # the one-count queries are the HWq = HWk ones
    for C, hw in ((64, 36), (40, 36), (64, 35)):
        assert lib.rpst_sanet_attention_workspace_size_c(3, C, hw) == \
            lib.rpst_sanet_attention_qk_workspace_size_c(3, C, hw, hw)


def test_wct_cs_argument_errors():
    """The two-count WCT entries: a count < 2 on either side is RPST_EINVAL naming both, a
    short workspace RPST_EWORKSPACE; the one-count sizes are the HWc = HWs ones."""
    from rpst import _lib
    lib, err = _lib_and_err()
    EINVAL, EWORKSPACE = _lib.constants("EINVAL", "EWORKSPACE")
    need = lib.rpst_wct_workspace_size_cs(2, 16, 240, 72)
    assert need > 0 and lib.rpst_wct_workspace_size_cs(2, 16, 240, 1) == 0
    for n, C, hw in ((2, 16, 240), (1, 256, 4096), (3, 512, 100)):
        assert lib.rpst_wct_workspace_size(n, C, hw) == lib.rpst_wct_workspace_size_cs(n, C, hw, hw)

    def fuse(c=1, s=1, out=1, n=2, C=16, hwc=240, hws=72, ws=1, nbytes=need):
        return lib.rpst_wct_fuse_cs(c, s, out, n, C, hwc, hws, None, ws, nbytes, None)

    def params(c=1, s=1, T=1, off=1, n=2, C=16, hwc=240, hws=72, ws=1, nbytes=need):
        return lib.rpst_wct_params_cs(c, s, None, T, off, n, C, hwc, hws, None, ws, nbytes, None)

    for f in (fuse, params):
        assert f(s=None) == EINVAL and "null pointer" in err()
        assert f(hws=1) == EINVAL and "HW=240/1" in err()
        assert f(hwc=0) == EINVAL and "HW=0/72" in err()
        assert f(nbytes=need - 1) == EWORKSPACE and "workspace" in err()
        assert f(ws=None) == EWORKSPACE
    buf = (ctypes.c_int * 2)()
    assert lib.rpst_wct_status_cs(1, 2, 16, 240, 1, ctypes.addressof(buf), None) == EINVAL
    assert lib.rpst_wct_status_cs(None, 2, 16, 240, 72, ctypes.addressof(buf), None) == EINVAL


def test_ops_refuse_cpu_tensors_and_wrong_shapes():
    from rpst import ops
    F, G = torch.zeros(2, 64, 4, 5), torch.zeros(2, 64, 6, 6)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.sanet_attention(F, G, G)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.wct_fuse(F, G)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.wct_params(F, G)
    for bad in (torch.zeros(3, 64, 6, 6), torch.zeros(2, 32, 6, 6), torch.zeros(2, 64, 36)):
        for call in (lambda: ops.sanet_attention(F, bad, bad), lambda: ops.wct_fuse(F, bad),
                     lambda: ops.wct_params(F, bad)):
            with pytest.raises(ValueError) as e:
                call()
            assert str(tuple(F.shape)) in str(e.value) and str(tuple(bad.shape)) in str(e.value)


def test_training_steps_and_fp64_matrices_refuse_before_any_kernel():
    import copy

    import network as net
    from helpers import rp_config
    from rpst import autograd
    c, s = torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 48)
    w = net.WCTRPNet(rp_config(4, 3), copy.deepcopy(net.vgg))
    with pytest.raises(ValueError, match="one shape"):
        autograd.wct_rp_losses(w, c, s)
    with pytest.raises(ValueError, match="one shape"):
        w(c, s)  # forward() with autograd on routes to the training step
    sa = net.SAModel({}, copy.deepcopy(net.vgg), 0, 32)
    with pytest.raises(ValueError, match="one shape"):
        autograd.samodel_losses(sa, c, s)
    with pytest.raises(ValueError, match=r"\(8, 40\).*\(8, 30\)"):
        w.whiten_and_color(torch.zeros(8, 40, dtype=torch.float64),
                           torch.zeros(8, 30, dtype=torch.float64))


def test_wct_cases_are_conditioned():
    """The GPU tests' WCT inputs: the oracle's eigenvalues of Cc + 1e-4 I, Cs + 1e-4 I and of
    Mid's argument stay far above its 1e-5 truncation (smallest: 1.075e-1, the 72-pixel style
    at C = 16), so the comparison is not about which side of the truncation a value falls."""
    from test_gpu_style_size import WCT_CASES, _wct_inputs
    for case in WCT_CASES:
        C, hc, hs = case.values
        assert hc[0] * hc[1] >= 4 * C and hs[0] * hs[1] >= 4 * C
        for cf, sf in zip(*_wct_inputs(C, hc, hs)):
            cF, sF = cf.reshape(C, -1).double(), sf.reshape(C, -1).double()
            cF, sF = cF - cF.mean(1, keepdim=True), sF - sF.mean(1, keepdim=True)
            eye = torch.eye(C, dtype=torch.float64)
            cc = cF @ cF.t() / (cF.shape[1] - 1) + eye
            cs = sF @ sF.t() / (sF.shape[1] - 1)
            sc = R.matrix_sqrt(cc)
            mid = sc @ cs @ sc + 1e-4 * eye
            for m in (cc + 1e-4 * eye, cs + 1e-4 * eye, (mid + mid.t()) / 2):
                assert float(torch.linalg.eigvalsh(m).min()) > 1e-2


def test_oracle_matches_reference_golden(golden):
    """The oracle restatement against the reference's own different-size outputs
    (tests/golden/style_size.npz): the GPU tests' other yardstick is the reference's."""
    from helpers import TOL_NET, rel_l2, t
    from rpst import synth
    import copy

    import network as net
    g = golden("style_size")
    w = net.WCTRPNet({"rp_blocks": int(g["wct_blocks"]), "hidden_dim": int(g["wct_hidden"]),
                      "resume": False}, copy.deepcopy(net.vgg))
    synth.synth_module_(w, int(g["wct_seed"]))
    sd = {k: v.detach() for k, v in w.state_dict().items()}
    assert (synth.checksum({k: v.numpy() for k, v in sd.items()}) == g["wct_checksum"]).all()
    ref = R.wct_rp_test(t(g["wct_content"]), t(g["wct_style"]), sd, int(g["wct_blocks"]))
    assert ref.shape == g["wct_out"].shape and rel_l2(ref, g["wct_out"]) < TOL_NET
