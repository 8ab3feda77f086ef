"""SE channel attention (`attention: se`), the parts that need no GPU: the float64
restatement (tests/se_ref.py) against the reference's recorded outputs, the mirror's
state_dict keys, the synthetic-weight rules of the attention blocks, and what keeps raising."""
import copy

import numpy as np
import pytest
import torch

import se_ref as S
from helpers import golden_net, multiscale_config, rel_l2


def _module(g, i):
    import network as net
    C = g[f"mod{i}_x"].shape[1]
    blk = net.SEBottleneck(C, C)
    ck = S.synth_block_(blk, int(g[f"mod{i}_seed"]))
    return blk.eval(), ck


def test_restatement_matches_reference_modules(golden):
    """se_ref.se_block, and its folded form (BatchNorm in the conv weights, the gate from the
    pooled h2), against the reference's fp32 outputs: the reference's own fp32 floor is
    1.3-1.8e-7 (mod*_floor), the bar 1e-6."""
    g = golden("se")
    for i in range(int(g["n_mod"])):
        blk, ck = _module(g, i)
        assert np.array_equal(ck, g[f"mod{i}_checksum"]), i
        assert float(g[f"mod{i}_floor"]) < 1e-6
        sd = blk.state_dict()
        for fn in (S.se_block, S.se_block_folded):
            out, gate = fn(g[f"mod{i}_x"], sd)
            assert rel_l2(out, g[f"mod{i}_out"]) < 1e-6, (i, fn.__name__)
            assert rel_l2(gate, g[f"mod{i}_gate"]) < 1e-6, (i, fn.__name__)
        a, b = S.se_block(g[f"mod{i}_x"], sd), S.se_block_folded(g[f"mod{i}_x"], sd)
        assert rel_l2(a[0], b[0]) < 1e-12 and rel_l2(a[1], b[1]) < 1e-12


def test_golden_gates_discriminate(golden):
    """A kernel that ignored the gate, or used one image's for the whole batch, could not pass:
    the recorded gates span (< 0.3, > 0.7) and differ by > 0.1 between the two images."""
    g = golden("se")
    for i in range(int(g["n_mod"])):
        gate = g[f"mod{i}_gate"].reshape(g[f"mod{i}_gate"].shape[0], -1)
        assert gate.min() < 0.3 and gate.max() > 0.7, i
        if gate.shape[0] > 1:
            assert np.abs(gate[0] - gate[1]).max() > 0.1


def test_fold_rounds_once(golden):
    """rpst.plan.fold_batchnorm: the float64 fold of se_ref, rounded once to fp32."""
    from rpst import plan
    g = golden("se")
    blk, _ = _module(g, 0)
    sd = blk.state_dict()
    for conv, bn, name in ((blk.conv1, blk.bn1, "1"), (blk.conv2, blk.bn2, "2"),
                           (blk.conv3, blk.bn3, "3")):
        w64, b64 = S.fold(sd[f"conv{name}.weight"], sd, "bn" + name)
        w, b = plan.fold_batchnorm(conv, bn)
        assert w.dtype == torch.float32 and torch.equal(w, w64.float())
        assert b.dtype == torch.float32 and torch.equal(b, b64.float())


def _keys(sd):
    names, shapes = S.key_table(sd)
    return list(names), shapes.tolist()


def test_state_dict_keys_match_reference(golden):
    import network as net
    g = golden("se")
    for i in range(int(g["n_mod"])):
        blk, _ = _module(g, i)
        assert _keys(blk.state_dict()) == (list(g[f"mod{i}_keys"]), g[f"mod{i}_shapes"].tolist())
    for i in range(int(g["n_net"])):
        m = golden_net(net.MultiScaleAdaINRPNet, S.golden_config(g, i), g, f"net{i}_")
        names, shapes = _keys(m.state_dict())
        assert names == list(g[f"net{i}_keys"]) and shapes == g[f"net{i}_shapes"].tolist()
        assert "rp_shared_encoder.0.attention_block.se.fc.2.weight" in names
        assert "rp_shared_encoder.0.attention_block.bn3.num_batches_tracked" in names
        assert not any("rp_decoder" in k and "attention_block" in k for k in names)


def test_synth_rules_for_attention_keys():
    import network as net
    from rpst import synth
    m = net.MultiScaleAdaINRPNet(dict(multiscale_config(32, 3, 0), attention="se"),
                                 copy.deepcopy(net.vgg))
    synth.synth_module_(m, 3)
    sd = m.state_dict()
    pre = "rp_shared_encoder.1.attention_block."
    for bn in ("bn1", "bn2", "bn3"):
        v = sd[pre + bn + ".running_var"]
        assert float(v.min()) >= 0.5 and float(v.max()) < 1.5
        w = sd[pre + bn + ".weight"]
        assert float(w.min()) >= 0.5 and float(w.max()) < 1.5
        assert float(sd[pre + bn + ".bias"].abs().max()) <= 0.125
        assert float(sd[pre + bn + ".running_mean"].abs().max()) <= 0.5
        nb = sd[pre + bn + ".num_batches_tracked"]
        assert nb.dtype == torch.int64 and int(nb) == 0
    fa, fb = sd[pre + "se.fc.0.weight"], sd[pre + "se.fc.2.weight"]
    assert tuple(fa.shape) == (2, 32) and tuple(fb.shape) == (32, 2)
    assert 0.5 / 32 ** 0.5 < float(fa.abs().max()) <= 1 / 32 ** 0.5
    assert 0.5 / 2 ** 0.5 < float(fb.abs().max()) <= 1 / 2 ** 0.5
    # conv weights of the block keep the He-uniform rule, and every key outside an attention
    # block is what it was
    k = pre + "conv2.weight"
    assert np.array_equal(sd[k].numpy(), synth.conv_param(3, k, tuple(sd[k].shape)))
    for k, v in sd.items():
        if ".attention_block." not in k:
            assert np.array_equal(v.numpy(), synth.conv_param(3, k, tuple(v.shape))), k


def test_synth_unchanged_without_attention_keys():
    """A module without '.attention_block.' keys gets synth.conv_param's values bit for bit
    (AdaptiveSAModel's 2-D f_psi weight included: the 2-D rule is for attention keys only)."""
    import network as net
    from rpst import synth
    am = net.AdaptiveSAModel({"ada_module": "relu"}, copy.deepcopy(net.vgg), 0, 64)
    synth.synth_module_(am, 11)
    sd = am.state_dict()
    assert any(v.dim() == 2 for v in sd.values())
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), synth.conv_param(11, k, tuple(v.shape))), k


def test_unsupported_attention_raises():
    import network as net
    with pytest.raises(NotImplementedError, match="sk"):
        net.Conv2dBlock(32, 32, 3, 1, padding=1, attention="sk")
    with pytest.raises(NotImplementedError, match="output_dim 8 < 16"):
        net.Conv2dBlock(3, 8, 3, 1, padding=1, attention="se")
    with pytest.raises(NotImplementedError):
        net.MultiScaleAdaINRPNet(dict(multiscale_config(8, 3, 0), attention="se"),
                                 copy.deepcopy(net.vgg))
    blk = net.Conv2dBlock(3, 16, 3, 1, padding=1, attention="se")
    assert isinstance(blk.attention_block, net.SEBottleneck)
    assert net.Conv2dBlock(3, 16, 3, 1, padding=1).attention_block is None


def test_se_is_inference_only_before_any_launch():
    """Training-mode BatchNorm has no kernel: the module refuses in training mode, and the
    network's forward() refuses before it touches its (CPU) inputs."""
    import network as net
    blk = net.SEBottleneck(16, 16)
    assert blk.training
    with pytest.raises(NotImplementedError, match="training-mode BatchNorm"):
        blk(torch.zeros(1, 16, 4, 4))
    m = net.MultiScaleAdaINRPNet(dict(multiscale_config(16, 3, 0), attention="se"),
                                 copy.deepcopy(net.vgg))
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(NotImplementedError, match="inference only"):
        m(x, x)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="inference only"):
        m(x, x)


def test_se_ops_refuse_cpu_tensors():
    import network as net
    from rpst import ops
    blk = net.SEBottleneck(16, 16).eval()
    x = torch.zeros(1, 16, 4, 4)
    with torch.no_grad():
        for call in (lambda: ops.se_bottleneck(x, blk), lambda: blk(x),
                     lambda: ops.se_gate(torch.zeros(1, 16), torch.zeros(16, 16), torch.zeros(16),
                                         torch.zeros(1, 16), torch.zeros(16, 1)),
                     lambda: ops.conv2d_gated(x, torch.zeros(512), None, torch.zeros(1, 16), x, 16)):
            with pytest.raises(RuntimeError, match="ROCm GPU"):
                call()


def test_gated_abi_argument_errors():
    """rpst_conv2d_gated / rpst_se_gate check their arguments before touching the device."""
    import ctypes
    from rpst import _lib
    lib = _lib.load()
    eps = ctypes.c_float(1e-5)
    st = lib.rpst_conv2d_gated(1, 1, None, 1, 1, 1, 1, 16, 8, 8, 16, 3, None, None, eps, None, 0,
                               None)
    assert st == -1 and "1x1" in lib.rpst_last_error().decode()
    st = lib.rpst_conv2d_gated(1, 1, None, None, 1, 1, 1, 16, 8, 8, 16, 1, None, None, eps, None,
                               0, None)
    assert st == -1 and "null gate" in lib.rpst_last_error().decode()
    st = lib.rpst_conv2d_gated(1, 1, None, 1, 1, 1, 1, 16, 8, 8, 16, 1, 1, None, eps, None, 0,
                               None)
    assert st == -1 and "together" in lib.rpst_last_error().decode()
    # statistics from the epilogue need the partials' workspace (Cout <= 64), none above that
    assert lib.rpst_conv2d_gated_workspace_size(2, 32, 24, 40, 32, 1) == 2 * 32 * (2 * 2 * 4) * 8
    assert lib.rpst_conv2d_gated_workspace_size(2, 128, 24, 40, 128, 1) == 0
    assert lib.rpst_conv2d_gated_workspace_size(2, 32, 24, 40, 32, 3) == 0
    st = lib.rpst_conv2d_gated(1, 1, None, 1, 1, 1, 2, 32, 24, 40, 32, 1, 1, 1, eps, None, 0, None)
    assert st == -3 and "workspace" in lib.rpst_last_error().decode()
    st = lib.rpst_se_gate(1, 1, 1, 1, 1, 1, 2, 32, 0, None)
    assert st == -1 and "R" in lib.rpst_last_error().decode()
    st = lib.rpst_se_gate(1, 1, 1, 1, None, 1, 2, 32, 2, None)
    assert st == -1 and "null pointer" in lib.rpst_last_error().decode()
