"""The live-clamp inputs of the AEA backward tests (helpers.peaked_attention_inputs) tell a
wrong clamp derivative from the right one, and the flat inputs the kernel tests used alone
before could not. float64 on the CPU at (2, 48, 8, 10): the gradients of
O = H aea(A, softmax(F^T G))^T by autograd of the oracle's restatement, beside those of a
deliberately wrong one with the same forward values: the sigmoid's derivative taken as
50 Q (its saturated-tail approximation, the (1 - Q) factor dropped) and the ReLU's mask taken
as all ones."""
import pytest
import torch

from helpers import (AEA_GRADS, aea_attention_grads, aea_live_case, clamp_liveness, gen,
                     peaked_attention_inputs, rel_l2, state_dict_of, synth_)
from oracle import restate as R

SHAPE = (2, 48, 8, 10)
MODES = ("aea", "relu")


class _TailSigmoid(torch.autograd.Function):
    """sigmoid(x) with the derivative Q in place of Q (1 - Q)."""

    @staticmethod
    def forward(ctx, x):
        q = torch.sigmoid(x)
        ctx.save_for_backward(q)
        return q

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0]


class _OpenRelu(torch.autograd.Function):
    """relu(x) with the mask [x > 0] of its derivative taken as all ones."""

    @staticmethod
    def forward(ctx, x):
        return torch.relu(x)

    @staticmethod
    def backward(ctx, g):
        return g


def _wrong_aea(x, f_x, sd, prefix, mode, scale_value=50.0):
    _, clamp = R.aea(x, f_x, sd, prefix, mode)
    if mode == "aea":
        return _TailSigmoid.apply(scale_value * (f_x - clamp)), clamp
    return torch.softmax(_OpenRelu.apply(f_x - clamp), dim=-1), clamp


def _both(F, G, mode):
    import network as net
    mod = (net.AEAModule if mode == "aea" else net.AEALReluModule)(SHAPE[2] * SHAPE[3])
    synth_(mod, 11)
    args = (F, G, gen(23, SHAPE), gen(24, SHAPE, 1.0, 0.2, relu=True),
            gen(25, SHAPE, 1.0, 0.2, relu=True), gen(26, SHAPE), state_dict_of(mod), mode,
            torch.float64)
    true = aea_attention_grads(*args)
    wrong = aea_attention_grads(*args, aea=_wrong_aea)
    for a, b in zip(true[:4], wrong[:4]):  # the same forward: only the derivative differs
        assert torch.equal(a, b)
    return true, wrong


def test_peaked_attention_inputs():
    """The generator's contract: fp32 (B, C, h, w), unit key columns, one dominant key per
    query (a permutation per image) with its probability spread over the clamp's range, and
    the same values for the same seed."""
    B, C, h, w = 3, 64, 9, 7
    F, G = peaked_attention_inputs(B, C, h, w, 3)
    assert F.shape == G.shape == (B, C, h, w) and F.dtype == G.dtype == torch.float32
    F2, G2 = peaked_attention_inputs(B, C, h, w, 3)
    assert torch.equal(F, F2) and torch.equal(G, G2)
    assert not torch.equal(F, peaked_attention_inputs(B, C, h, w, 4)[0])
    Gd = G.double().view(B, C, -1)
    assert (Gd.norm(dim=1) - 1).abs().max() < 1e-6
    P = torch.softmax(torch.bmm(F.double().view(B, C, -1).transpose(1, 2), Gd), -1)
    top, key = P.max(-1)
    for b in range(B):
        assert sorted(key[b].tolist()) == list(range(h * w))
    assert top.min() > 0.2 and top.max() < 0.98
    assert (top < 0.45).any() and (top > 0.85).any()


def test_clamp_liveness():
    P = torch.tensor([[[0.70, 0.30], [0.50, 0.50], [0.99, 0.01], [0.60, 0.40]]]).double()
    P = torch.cat([P, torch.zeros(1, 4, 2, dtype=torch.float64)], 2)  # (1, 4, 4)
    c = torch.tensor([0.65, 0.7, 0.8, 0.45]).double().view(1, 4, 1)
    # aea: |50 (P - c)| < 4 needs an entry within 0.08 of c: rows 0 (0.70) and 3 (0.40)
    assert clamp_liveness(P, c, "aea") == 0.5
    # relu: an entry above c: rows 0, 2 and 3
    assert clamp_liveness(P, c, "relu") == 0.75


@pytest.mark.parametrize("mode", MODES)
def test_live_inputs_discriminate(mode):
    """On the live inputs the wrong derivative moves every f_psi gradient and dF by rel-L2
    >= 0.1 (the kernel tests' bars are <= 1e-4), and the case the kernel tests share meets
    its liveness conditions (asserted in helpers.aea_live_bars)."""
    case = aea_live_case(mode, SHAPE)
    true, wrong = _both(case.F, case.G, mode)
    assert all(torch.equal(true[4][k], case.g64[k]) for k in AEA_GRADS)
    for k in ("dF",) + AEA_GRADS[3:]:
        d = rel_l2(wrong[4][k], true[4][k])
        print(f"live {mode} {k}: wrong derivative off by {d:.3e}")
        assert d >= 0.1, (k, d)


@pytest.mark.parametrize("mode", MODES)
def test_flat_inputs_do_not_discriminate(mode):
    """On the flat inputs (gen(21 / 22, ..., 0.2): P ~ 1 / HW everywhere) the clamp is dead.
    'aea': Q < 1e-13, so 1 - Q is 1 to fp32 and beyond and the wrong derivative changes no
    gradient by 1e-6. 'relu': no entry of P passes its clamp, and the true dF, dG and f_psi
    gradients are identically zero: a check on them holds whatever the second softmax's row
    statistics or dq_dot are. With the mask all ones the f_psi gradients stay zero to
    rounding too (dc = -rowsum(dR), and a softmax backward's rows sum to zero), so no f_psi
    check sees the mask there; only dF and dG would (~1.5e-3)."""
    F, G = gen(21, SHAPE, 0.2), gen(22, SHAPE, 0.2)
    true, wrong = _both(F, G, mode)
    assert clamp_liveness(true[2], true[1], mode) == 0.0
    if mode == "aea":
        assert true[3].max() < 1e-13
        for k in AEA_GRADS:
            d = rel_l2(wrong[4][k], true[4][k])
            print(f"flat aea {k}: wrong derivative off by {d:.3e}")
            assert d < 1e-6, (k, d)
    else:
        assert not (true[2] > true[1]).any()
        for k in ("dF", "dG") + AEA_GRADS[3:]:
            print(f"flat relu {k}: true max {float(true[4][k].abs().max()):.3e}, "
                  f"all-ones mask max {float(wrong[4][k].abs().max()):.3e}")
            assert not true[4][k].any(), k
            if k.startswith("f_psi"):
                assert wrong[4][k].abs().max() < 1e-12, k
