"""The inputs of the training-glue kernel tests (tests/train_glue_ref.py) tell a wrong kernel
from a right one. float64 on the CPU: each reference beside a deliberately wrong form of the
same operation, the slips a per-plane kernel invites: HW written for HW - 1 in the unbiased
variance's divisor (mean_variance_norm backward, the loss seed), a grid-stride loop that
does not repeat (sq_diff_mean), a softmax backward without its rowsum(dP P) term and a softmax
without the row maximum subtracted (SANet attention backward on peaked rows). The wrong form
has to miss the GPU test's bar by a factor of 3 (the sum: to miss it), so a kernel test that
passes at that bar rules the slip out."""
import pytest
import torch

import train_glue_ref as T
from helpers import rel_l2


@pytest.mark.parametrize("shape", T.MVN_SHAPES)
def test_mvn_backward_inputs_discriminate(shape):
    x, dy, _ = T.mvn_inputs(shape)
    ref = T.mvn_backward_ref(x, dy)
    assert rel_l2(T.mvn_backward_form(x, dy), ref) < 1e-12  # the closed form is autograd's
    f32 = rel_l2(T.mvn_backward_ref(x, dy, torch.float32), ref)
    d = rel_l2(T.mvn_backward_form(x, dy, slip=True), ref)
    print(f"mvn backward {shape}: HW for HW - 1 moves dx by {d:.3e}, fp32 autograd {f32:.3e}")
    assert d > 3 * T.MVN_BAR, (shape, d)
    assert f32 < T.MVN_BAR / 3, (shape, f32)


@pytest.mark.parametrize("wts", T.SEED_WTS)
@pytest.mark.parametrize("content", [False, True])
@pytest.mark.parametrize("shape", T.SEED_SHAPES)
def test_loss_seed_inputs_discriminate(shape, content, wts):
    F, Tt, Fc, _ = T.seed_inputs(shape)
    Fc = Fc if content else None
    ref = T.seed_ref(F, Tt, Fc, wts)
    assert rel_l2(T.seed_form(F, Tt, Fc, wts), ref) < 1e-12
    f32 = rel_l2(T.seed_ref(F, Tt, Fc, wts, torch.float32), ref)
    d = rel_l2(T.seed_form(F, Tt, Fc, wts, slip=True), ref)
    print(f"loss seed {shape} content {content} wts {wts}: HW for HW - 1 moves it by {d:.3e}, "
          f"fp32 autograd {f32:.3e}")
    assert d > 3 * T.SEED_BAR, (shape, d)
    assert f32 < T.SEED_BAR / 3, (shape, f32)


@pytest.mark.parametrize("n", [n for n in T.SQ_DIFF_NS if n > T.SQ_DIFF_GRID])
def test_sq_diff_inputs_discriminate(n):
    """A grid of 1024 x 256 threads that takes one element each leaves out the tail."""
    a, b = T.sq_diff_inputs(n)
    ref = T.sq_diff_ref(a, b)
    d = abs(T.sq_diff_ref(a, b, first=T.SQ_DIFF_GRID) - ref) / ref
    print(f"sq_diff_mean n = {n}: one pass of the grid is off by {d:.3e}")
    assert d > T.SQ_DIFF_BAR, (n, d)


@pytest.mark.parametrize("case", T.ATTN_PEAKED)
def test_peaked_attention_inputs_discriminate(case):
    """The rows are peaked (median largest probability >= 0.7), three times every gradient's
    CPU float32 error stays under the 1e-4 cap of its bar, a softmax backward without
    rowsum(dP P) moves dF by more than 1, and where the largest logit passes 89 a float32
    exp(S) without the row maximum is not finite."""
    (F, G, H, dO), S, P, g64, f32 = T.attn_peaked_case(case)
    peak = T.row_peak_median(P)
    wrong = T.attn_grads(F, G, H, dO, drop_rowsum=True)[2]
    d = rel_l2(wrong["dF"], g64["dF"])
    print(f"peaked attention {case}: |S| max {float(S.abs().max()):.1f}, S max "
          f"{float(S.max()):.1f}, peak median {peak:.3f}, fp32 "
          + " ".join(f"{k} {v:.2e}" for k, v in f32.items())
          + f", no rowsum moves dF by {d:.2f}")
    assert peak >= 0.7, peak
    assert all(torch.isfinite(v).all() and float(v.norm()) > 1e-3 for v in g64.values())
    assert all(3 * f32[k] <= 1e-4 for k in T.ATTN_GRADS), f32  # no bar passes its cap
    assert T.row_sum_residue(g64["dG"]) < 1e-12
    assert d > 1, d
    if float(S.abs().max()) > 89:
        assert float(S.max()) > 89  # (an overflow needs the positive side)
        assert not torch.isfinite(torch.exp(S.float())).all()
