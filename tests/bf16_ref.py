"""CPU emulation of the opt-in bf16 inference path (rpst_conv2d_bf16, DESIGN.md "bf16
inference"): test infrastructure, not a fallback.

The kernel's contract is restated operation by operation: the fp32 input value is formed (the
AdaIN affine first, where the conv loads through it), rounded once to bf16 (nearest even); the
weights are rounded the same way; the products are exact; the sum is taken in float64 here (or
in float32, `acc`, to measure what the accumulation order is worth); bias and activation follow.
"""
import torch
import torch.nn.functional as F

from oracle import restate as R

ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2


def round_bf16(x):
    """x rounded once to bf16 (nearest even), as an fp32 tensor."""
    return x.float().bfloat16().float()


def activate(y, act):
    if act == ACT_RELU:
        return F.relu(y)
    if act == ACT_LRELU:
        return F.leaky_relu(y, 0.2)
    return y


def conv_bf16(x, w, b=None, pad="zero", act=ACT_NONE, acc=torch.float64):
    """act(conv3x3(round_bf16(x), round_bf16(w)) + b), summed in `acc`; pad "zero" / "reflect".
    -> a tensor of dtype acc."""
    x, w = round_bf16(x).to(acc), round_bf16(w).to(acc)
    x = F.pad(x, (1, 1, 1, 1), mode="reflect" if pad == "reflect" else "constant")
    return activate(F.conv2d(x, w, None if b is None else b.to(acc)), act)


def conv_plain(x, w, b=None, pad="zero", act=ACT_NONE, acc=torch.float64):
    """The same conv without any rounding (the layers the plan keeps on fp32 kernels)."""
    x = F.pad(x.to(acc), (1, 1, 1, 1), mode="reflect" if pad == "reflect" else "constant")
    return activate(F.conv2d(x, w.to(acc), None if b is None else b.to(acc)), act)


def adain_affine(x, mean_c, std_c, mean_s, std_s, dtype=torch.float32):
    """The loader's AdaIN value fma(x - mean_c, std_s / std_c, mean_s) per (n, c), formed in
    `dtype` from fp32 statistics (N, C, 1, 1)."""
    x, mean_c, std_c, mean_s, std_s = (t.float().to(dtype) for t in (x, mean_c, std_c, mean_s,
                                                                     std_s))
    return (x - mean_c) * (std_s / std_c) + mean_s


def adain_rp_test_bf16(content, style, sd, rp_blocks, eligible, acc=torch.float64):
    """AdaINRPNet.test() (oracle.restate.adain_rp_test) as precision "bf16" runs it:
    eligible(cout, cin) says which convs round their input and weights to bf16 (the plan's
    conv2d_bf16 steps); activations between layers are fp32, as in memory; the statistics are
    fp32 values of a float64 reduction; the AdaIN affine is formed in fp32 in the first
    decoder conv's loader. Every conv sums in `acc`. -> fp32 (N, 3, H, W)."""
    def stack(x, prefix):
        for i in range(rp_blocks):
            w, b = sd[f"{prefix}{2 * i}.weight"], sd[f"{prefix}{2 * i}.bias"]
            f = conv_bf16 if eligible(w.shape[0], w.shape[1]) else conv_plain
            x = f(x, w, b, "zero", ACT_RELU, acc).float()
        return x

    with torch.no_grad():
        cf = stack(content.float(), "rp_shared_encoder.")
        sf = stack(style.float(), "rp_shared_encoder.")
        (mc, sc), (ms, ss) = (tuple(t.float() for t in R.calc_mean_std(f.double()))
                              for f in (cf, sf))
        return stack(adain_affine(cf, mc, sc, ms, ss), "rp_decoder.")
