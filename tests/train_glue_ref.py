"""Inputs, shapes and CPU references of the training-glue kernel tests
(tests/test_gpu_train_glue.py, the peaked cases of tests/test_gpu_attn_bwd.py), shared with
tests/test_train_glue_cpu.py, which shows in float64 that these inputs tell a wrong kernel
from a right one. Every reference is torch autograd on the CPU in the given dtype (float64:
the reference; float32: the rounding floor of the same formula) on the fp32 inputs of
helpers.gen. The closed forms beside them take the divisor of the unbiased variance as an
argument, so the HW-for-HW-1 slip can be written down."""
import torch
import torch.nn.functional as Fn

from helpers import gen
from oracle import restate as R

# ---- mean_variance_norm backward ------------------------------------------------------------
# (N, C, H, W): HW = 35 (less than one wave), 256 (exactly one stride of the per-plane loop),
# 257 (one element in the second iteration), 1000 (several iterations), 4096 (production)
MVN_SHAPES = [(1, 5, 5, 7), (2, 3, 16, 16), (1, 3, 257, 1), (2, 2, 25, 40), (1, 2, 64, 64)]
MVN_BAR = 1e-6


def mvn_inputs(shape):
    """x, dy, and the prefill of the accumulate = 1 run."""
    return gen(1, shape, 2.0, 0.5), gen(2, shape), gen(3, shape)


def mvn_backward_ref(x, dy, dtype=torch.float64):
    xd = x.to(dtype).clone().requires_grad_()
    R.mean_variance_norm(xd).backward(dy.to(dtype))
    return xd.grad


def mvn_backward_form(x, dy, slip=False):
    """dx = (dy - mean(dy) - y sum(dy y) / (HW - 1)) / s in float64; slip: HW for HW - 1."""
    x, dy = x.double(), dy.double()
    hw = x.shape[2] * x.shape[3]
    m, s = R.calc_mean_std(x)
    y = (x - m) / s
    k = (dy * y).sum((2, 3), keepdim=True) / (hw if slip else hw - 1)
    return (dy - dy.mean((2, 3), keepdim=True) - y * k) / s


# ---- AdaIN backward -------------------------------------------------------------------------
ADAIN_SHAPES = [(2, 6, 9, 11), (3, 2, 16, 16), (1, 2, 257, 1), (2, 3, 20, 23), (1, 3, 64, 64)]


def adain_inputs(shape):
    """content, style, g: the inputs of test_adain_backward."""
    return gen(8, shape, 2.0, 0.5), gen(9, shape, 1.0, -1.0), gen(10, shape)


def adain_backward_ref(c, s, g, dtype=torch.float64):
    cd, sd = (t.to(dtype).clone().requires_grad_() for t in (c, s))
    R.adain(cd, sd).backward(g.to(dtype))
    return cd.grad, sd.grad


# ---- the loss seed --------------------------------------------------------------------------
SEED_SHAPES = [(1, 5, 5, 7), (2, 3, 16, 17), (1, 2, 64, 64)]
SEED_WTS = [(10.0, 1.0), (0.37, 2.5)]
SEED_BAR = 1e-6


def seed_inputs(shape):
    """F, the style target T, the content target Fc, and the prefill of the acc run."""
    return (gen(3, shape, 1.0, 0.4), gen(4, shape, 1.5, -0.2), gen(5, shape, 1.0, 0.3),
            gen(6, shape))


def seed_ref(F, T, Fc, wts, dtype=torch.float64):
    """d/dF of w_s style_loss(F, T) + w_c mse(F, Fc) (Fc None: the style term alone)."""
    Fd = F.to(dtype).clone().requires_grad_()
    loss = wts[0] * R.style_loss(Fd, T.to(dtype))
    if Fc is not None:
        loss = loss + wts[1] * Fn.mse_loss(Fd, Fc.to(dtype))
    loss.backward()
    return Fd.grad


def seed_form(F, T, Fc, wts, slip=False):
    """The same in closed form, float64: a + b (F - mu) + w_c 2 (F - Fc) / (N C HW) with
    a = w_s 2 (mu - mu_t) / (N C HW), b = w_s 2 (sigma - sigma_t) / (N C (HW - 1) sigma);
    slip: HW for HW - 1 in b."""
    F, T = F.double(), T.double()
    nc, hw = F.shape[0] * F.shape[1], F.shape[2] * F.shape[3]
    mu, sd = R.calc_mean_std(F)
    mut, sdt = R.calc_mean_std(T)
    a = wts[0] * 2.0 * (mu - mut) / (nc * hw)
    b = wts[0] * 2.0 * (sd - sdt) / (nc * (hw if slip else hw - 1) * sd)
    out = a + b * (F - mu)
    if Fc is not None:
        out = out + wts[1] * 2.0 * (F - Fc.double()) / (nc * hw)
    return out


# ---- sq_diff_mean ---------------------------------------------------------------------------
# 262144 = 1024 blocks of 256 (the whole grid, one pass); 262145 is the first n at which the
# grid-stride loop repeats
SQ_DIFF_NS = [1, 255, 257, 65536, 262144, 262145, 1000003]
SQ_DIFF_GRID = 1024 * 256
SQ_DIFF_BAR = 1e-6


def sq_diff_inputs(n):
    return gen(11, (n,), 1.0, 0.5), gen(12, (n,))


def sq_diff_ref(a, b, first=None):
    """float64 mean of (a - b)^2 (a python float); first: the sum over the first `first`
    elements only, still divided by n (a grid-stride loop that does not repeat)."""
    d = (a.double() - b.double())[:first]
    return float((d * d).sum() / a.numel())


# ---- nearest x2 upsample backward -----------------------------------------------------------
UPSAMPLE_G_SHAPES = [(2, 3, 2, 2), (1, 5, 14, 18), (2, 2, 66, 130)]


def upsample_backward_ref(g, dtype=torch.float64):
    n, c, h2, w2 = g.shape
    x = torch.zeros((n, c, h2 // 2, w2 // 2), dtype=dtype, requires_grad=True)
    Fn.interpolate(x, scale_factor=2, mode="nearest").backward(g.to(dtype))
    return x.grad


# ---- SANet attention backward on peaked rows ------------------------------------------------
# (B, C, HWc, HWs, scale of F and G)
ATTN_PEAKED = [(2, 64, 300, 520, 3.0),    # ragged tiles, HWc != HWs
               (2, 48, 300, 520, 3.0),    # C off the 16-byte path
               (2, 128, 257, 129, 2.0),   # one element past a tile on both sides
               (1, 64, 2100, 68, 3.0),    # 2048 + 52 queries: crosses the chunk seam
               (1, 512, 1024, 1024, 1.0)]  # the training channel count, 8 x 8 tiles
ATTN_GRADS = ("dF", "dG", "dH")


def attn_inputs(case):
    B, C, hwc, hws, s = case
    return (gen(5, (B, C, hwc), s), gen(6, (B, C, hws), s), gen(7, (B, C, hws), 1.0),
            gen(8, (B, C, hwc), 1.0))


def attn_grads(F, G, H, dO, dtype=torch.float64, drop_rowsum=False):
    """Autograd in `dtype` of sum(O dO), O = H softmax(F^T G)^T -> (S, P, {dF, dG, dH}), all
    detached. drop_rowsum: the softmax backward taken as dS = P dP, its rowsum(dP P) term
    dropped (the forward is unchanged)."""
    Fd, Gd, Hd = (x.to(dtype).clone().requires_grad_() for x in (F, G, H))
    S = torch.bmm(Fd.transpose(1, 2), Gd)
    P = _NoRowsumSoftmax.apply(S) if drop_rowsum else torch.softmax(S, -1)
    (torch.bmm(Hd, P.transpose(1, 2)) * dO.to(dtype)).sum().backward()
    return S.detach(), P.detach(), dict(dF=Fd.grad, dG=Gd.grad, dH=Hd.grad)


class _NoRowsumSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, S):
        P = torch.softmax(S, -1)
        ctx.save_for_backward(P)
        return P

    @staticmethod
    def backward(ctx, dP):
        return ctx.saved_tensors[0] * dP


def row_peak_median(P):
    """Median over the query rows of the largest probability."""
    return float(P.amax(-1).flatten().median())


_ATTN_CASES = {}


def attn_peaked_case(case):
    """The float64 reference of one ATTN_PEAKED case and the CPU float32 torch form's rel-L2
    against it per gradient, formed once per session and shared (read only):
    (inputs, S, P, g64, {name: fp32 error}), the fp32 error dict also holding under 'gsum'
    the float32 form's row_sum_residue of dG."""
    from helpers import rel_l2
    if case not in _ATTN_CASES:
        inputs = attn_inputs(case)
        S, P, g64 = attn_grads(*inputs)
        g32 = attn_grads(*inputs, dtype=torch.float32)[2]
        f32 = {k: rel_l2(g32[k], g64[k]) for k in ATTN_GRADS}
        f32["gsum"] = row_sum_residue(g32["dG"])
        _ATTN_CASES[case] = (inputs, S, P, g64, f32)
    return _ATTN_CASES[case]


def row_sum_residue(dG):
    """max_c |sum_j dG[c][j]| / max|dG|: the softmax is shift invariant per row, so the rows of
    dS sum to 0 and so does F dS 1 (float64: ~1e-16)."""
    dG = dG.double()
    return float(dG.sum(-1).abs().max() / dG.abs().max())
