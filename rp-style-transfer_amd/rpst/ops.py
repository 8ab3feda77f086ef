"""Tensor-level wrappers over the rpst C ABI (device memory and streams come from torch).

Every op takes ROCm-device fp32 tensors, allocates its outputs/workspace through the
torch caching allocator and launches on torch's current stream. CPU tensors, wrong
dtypes and autograd-requiring inputs raise: this is the product path and it has no
CPU or ATen fallback (the CPU restatement lives in oracle/, for tests only).
"""
from __future__ import annotations

from typing import Optional, Tuple

import os

import torch

from . import _lib

# the codes of include/rpst.h (RPST_<name>), read from it
PAD_ZERO, PAD_REFLECT = _lib.constants("PAD_ZERO", "PAD_REFLECT")
IN_NONE, IN_MAXPOOL2, IN_UPSAMPLE2, IN_ADD_UPSAMPLE2, IN_ADAIN, IN_ADD_ADAIN = _lib.constants(
    "IN_NONE", "IN_MAXPOOL2", "IN_UPSAMPLE2", "IN_ADD_UPSAMPLE2", "IN_ADAIN", "IN_ADD_ADAIN")
# conv epilogue: none / ReLU / LeakyReLU(0.2)
ACT_NONE, ACT_RELU, ACT_LRELU = _lib.constants("ACT_NONE", "ACT_RELU", "ACT_LRELU")
# rpst_conv2d_algorithm
ALGO_DIRECT, ALGO_WINOGRAD, ALGO_WINOGRAD4, ALGO_NARROW = _lib.constants(
    "CONV_DIRECT", "CONV_WINOGRAD", "CONV_WINOGRAD4", "CONV_NARROW")
# rpst_wct_status bits
WCT_NOCONV, WCT_TIMEOUT = _lib.constants("WCT_NOCONV", "WCT_TIMEOUT")


def _act(relu) -> int:
    """The conv `relu` argument: a bool (ReLU or not) or an ACT_* code."""
    if isinstance(relu, bool):
        return ACT_RELU if relu else ACT_NONE
    a = int(relu)
    if a not in (ACT_NONE, ACT_RELU, ACT_LRELU):
        raise ValueError(f"rpst: unknown activation code {relu}")
    return a


class Trace:
    """Optional per-launch HIP-event timing (bench.py): records (name, flops, bytes,
    start, end) around each traced launch on torch's current stream, which is the
    stream every rpst kernel is launched on."""

    def __init__(self):
        self.records = []

    def summary(self, median: bool = False):
        """name -> {launches, ms (total), flops, bytes}. median=True reports launches x the
        median launch time as "ms", so one launch delayed by host work between the events
        (an idle GPU waiting on the host) does not move a short stand-alone measurement."""
        torch.cuda.synchronize()
        agg, times = {}, {}
        for name, flops, nbytes, e0, e1 in self.records:
            ms = e0.elapsed_time(e1)
            a = agg.setdefault(name, {"launches": 0, "ms": 0.0, "flops": flops, "bytes": nbytes})
            a["launches"] += 1
            a["ms"] += ms
            times.setdefault(name, []).append(ms)
        if median:
            for name, a in agg.items():
                t = sorted(times[name])
                a["ms"] = t[len(t) // 2] * a["launches"]
        return agg


TRACE: Optional[Trace] = None


class _traced:
    def __init__(self, name, flops=0.0, nbytes=0.0):
        self.args = (name, flops, nbytes)

    def __enter__(self):
        if TRACE is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if TRACE is not None:
            self.e1.record()
            TRACE.records.append((*self.args, self.e0, self.e1))


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _check(*ts: torch.Tensor, dtype=torch.float32) -> None:
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "rpst kernels run on a ROCm GPU only; got a CPU tensor (the CPU reference "
                "path is oracle/, which is test infrastructure, not a fallback)")
        if t.dtype != dtype:
            raise RuntimeError(f"rpst kernel expects {dtype} tensors, got {t.dtype}")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"rpst: tensors on different devices ({dev} vs {t.device})")
        if torch.is_grad_enabled() and t.requires_grad:
            raise NotImplementedError(
                "rpst: a bare kernel op has no autograd formula (the networks train through "
                "rpst.autograd's model steps); call it under torch.no_grad()")


def _c(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous() else t.contiguous()


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _shape(x) -> tuple:  # x: a tensor or its shape
    return tuple(x.shape) if isinstance(x, torch.Tensor) else tuple(x)


# ---- the frame of the conv wrappers: checked input, output, bias pointer, trace ----------
def _conv_in(x: torch.Tensor, *others):
    """x (N, Cin, H, W) and `others` (None entries skipped) pass _check -> x contiguous, shape."""
    assert x.dim() == 4
    _check(x, *others)
    x = _c(x)
    return x, tuple(x.shape)


def _conv_out(x: torch.Tensor, shape, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A conv's output on x's device: a new fp32 tensor of `shape`, or the caller's `out`
    validated against it (a channel count of None: any)."""
    if out is None:
        return torch.empty(shape, device=x.device, dtype=torch.float32)
    n, c, h, w = shape
    if out.dim() != 4 or not out.is_contiguous() or out.dtype != torch.float32 or \
            out.device != x.device or (out.shape[0], out.shape[2], out.shape[3]) != (n, h, w) \
            or (c is not None and out.shape[1] != c):
        raise ValueError(f"rpst: out must be a contiguous fp32 ({n}, {'C' if c is None else c}, "
                         f"{h}, {w}) tensor on the input's device")
    return out


def _bias_ptr(bias: Optional[torch.Tensor]) -> Optional[int]:
    return _ptr(None if bias is None else _c(bias.detach()))


def _conv_traced(shape, cout: int, ksize: int, in_op: int, moved: int, name=None):
    """Trace entry of a k x k conv over a (n, cin, hs, ws) source: `moved` fp32 elements."""
    n, cin, hs, ws = shape
    h, w = conv_out_hw(hs, ws, in_op)
    return _traced(name or _conv_name(ksize, cin, cout, hs, ws, n, in_op),
                   2.0 * n * cout * h * w * cin * ksize * ksize, 4.0 * moved)


def calc_mean_std(feat: torch.Tensor, eps: float = 1e-5) -> Tuple[torch.Tensor, torch.Tensor]:
    """network/base.py:399-407 on the GPU: (N,C,H,W) -> mean, std of shape (N,C,1,1)."""
    assert feat.dim() == 4
    _check(feat)
    feat = _c(feat)
    N, C = feat.shape[:2]
    hw = feat.numel() // (N * C)
    mean = torch.empty((N, C, 1, 1), device=feat.device, dtype=torch.float32)
    std = torch.empty_like(mean)
    with _traced(f"stats C{C} {hw}px N{N}", 0.0, 4.0 * N * C * hw):
        _lib.call("rpst_calc_mean_std", feat.data_ptr(), mean.data_ptr(), std.data_ptr(),
                  N, C, hw, eps, _stream(feat))
    return mean, std


def adaptive_instance_normalization(content: torch.Tensor, style: torch.Tensor,
                                    eps: float = 1e-5,
                                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """network/base.py:410-418 on the GPU (stats + apply, 2 launches)."""
    assert content.size() == style.size()
    assert content.dim() == 4
    _check(content, style)
    content, style = _c(content), _c(style)
    N, C = content.shape[:2]
    hw = content.numel() // (N * C)
    if out is None:
        out = torch.empty_like(content)
    ws, nbytes = _lib.workspace("adain", content, N, C)
    with _traced(f"adain C{C} {hw}px N{N}", 0.0, 3.0 * 4 * N * C * hw):
        _lib.call("rpst_adain", content.data_ptr(), style.data_ptr(), out.data_ptr(), N, C, hw,
                  eps, ws.data_ptr(), nbytes, _stream(content))
    return out


SEG_LABELS = 256  # rows per image of a segment plan / per plane of masked AdaIN params


def _check_seg(seg: torch.Tensor, n: int, like: torch.Tensor) -> torch.Tensor:
    _check(seg, dtype=torch.uint8)
    if seg.dim() != 3 or seg.shape[0] != n:
        raise ValueError(f"rpst: label map must be uint8 (N={n}, h, w), got {tuple(seg.shape)}")
    if seg.device != like.device:
        raise RuntimeError(f"rpst: tensors on different devices ({like.device} vs {seg.device})")
    return _c(seg)


def segment_plan(c_seg: torch.Tensor, s_seg: torch.Tensor) -> torch.Tensor:
    """compute_label_info (network/base.py:421-439) on the GPU for N image pairs: uint8 label
    maps (N, hc, wc) and (N, hs, ws) -> int32 (N, 256, 4) = (content count, style count,
    valid, 0) per label. Stays on the device; one plan serves every feature level."""
    if c_seg.dim() != 3:
        raise ValueError(f"rpst: label map must be uint8 (N, h, w), got {tuple(c_seg.shape)}")
    n = c_seg.shape[0]
    c_seg, s_seg = _check_seg(c_seg, n, c_seg), _check_seg(s_seg, n, c_seg)
    plan = torch.empty((n, SEG_LABELS, 4), device=c_seg.device, dtype=torch.int32)
    hwc, hws = c_seg[0].numel(), s_seg[0].numel()
    with _traced(f"segplan {hwc}px N{n}", 0.0, 1.0 * n * (hwc + hws)):
        _lib.call("rpst_segment_plan", c_seg.data_ptr(), s_seg.data_ptr(), n, hwc, hws,
                  plan.data_ptr(), _stream(c_seg))
    return plan


def _masked_args(content, style, c_seg, s_seg, plan):
    assert content.dim() == 4 and style.dim() == 4
    _check(content, style)
    if content.shape[:2] != style.shape[:2]:
        raise ValueError("rpst: content and style differ in N or C")
    content, style = _c(content), _c(style)
    n = content.shape[0]
    c_seg, s_seg = _check_seg(c_seg, n, content), _check_seg(s_seg, n, content)
    if tuple(c_seg.shape[1:]) != tuple(content.shape[2:]) or \
            tuple(s_seg.shape[1:]) != tuple(style.shape[2:]):
        raise ValueError("rpst: label maps must have their feature's (h, w): "
                         f"{tuple(c_seg.shape[1:])} vs {tuple(content.shape[2:])}, "
                         f"{tuple(s_seg.shape[1:])} vs {tuple(style.shape[2:])}")
    if plan is None:
        plan = segment_plan(c_seg, s_seg)
    else:
        _check(plan, dtype=torch.int32)
        if tuple(plan.shape) != (n, SEG_LABELS, 4) or plan.device != content.device:
            raise ValueError(f"rpst: segment plan must be int32 ({n}, 256, 4) on the tensors' "
                             "device")
        plan = _c(plan)
    return content, style, c_seg, s_seg, plan


def masked_adain_params(content: torch.Tensor, style: torch.Tensor, c_seg: torch.Tensor,
                        s_seg: torch.Tensor, plan: Optional[torch.Tensor] = None,
                        eps: float = 1e-5) -> torch.Tensor:
    """Per-label AdaIN statistics (network/base.py:465-491 for every valid label at once):
    -> fp32 (N, C, 256, 4) = (mean_c, std_c, std_s, mean_s) per (image, channel, label);
    rows of invalid or absent labels are pass-through (std_c = -1)."""
    return _masked_params(*_masked_args(content, style, c_seg, s_seg, plan), eps)


def _masked_params(content, style, c_seg, s_seg, plan, eps):
    N, C = content.shape[:2]
    hwc, hws = c_seg[0].numel(), s_seg[0].numel()
    params = torch.empty((N, C, SEG_LABELS, 4), device=content.device, dtype=torch.float32)
    ws, nbytes = _lib.workspace("masked_adain", content, N, C)
    with _traced(f"masked stats C{C} {hwc}px N{N}", 0.0, (4.0 * C + 1) * N * (hwc + hws)):
        _lib.call("rpst_masked_adain_params", content.data_ptr(), style.data_ptr(),
                  c_seg.data_ptr(), s_seg.data_ptr(), plan.data_ptr(), N, C, hwc, hws, eps,
                  params.data_ptr(), ws.data_ptr(), nbytes, _stream(content))
    return params


def masked_adain(content: torch.Tensor, style: torch.Tensor, c_seg: torch.Tensor,
                 s_seg: torch.Tensor, skip: Optional[torch.Tensor] = None,
                 plan: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                 eps: float = 1e-5) -> torch.Tensor:
    """adaptive_instance_normalization_with_segment (network/base.py:494-530) for a batch,
    image n with its own label maps c_seg[n], s_seg[n] (uint8, already at the features'
    sizes): [skip +] the content with every validly labelled pixel re-normalised to its
    label's style statistics; other pixels are copied (plan + stats + apply launches)."""
    content, style, c_seg, s_seg, plan = _masked_args(content, style, c_seg, s_seg, plan)
    if skip is not None:
        _check(skip)
        if skip.shape != content.shape or skip.device != content.device:
            raise ValueError("rpst: skip must have the content's shape and device")
        skip = _c(skip)
    params = _masked_params(content, style, c_seg, s_seg, plan, eps)
    N, C = content.shape[:2]
    hw = c_seg[0].numel()
    if out is None:
        out = torch.empty_like(content)
    elif out.shape != content.shape or not out.is_contiguous() or out.dtype != torch.float32 \
            or out.device != content.device:
        raise ValueError("rpst: out must be a contiguous fp32 tensor of the content's shape")
    with _traced(f"masked apply C{C} {hw}px N{N}", 0.0,
                 ((3.0 if skip is not None else 2.0) * 4 * C + 1) * N * hw):
        _lib.call("rpst_masked_adain_apply", content.data_ptr(), _ptr(skip), c_seg.data_ptr(),
                  params.data_ptr(), out.data_ptr(), N, C, hw, _stream(content))
    return out


def mean_variance_norm(feat: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """network/sanet.py:20-24 on the GPU."""
    assert feat.dim() == 4
    _check(feat)
    feat = _c(feat)
    N, C = feat.shape[:2]
    hw = feat.numel() // (N * C)
    out = torch.empty_like(feat)
    ws, nbytes = _lib.workspace("adain", feat, N, C)
    _lib.call("rpst_mean_variance_norm", feat.data_ptr(), out.data_ptr(), N, C, hw, eps,
              ws.data_ptr(), nbytes, _stream(feat))
    return out


def pack_conv_weight(weight: torch.Tensor) -> torch.Tensor:
    """Repack (Cout,Cin,k,k) fp32 weights into the conv kernel's K-major layout."""
    _check(weight)
    weight = _c(weight.detach())
    cout, cin, kh, kw = weight.shape
    assert kh == kw and kh in (1, 3), "rpst conv supports 1x1 and 3x3 kernels"
    nbytes = _lib.load().rpst_conv2d_packed_size(cout, cin, kh)
    packed = torch.empty(nbytes // 4, device=weight.device, dtype=torch.float32)
    _lib.call("rpst_conv2d_pack", weight.data_ptr(), packed.data_ptr(), cout, cin, kh,
              _stream(weight))
    return packed


def pack_conv7_weight(weight: torch.Tensor) -> torch.Tensor:
    """Repack (Cout,Cin,7,7) fp32 weights into the 7x7 kernel's K-major layout
    (rpst_conv7_pack)."""
    _check(weight)
    weight = _c(weight.detach())
    cout, cin, kh, kw = weight.shape
    assert kh == 7 and kw == 7, "pack_conv7_weight takes 7x7 kernels"
    nbytes = _lib.load().rpst_conv7_packed_size(cout, cin)
    packed = torch.empty(nbytes // 4, device=weight.device, dtype=torch.float32)
    _lib.call("rpst_conv7_pack", weight.data_ptr(), packed.data_ptr(), cout, cin,
              _stream(weight))
    return packed


def conv_weight_flip(weight: torch.Tensor) -> torch.Tensor:
    """(Cout, Cin, k, k) -> the flip-transposed (Cin, Cout, k, k) weights of the conv's dgrad
    (rpst_conv_weight_flip)."""
    wd = weight.detach().contiguous()
    cout, cin, k, _ = wd.shape
    wt = torch.empty((cin, cout, k, k), device=wd.device, dtype=torch.float32)
    _lib.call("rpst_conv_weight_flip", wd.data_ptr(), wt.data_ptr(), cout, cin, k, _stream(wd))
    return wt


def conv2d_k7(x: torch.Tensor, packed: torch.Tensor, bias: Optional[torch.Tensor], cout: int,
              pad: int = PAD_REFLECT, act=ACT_NONE, out: Optional[torch.Tensor] = None,
              out_channel_offset: int = 0, x2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(conv7x7(pad3(x)) + bias) (rpst_conv7), written to channels [out_channel_offset,
    out_channel_offset + cout) of `out` (a contiguous (N, C_total, H, W) tensor whose other
    channels are left alone; default: a new (N, cout, H, W) tensor). x2: the conv runs over
    the batch cat([x, x2]) of two equal halves, read in place. Returns `out`."""
    x, (n, cin, h, w) = _conv_in(x, x2, packed, bias, out)
    if x2 is not None:
        if x2.shape != x.shape:
            raise ValueError("rpst: conv2d_k7's second input must have the first one's shape")
        x2 = _c(x2)
        n *= 2
    if out is None and out_channel_offset:
        raise ValueError("rpst: conv2d_k7 with a channel offset needs the tensor to write into")
    out = _conv_out(x, (n, cout if out is None else None, h, w), out)
    with _conv_traced((n, cin, h, w), cout, 7, IN_NONE, n * (cin + cout) * h * w,
                      f"conv7x7 {cin}->{cout} {h}x{w} N{n}"):
        _lib.call("rpst_conv7", x.data_ptr(), _ptr(x2), packed.data_ptr(), _bias_ptr(bias),
                  out.data_ptr(), n, cin, h, w, cout, pad, _act(act), int(out_channel_offset),
                  out.shape[1], _stream(x))
    return out


def conv_out_hw(h: int, w: int, in_op: int) -> Tuple[int, int]:
    if in_op == IN_MAXPOOL2:
        return (h + 1) // 2, (w + 1) // 2
    if in_op == IN_UPSAMPLE2:
        return 2 * h, 2 * w
    return h, w


_ALGO_TAG = {ALGO_DIRECT: "conv", ALGO_WINOGRAD: "wino", ALGO_WINOGRAD4: "wino4",
             ALGO_NARROW: "narrow"}


def _conv_name(ksize, cin, cout, hs, ws, n, in_op):
    """Trace key of a conv launch: 'wino3x3' / 'wino43x3' / 'narrow3x3' when the library
    runs it as Winograd F(2x2,3x3) / F(4x4,3x3) / the VALU narrow kernel (the recorded
    FLOPs stay the direct-convolution count). hs, ws: the SOURCE size; the key carries the
    output size."""
    algo = "conv"
    if TRACE is not None:
        algo = _ALGO_TAG[_lib.load().rpst_conv2d_algorithm(cout, cin, hs, ws, ksize, in_op)]
    h, w = conv_out_hw(hs, ws, in_op)
    return f"{algo}{ksize}x{ksize} {cin}->{cout} {h}x{w} N{n} op{in_op}"


# Training conv forms, chosen on the gradient bars derived from the reference's own fp32
# noise floor (tests/test_gpu_train.py, tests/golden/grad_floors.npz; round 6, VERDICT r05
# item 4). A family in TRAIN_F4 runs F(4x4) (the 32-channel form) on every chain of its
# step; the others run F(2x2) ("precise mode") on the differentiated chains and F(4x4) only
# on the step's constant branches (precise_convs(on=False): the VGG loss targets, WCT-RP's
# detached encoder + WCT, SourceNet's frozen VGG). Measured (profiles/r06/train_forms.log):
#   WCT-RP, MultiScale, SourceNet: every test green with F(4x4) throughout, training
#     108.9 -> 118.9, 168.4 -> 188.0, 185.8 -> 206.7 img/s;
#   AdaIN-RP: the CPU-autograd check at hidden 8, 40x56 reads rp_shared_encoder.0.weight
#     3.3e-3 against its 1e-4 floor bar (64.3 -> 75.0 img/s forgone);
#   SAModel / AdaptiveSAModel: the losses move 2.7e-4 against the reference's ~1e-7 floor
#     (their frozen VGG features feed the attention, ~1e3 x amplification), and the steps are
#     slower on F(4x4) anyway (42.8 -> 39.8, 39.8 -> 37.2 img/s); their frozen features stay
#     precise too.
# Where a training step runs F(4x4) it runs the 32-channel form (rpst_conv2d_set_precise(2)),
# not the position-quarter kernel: on the quarter kernel SourceNet's decoder.1.weight gradient
# reads 7.4e-4 against its 6.0e-4 floor bar (RPST_TRAIN_QUARTER=1 is the A/B switch).
#   LDMSAdaINRPNet ("ld"): precise. F(4x4) on its 3x3 chains is 3.3 % faster (600.3 -> 580.3 ms
#     a step at N = 4, 512^2; the step's time is the 7x7 branch's, which has one form) and reads
#     rp_enc0_small_revf.conv.weight 9.7e-4 against its 1e-4 bar in the CPU-autograd check at
#     hidden 8, 16x24 (profiles/ld_train/train_forms.log).
TRAIN_F4 = {"adain": False, "multiscale": True, "wct": True, "sanet": False, "source": True,
            "ld": False}


class precise_convs:
    """Context manager: this thread's convolutions avoid F(4x4,3x3) (rpst_conv2d_set_precise,
    include/rpst.h) — used by the training steps, whose gradients pass ~30 convolutions.
    `model`: the step's network family (TRAIN_F4); on=False: a constant (not differentiated)
    branch of the step, where F(4x4) is allowed. RPST_TRAIN_PRECISE=1 / 0 forces precise /
    F(4x4) everywhere (accuracy A/B). F(4x4) inside a training step is level 2 of the C
    switch: the 32-channel kernel only."""

    def __init__(self, model: Optional[str] = None, on: Optional[bool] = None):
        self.model, self.on = model, on

    def __enter__(self):
        env = os.environ.get("RPST_TRAIN_PRECISE")
        f4 = os.environ.get("RPST_TRAIN_F4")  # comma list of families: TRAIN_F4 override (A/B)
        if env is not None and env != "":
            on = env != "0"
        elif self.on is not None:
            on = self.on
        elif f4 is not None:
            on = self.model not in f4.split(",")
        else:
            on = not TRAIN_F4.get(self.model, False)
        # RPST_TRAIN_QUARTER=1: the constant branches may take the position-quarter kernel
        # too (level 0 instead of 2; accuracy / speed A/B)
        quarter = os.environ.get("RPST_TRAIN_QUARTER", "") == "1"
        self._old = _lib.load().rpst_conv2d_set_precise(1 if on else (0 if quarter else 2))
        return self

    def __exit__(self, *exc):
        _lib.load().rpst_conv2d_set_precise(self._old)
        return False


def pool_pass_pays(x, cout: int, ksize: int) -> bool:
    """For a conv whose input is max_pool2d(x, 2, 2, ceil_mode=True) (x a tensor or its
    shape): True when the library would run the pooled map's conv as F(4x4,3x3) (measured:
    pool pass + F(4x4) is faster than the F(2x2) conv with the pool fused into its loader,
    profiles/r01_bench_sanet_w4*)."""
    n, cin, h, w = _shape(x)
    return ksize == 3 and _lib.load().rpst_conv2d_algorithm(
        cout, cin, (h + 1) // 2, (w + 1) // 2, ksize, IN_NONE) == ALGO_WINOGRAD4


def conv2d_pair(x: torch.Tensor, x2: torch.Tensor, packed: torch.Tensor,
                bias: Optional[torch.Tensor], cout: int, ksize: int, pad: int = PAD_ZERO,
                relu: bool = False) -> torch.Tensor:
    """conv2d over the batch cat([x, x2]) without materialising the concatenation
    (rpst_conv2d_pair: the kernel reads images >= len(x) from x2 in place)."""
    assert x2.dim() == 4 and tuple(x.shape[1:]) == tuple(x2.shape[1:])
    x, (n1, cin, hs, ws) = _conv_in(x, x2, packed, bias)
    x2 = _c(x2)
    n = n1 + x2.shape[0]
    out = _conv_out(x, (n, cout, hs, ws))
    with _conv_traced((n, cin, hs, ws), cout, ksize, IN_NONE,
                      x.numel() + x2.numel() + out.numel()):
        _lib.call("rpst_conv2d_pair", x.data_ptr(), x2.data_ptr(), n1, packed.data_ptr(),
                  _bias_ptr(bias), out.data_ptr(), n, cin, hs, ws, cout, ksize, pad, _act(relu),
                  _stream(x))
    return out


def conv2d(x: torch.Tensor, packed: torch.Tensor, bias: Optional[torch.Tensor], cout: int,
           ksize: int, pad: int = PAD_ZERO, in_op: int = IN_NONE, relu: bool = False,
           aux: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
           out: Optional[torch.Tensor] = None, fold: bool = True) -> torch.Tensor:
    """out = act(conv_k(in_op(x)) + bias) [+ residual]; see include/rpst.h. fold: let the
    library fold an ADAIN loader into per-image weights when it has a workspace for it
    (rpst_conv2d_ws); False keeps the affine in the tile loader (rpst_conv2d)."""
    if in_op == IN_ADD_ADAIN:
        raise ValueError("rpst: the skip-AdaIN operator takes two inputs: use conv2d_skip_adain")
    x, (n, cin, hs, ws) = _conv_in(x, packed, bias, aux, residual)
    h, w = conv_out_hw(hs, ws, in_op)
    out = _conv_out(x, (n, cout, h, w), out)
    if residual is not None:
        residual = _c(residual)
        assert tuple(residual.shape) == (n, cout, h, w)
    if aux is not None:
        aux = _c(aux)
        if in_op == IN_ADAIN:
            assert aux.numel() == 4 * n * cin, "ADAIN aux = [mean_c|mean_s|std_c|std_s]"
        else:
            assert tuple(aux.shape) == (n, cin, h // 2, w // 2)
    with _conv_traced(x.shape, cout, ksize, in_op, x.numel() + out.numel()):
        nbytes = _lib.workspace_bytes("conv2d", n, cin, hs, ws, cout, ksize,
                                      in_op) if fold else 0
        args = (x.data_ptr(), _ptr(aux), packed.data_ptr(), _bias_ptr(bias), _ptr(residual),
                out.data_ptr(), n, cin, hs, ws, cout, ksize, pad, in_op, _act(relu))
        if nbytes:
            ws_t = _lib.scratch(nbytes, x)
            _lib.call("rpst_conv2d_ws", *args, ws_t.data_ptr(), nbytes, _stream(x))
        else:
            _lib.call("rpst_conv2d", *args, _stream(x))
    return out


def conv2d_pool_fuses(x: torch.Tensor, cout: int, ksize: int, in_op: int = IN_NONE) -> bool:
    """True when the library runs this conv on F(4x4), whose epilogue can write the output
    max-pooled (rpst_conv2d_pool)."""
    if os.environ.get("RPST_POOL_EPILOGUE", "") == "0":  # A/B switch: the separate pool pass
        return False
    n, cin, hs, ws = _shape(x)
    return in_op in (IN_NONE, IN_ADAIN, IN_UPSAMPLE2) and _lib.load().rpst_conv2d_algorithm(
        cout, cin, hs, ws, ksize, in_op) == ALGO_WINOGRAD4


def conv2d_pool(x: torch.Tensor, packed: torch.Tensor, bias: Optional[torch.Tensor], cout: int,
                ksize: int, pad: int = PAD_ZERO, in_op: int = IN_NONE,
                relu: bool = False) -> torch.Tensor:
    """max_pool2d(conv2d(x), 2, 2, ceil_mode=True) with the pool in the F(4x4) epilogue
    (rpst_conv2d_pool; the full-resolution output is never written). Needs
    conv2d_pool_fuses(x, cout, ksize, in_op)."""
    assert in_op in (IN_NONE, IN_UPSAMPLE2)
    x, (n, cin, hs, ws) = _conv_in(x, packed, bias)
    h, w = conv_out_hw(hs, ws, in_op)
    out = _conv_out(x, (n, cout, (h + 1) // 2, (w + 1) // 2))
    with _conv_traced(x.shape, cout, ksize, in_op, x.numel() + out.numel()):
        _lib.call("rpst_conv2d_pool", x.data_ptr(), None, packed.data_ptr(), _bias_ptr(bias),
                  out.data_ptr(), n, cin, hs, ws, cout, ksize, pad, in_op, _act(relu),
                  _stream(x))
    return out


def conv2d_masked(x: torch.Tensor, packed: torch.Tensor, cout: int, ksize: int,
                  mask: torch.Tensor, pad: int = PAD_ZERO) -> torch.Tensor:
    """out = conv_k(x), zeroed where mask <= 0 (rpst_conv2d_masked): a conv dgrad fused with
    the ReLU backward of the layer before it (mask = that ReLU's output)."""
    x, (n, cin, h, w) = _conv_in(x, packed, mask)
    mask = _c(mask)
    assert tuple(mask.shape) == (n, cout, h, w)
    out = _conv_out(x, (n, cout, h, w))
    with _conv_traced(x.shape, cout, ksize, IN_NONE, x.numel() + 2 * out.numel()):
        _lib.call("rpst_conv2d_masked", x.data_ptr(), packed.data_ptr(), None, mask.data_ptr(),
                  out.data_ptr(), n, cin, h, w, cout, ksize, pad, _stream(x))
    return out


def conv2d_skip_adain(x: torch.Tensor, content: torch.Tensor, params: torch.Tensor,
                      packed: torch.Tensor, bias: Optional[torch.Tensor], cout: int,
                      ksize: int = 3, pad: int = PAD_REFLECT, relu=ACT_LRELU,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = act(conv(pad(x + AdaIN(content))) + bias): the skip fusion of
    MultiScaleAdaINRPNet.decode (adain_rp.py:301); params = adain_params(...) of
    (content, style) — the sum is formed in the conv's tile loader."""
    assert x.shape == content.shape
    x, (n, cin, h, w) = _conv_in(x, content, params, packed, bias)
    content, params = _c(content), _c(params)
    assert params.numel() == 4 * n * cin, "params = [mean_c|mean_s|std_c|std_s]"
    out = _conv_out(x, (n, cout, h, w), out)
    with _conv_traced(x.shape, cout, ksize, IN_ADD_ADAIN, 2 * x.numel() + out.numel()):
        _lib.call("rpst_conv2d_skip_adain", x.data_ptr(), content.data_ptr(), params.data_ptr(),
                  packed.data_ptr(), _bias_ptr(bias), out.data_ptr(), n, cin, h, w, cout, ksize,
                  pad, _act(relu), _stream(x))
    return out


def conv2d_stats(x: torch.Tensor, packed: torch.Tensor, bias: Optional[torch.Tensor], cout: int,
                 ksize: int, pad: int = PAD_ZERO, in_op: int = IN_NONE, relu: bool = False,
                 aux: Optional[torch.Tensor] = None, eps: float = 1e-5,
                 store_n: Optional[int] = None):
    """conv2d plus calc_mean_std of its output, reduced in the conv epilogue:
    returns (out, mean (N,Cout,1,1), std (N,Cout,1,1)). store_n: write out[:store_n] only
    (rpst_conv2d_stats_store; out[store_n:] unspecified, the statistics cover every image)."""
    x, (n, cin, hs, ws) = _conv_in(x, packed, bias, aux)
    out = _conv_out(x, (n, cout, *conv_out_hw(hs, ws, in_op)))
    mean = torch.empty((n, cout, 1, 1), device=x.device, dtype=torch.float32)
    std = torch.empty_like(mean)
    ws_t, nbytes = _lib.workspace("conv2d_stats", x, n, cin, hs, ws, cout, ksize, in_op)
    args = (x.data_ptr(), _ptr(aux), packed.data_ptr(), _bias_ptr(bias), None, out.data_ptr(), n,
            cin, hs, ws, cout, ksize, pad, in_op, _act(relu), mean.data_ptr(), std.data_ptr(), eps)
    with _conv_traced(x.shape, cout, ksize, in_op, x.numel() + out.numel()):
        if store_n is None or store_n >= n:
            _lib.call("rpst_conv2d_stats", *args, ws_t.data_ptr(), nbytes, _stream(x))
        else:
            _lib.call("rpst_conv2d_stats_store", *args, int(store_n), ws_t.data_ptr(), nbytes,
                      _stream(x))
    return out, mean, std


# ---- opt-in bf16 inference: the 3x3 conv on the bf16 MFMA (rpst_conv2d_bf16) --------------
def conv2d_bf16_supports(cout: int, cin: int, ksize: int = 3, pad: int = PAD_ZERO,
                         in_op: int = IN_NONE) -> bool:
    """True when a plan lowered with precision="bf16" sends this conv to conv2d_bf16
    (rpst_conv2d_bf16_supports: host only)."""
    return bool(_lib.load().rpst_conv2d_bf16_supports(cout, cin, ksize, pad, in_op))


def pack_conv_weight_bf16(weight: torch.Tensor) -> torch.Tensor:
    """(Cout,Cin,3,3) fp32 weights rounded once to bf16 (nearest even) in conv2d_bf16's layout
    [Cin/16][9][Cout_pad][16]: a flat bfloat16 tensor (rpst_conv2d_bf16_pack)."""
    _check(weight)
    weight = _c(weight.detach())
    cout, cin, kh, kw = weight.shape
    nbytes = _lib.load().rpst_conv2d_bf16_packed_size(cout, cin) if kh == kw == 3 else 0
    if not nbytes:
        raise ValueError(f"rpst: conv2d_bf16 has no kernel for {tuple(weight.shape)} weights "
                         "(3x3, Cin a multiple of 16 in [16, 256], Cout >= 16)")
    packed = torch.empty(nbytes // 2, device=weight.device, dtype=torch.bfloat16)
    _lib.call("rpst_conv2d_bf16_pack", weight.data_ptr(), packed.data_ptr(), cout, cin,
              _stream(weight))
    return packed


def conv2d_bf16(x: torch.Tensor, packed: torch.Tensor, bias: Optional[torch.Tensor], cout: int,
                pad: int = PAD_ZERO, in_op: int = IN_NONE, relu=False,
                aux: Optional[torch.Tensor] = None, x2: Optional[torch.Tensor] = None,
                stats: bool = False, eps: float = 1e-5, store_n: Optional[int] = None):
    """act(conv3x3(in_op(x)) + bias) with bf16 operands and fp32 accumulation
    (rpst_conv2d_bf16): x and the result are fp32; x (after the AdaIN affine under IN_ADAIN,
    aux = adain_params(...)) and the weights are each rounded once to bf16. packed:
    pack_conv_weight_bf16(weight). x2: the conv runs over cat([x, x2]) read in place. stats:
    also calc_mean_std of the output from the epilogue -> (out, mean, std); store_n as
    conv2d_stats. A layer the kernel does not run raises (no fp32 fallback)."""
    x, (n, cin, h, w) = _conv_in(x, x2, bias, aux)
    _check(packed, dtype=torch.bfloat16)
    n1 = n
    if x2 is not None:
        assert x2.dim() == 4 and tuple(x2.shape[1:]) == (cin, h, w)
        x2 = _c(x2)
        n += x2.shape[0]
    if aux is not None:
        aux = _c(aux)
        assert aux.numel() == 4 * n * cin, "ADAIN aux = [mean_c|mean_s|std_c|std_s]"
    if store_n is not None and not stats:
        raise ValueError("rpst: conv2d_bf16's store_n goes with stats=True")
    out = _conv_out(x, (n, cout, h, w))
    mean = std = ws_t = None
    nbytes = 0
    if stats:
        mean = torch.empty((n, cout, 1, 1), device=x.device, dtype=torch.float32)
        std = torch.empty_like(mean)
        ws_t, nbytes = _lib.workspace("conv2d_bf16", x, n, cin, h, w, cout)
    moved = x.numel() + (0 if x2 is None else x2.numel()) + out.numel()
    with _conv_traced((n, cin, h, w), cout, 3, in_op, moved,
                      f"bf16conv3x3 {cin}->{cout} {h}x{w} N{n} op{in_op}"):
        _lib.call("rpst_conv2d_bf16", x.data_ptr(), _ptr(x2), n1, _ptr(aux), packed.data_ptr(),
                  _bias_ptr(bias), out.data_ptr(), n, cin, h, w, cout, pad, in_op, _act(relu),
                  _ptr(mean), _ptr(std), eps, n if store_n is None else int(store_n),
                  _ptr(ws_t), nbytes, _stream(x))
    return (out, mean, std) if stats else out


def se_gate(mean_h2: torch.Tensor, w3: torch.Tensor, b3: torch.Tensor, fc_a: torch.Tensor,
            fc_b: torch.Tensor) -> torch.Tensor:
    """SE gate (network/attention.py:17-22 on conv3's pooled output): mean_h2 (N, C[, 1, 1]),
    w3 (C, C) / b3 (C) = conv3 with bn3 folded, fc_a (R, C), fc_b (C, R) ->
    sigmoid(fc_b relu(fc_a (w3 mean_h2 + b3))) of shape (N, C) (rpst_se_gate)."""
    _check(mean_h2, w3, b3, fc_a, fc_b)
    n, c = mean_h2.shape[:2]
    if mean_h2.numel() != n * c:
        raise ValueError(f"rpst: mean_h2 must be (N, C) or (N, C, 1, 1), got {tuple(mean_h2.shape)}")
    r = fc_a.shape[0]
    if tuple(w3.shape) != (c, c) or tuple(b3.shape) != (c,) or tuple(fc_a.shape) != (r, c) \
            or tuple(fc_b.shape) != (c, r):
        raise ValueError("rpst: se_gate needs w3 (C, C), b3 (C), fc_a (R, C), fc_b (C, R)")
    mean_h2, w3, b3, fc_a, fc_b = (_c(t.detach()) for t in (mean_h2, w3, b3, fc_a, fc_b))
    gate = torch.empty((n, c), device=mean_h2.device, dtype=torch.float32)
    with _traced(f"se_gate C{c} R{r} N{n}", 0.0, 0.0):
        _lib.call("rpst_se_gate", mean_h2.data_ptr(), w3.data_ptr(), b3.data_ptr(),
                  fc_a.data_ptr(), fc_b.data_ptr(), gate.data_ptr(), n, c, r, _stream(mean_h2))
    return gate


def conv2d_gated(x: torch.Tensor, packed: torch.Tensor, bias: Optional[torch.Tensor],
                 gate: torch.Tensor, residual: torch.Tensor, cout: int, ksize: int = 1,
                 stats: bool = False, eps: float = 1e-5):
    """out = relu(gate[n, co] * (conv_k(x) + bias) + residual) (rpst_conv2d_gated, the tail of
    an SE block); stats: also calc_mean_std of out -> (out, mean, std)."""
    x, (n, cin, h, w) = _conv_in(x, packed, bias, gate, residual)
    gate, residual = _c(gate), _c(residual)
    if gate.numel() != n * cout or gate.shape[0] != n:
        raise ValueError(f"rpst: gate must be (N, Cout), got {tuple(gate.shape)}")
    if tuple(residual.shape) != (n, cout, h, w):
        raise ValueError("rpst: residual must have the output's shape")
    out = _conv_out(x, (n, cout, h, w))
    mean = std = None
    nbytes = 0
    if stats:
        mean = torch.empty((n, cout, 1, 1), device=x.device, dtype=torch.float32)
        std = torch.empty_like(mean)
        nbytes = _lib.workspace_bytes("conv2d_gated", n, cin, h, w, cout, ksize)
    ws_t = _lib.scratch(nbytes, x) if nbytes else None
    with _conv_traced(x.shape, cout, ksize, IN_NONE, x.numel() + 2 * out.numel(),
                      f"gated{ksize}x{ksize} {cin}->{cout} {h}x{w} N{n}"):
        _lib.call("rpst_conv2d_gated", x.data_ptr(), packed.data_ptr(), _bias_ptr(bias),
                  gate.data_ptr(), residual.data_ptr(), out.data_ptr(), n, cin, h, w, cout,
                  ksize, _ptr(mean), _ptr(std), eps, _ptr(ws_t), nbytes, _stream(x))
    return (out, mean, std) if stats else out


def se_bottleneck(x: torch.Tensor, block, stats: bool = False):
    """An SEBottleneck (network/attention.py:25-66) in eval mode on x (N, C, H, W): conv1
    (1x1, ReLU), conv2 (3x3 zero pad, ReLU, with the statistics epilogue for its mean), the
    gate, the gated conv3 with residual x -> (out, gate (N, C, 1, 1)), or with stats (out,
    gate, mean, std) where mean / std = calc_mean_std(out). The BatchNorms are folded from
    their running statistics (rpst.plan.se_folded)."""
    from . import plan
    assert x.dim() == 4
    _check(x)
    x = _c(x)
    c = x.shape[1]
    (p1, b1), (p2, b2), (p3, b3), w3 = plan.se_folded(block)
    h1 = conv2d(x, p1, b1, c, 1, relu=True)
    h2, mean_h2, _ = conv2d_stats(h1, p2, b2, c, 3, pad=PAD_ZERO, relu=True)
    gate = se_gate(mean_h2, w3, b3, block.se.fc[0].weight, block.se.fc[2].weight)
    res = conv2d_gated(h2, p3, b3, gate, x, c, 1, stats=stats)
    gate4 = gate.view(gate.shape[0], c, 1, 1)
    return (res[0], gate4, res[1], res[2]) if stats else (res, gate4)


def adain_params(mean_c, std_c, mean_s, std_s) -> torch.Tensor:
    """aux vector of RPST_IN_ADAIN: [mean_c | mean_s | std_c | std_s] (N*C each)."""
    return torch.cat([mean_c.reshape(-1), mean_s.reshape(-1), std_c.reshape(-1),
                      std_s.reshape(-1)])


# ---- LDMSAdaINRPNet4: nearest resize of the coarse pyramid, its statistics, the concat ----
def nearest_index_table(size_in: int, size_out: int) -> torch.Tensor:
    """F.interpolate's default-mode source index of every destination index along one axis:
    int32 (size_out,) on the host, min(floor(dst * (float32(in) / float32(out))), in - 1) as
    the kernels compute it (rpst_nearest_index_table: the same statement of the rule)."""
    import ctypes
    size_in, size_out = int(size_in), int(size_out)
    buf = (ctypes.c_int * max(size_out, 1))()
    _lib.call("rpst_nearest_index_table", size_in, size_out, ctypes.addressof(buf))
    return torch.tensor(list(buf[:size_out]), dtype=torch.int32)


def nearest_counts(size_in: int, size_out: int) -> torch.Tensor:
    """Replication count of every source index under nearest_index_table: int64 (size_in,)."""
    return torch.bincount(nearest_index_table(size_in, size_out).long(), minlength=int(size_in))


def _resize_args(src: torch.Tensor, size):
    assert src.dim() == 4
    H, W = (int(v) for v in size)
    n, c, h, w = src.shape
    if h > H or w > W:
        raise ValueError(f"rpst: nearest resize enlarges only ({h}x{w} -> {H}x{W})")
    return n, c, h, w, H, W


def resize_nearest(src: torch.Tensor, size, out: Optional[torch.Tensor] = None,
                   out_channel_offset: int = 0) -> torch.Tensor:
    """F.interpolate(src, size) (default mode 'nearest', adain_rp.py:813-815) written to channels
    [out_channel_offset, out_channel_offset + C) of `out` (a contiguous (N, C_total, H, W)
    tensor whose other channels are left alone; default: a new (N, C, H, W) tensor). A pure
    gather: bit-identical to torch's. Returns `out`."""
    _check(src, out)
    n, c, h, w, H, W = _resize_args(src, size)
    src = _c(src)
    if out is None and out_channel_offset:
        raise ValueError("rpst: resize_nearest with a channel offset needs the tensor to write "
                         "into")
    out = _conv_out(src, (n, c if out is None else None, H, W), out)
    with _traced(f"resize_nearest C{c} {h}x{w}->{H}x{W} N{n}", 0.0,
                 4.0 * n * c * (h * w + H * W)):
        _lib.call("rpst_resize_nearest", src.data_ptr(), out.data_ptr(), n, c, h, w, H, W,
                  int(out_channel_offset), out.shape[1], _stream(src))
    return out


def resized_mean_std(src: torch.Tensor, size,
                     eps: float = 1e-5) -> Tuple[torch.Tensor, torch.Tensor]:
    """calc_mean_std(F.interpolate(src, size)) from src alone (the resize is not written): every
    source pixel weighted by its replication count -> mean, std of shape (N, C, 1, 1)."""
    _check(src)
    n, c, h, w, H, W = _resize_args(src, size)
    src = _c(src)
    mean = torch.empty((n, c, 1, 1), device=src.device, dtype=torch.float32)
    std = torch.empty_like(mean)
    ws, nbytes = _lib.workspace("resized_mean_std", src, h, w)
    with _traced(f"resized_mean_std C{c} {h}x{w}->{H}x{W} N{n}", 0.0, 4.0 * n * c * h * w):
        _lib.call("rpst_resized_mean_std", src.data_ptr(), mean.data_ptr(), std.data_ptr(), n, c,
                  h, w, H, W, eps, ws.data_ptr(), nbytes, _stream(src))
    return mean, std


def ld4_fuse(y: Optional[torch.Tensor], fine: torch.Tensor, coarse: torch.Tensor,
             params_fine: torch.Tensor, params_coarse: torch.Tensor, n: Optional[int] = None,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A decoder block's input of LDMSAdaINRPNet4.decode (adain_rp.py:786-798) in one pass:
    cat([y, AdaIN(cat([fine, F.interpolate(coarse, (H, W))]), style)], dim=1) of shape
    (n, Ca + 2h, H, W). y (n, Ca, H, W) or None (the first block); fine (>= n, h, H, W) and
    coarse (>= n, h, hc, wc) are read at their first n images, so a [content; style] batch is
    passed whole (n defaults to y's batch, else fine's); params_fine / params_coarse =
    adain_params(mean_c, std_c, mean_s, std_s) of the two halves, n * h each."""
    assert fine.dim() == 4 and coarse.dim() == 4
    _check(y, fine, coarse, params_fine, params_coarse, out)
    fine, coarse = _c(fine), _c(coarse)
    params_fine, params_coarse = _c(params_fine), _c(params_coarse)
    if n is None:
        n = fine.shape[0] if y is None else y.shape[0]
    n = int(n)
    hd, H, W = fine.shape[1:]
    hc, wc = coarse.shape[2:]
    ca = 0
    if y is not None:
        y = _c(y)
        ca = y.shape[1]
        if y.dim() != 4 or (y.shape[0], y.shape[2], y.shape[3]) != (n, H, W) or ca == 0:
            raise ValueError(f"rpst: ld4_fuse's y must be ({n}, Ca > 0, {H}, {W}), got "
                             f"{tuple(y.shape)}")
    if n < 1 or fine.shape[0] < n or coarse.shape[0] < n or coarse.shape[1] != hd:
        raise ValueError("rpst: ld4_fuse needs fine (>= n, h, H, W) and coarse (>= n, h, hc, wc), "
                         f"got {tuple(fine.shape)} and {tuple(coarse.shape)} for n = {n}")
    if hc > H or wc > W:
        raise ValueError(f"rpst: nearest resize enlarges only ({hc}x{wc} -> {H}x{W})")
    if params_fine.numel() != 4 * n * hd or params_coarse.numel() != 4 * n * hd:
        raise ValueError("rpst: ld4_fuse params = [mean_c | mean_s | std_c | std_s], n * h each")
    out = _conv_out(fine, (n, ca + 2 * hd, H, W), out)
    with _traced(f"ld4_fuse {ca}+2x{hd} {hc}x{wc}->{H}x{W} N{n}", 0.0,
                 4.0 * n * ((2 * ca + 3 * hd) * H * W + hd * hc * wc)):
        _lib.call("rpst_ld4_fuse", _ptr(y), fine.data_ptr(), coarse.data_ptr(),
                  params_fine.data_ptr(), params_coarse.data_ptr(), out.data_ptr(), n, ca, hd, H,
                  W, hc, wc, _stream(fine))
    return out


def maxpool2x2_ceil(x: torch.Tensor) -> torch.Tensor:
    _check(x)
    x = _c(x)
    n, c, h, w = x.shape
    out = torch.empty((n, c, (h + 1) // 2, (w + 1) // 2), device=x.device, dtype=x.dtype)
    _lib.call("rpst_maxpool2x2_ceil", x.data_ptr(), out.data_ptr(), n, c, h, w, _stream(x))
    return out


def upsample_nearest2x(x: torch.Tensor) -> torch.Tensor:
    _check(x)
    x = _c(x)
    n, c, h, w = x.shape
    out = torch.empty((n, c, 2 * h, 2 * w), device=x.device, dtype=x.dtype)
    _lib.call("rpst_upsample_nearest2x", x.data_ptr(), out.data_ptr(), n, c, h, w, _stream(x))
    return out


def add_upsample_nearest2x(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a + upsample_nearest2x(b) (the merge conv's input, sanet.py:147-149)."""
    _check(a, b)
    a, b = _c(a), _c(b)
    n, c, h, w = a.shape
    assert tuple(b.shape) == (n, c, h // 2, w // 2) and h % 2 == 0 and w % 2 == 0
    out = torch.empty_like(a)
    _lib.call("rpst_add_upsample_nearest2x", a.data_ptr(), b.data_ptr(), out.data_ptr(), n, c,
              h, w, _stream(a))
    return out


def conv_algorithm(cout: int, cin: int, hs: int, ws: int, ksize: int, in_op: int) -> int:
    """The library's algorithm choice for a conv (0 direct, 1 F(2x2), 2 F(4x4), 3 narrow)."""
    return int(_lib.load().rpst_conv2d_algorithm(cout, cin, hs, ws, ksize, in_op))


# Cap on the materialised attention matrix per launch; larger batches are chunked.
SANET_WS_CAP = 8 << 30


def _pair_shapes(what: str, content: torch.Tensor, style: torch.Tensor) -> None:
    """content (n, C, h, w) and style (n, C, h', w'): the batch and the channels are shared,
    the spatial size is each one's own. ValueError names both shapes."""
    if content.dim() != 4 or style.dim() != 4 or content.shape[:2] != style.shape[:2]:
        raise ValueError(f"rpst: {what}: content {tuple(content.shape)} and style "
                         f"{tuple(style.shape)} must be 4-d and share their batch and channels "
                         "(only the spatial size may differ)")


def sanet_attention(F: torch.Tensor, G: torch.Tensor, H: torch.Tensor) -> torch.Tensor:
    """SANet core (sanet.py:86-94): O = H softmax(F^T G)^T per image. F (B,C,h,w) comes from
    the content, G and H (B,C,h',w') from the style, whose size may differ; O is F-shaped."""
    if G.shape != H.shape:
        raise ValueError(f"rpst: sanet_attention: G {tuple(G.shape)} and H {tuple(H.shape)} "
                         "must have one shape")
    _pair_shapes("sanet_attention", F, G)
    _check(F, G, H)
    F, G, H = _c(F), _c(G), _c(H)
    B, C, h, w = F.shape
    hw, hwk = h * w, G.shape[2] * G.shape[3]
    out = torch.empty_like(F)
    lib = _lib.load()
    # flash path (S never written): no workspace, the whole batch in one launch
    per_img = lib.rpst_sanet_attention_qk_workspace_size_c(1, C, hw, hwk)
    chunk = B if per_img == 0 else max(1, min(B, SANET_WS_CAP // per_img))
    ws_bytes = lib.rpst_sanet_attention_qk_workspace_size_c(chunk, C, hw, hwk)
    ws = _lib.scratch(ws_bytes, F)
    name = f"HW{hw}" if hw == hwk else f"HW{hw}x{hwk}"
    for b0 in range(0, B, chunk):
        nb = min(chunk, B - b0)
        with _traced(f"sanet_attention C{C} {name} N{nb}", 4.0 * nb * hw * hwk * C, 0.0):
            _lib.call("rpst_sanet_attention_qk", F[b0].data_ptr(), G[b0].data_ptr(),
                      H[b0].data_ptr(), out[b0].data_ptr(), nb, C, hw, hwk, ws.data_ptr(),
                      ws_bytes, _stream(F))
    return out


def cosine_affinity(content: torch.Tensor, style: torch.Tensor) -> torch.Tensor:
    """cal_affinity_matrix (sanet.py:12-18): normalize(c)^T normalize(s), (B, HW, HW)."""
    assert content.size() == style.size() and content.dim() == 4
    _check(content, style)
    content, style = _c(content), _c(style)
    B, C, h, w = content.shape
    hw = h * w
    out = torch.empty((B, hw, hw), device=content.device, dtype=torch.float32)
    ws, nbytes = _lib.workspace("cosine_affinity", content, B, C, hw)
    _lib.call("rpst_cosine_affinity", content.data_ptr(), style.data_ptr(), out.data_ptr(), B, C,
              hw, ws.data_ptr(), nbytes, _stream(content))
    return out


AEA_MODES = {"aea": 0, "relu": 1}


def _mlp_params(f_psi):
    """(W1, b1, w2, b2, hidden) of f_psi = Sequential(Linear, LeakyReLU, Linear, head)."""
    l1, l2 = f_psi[0], f_psi[2]
    ps = [l1.weight, l1.bias, l2.weight, l2.bias]
    _check(*ps)
    return [_c(p.detach()) for p in ps] + [l1.out_features]


def aea_clamp(x: torch.Tensor, f_x: torch.Tensor, f_psi, mode: int, scale: float,
              from_value: float, interval: float):
    """AEAModule / AEALReluModule.forward (sanet.py:42-47 / 63-69):
    returns (clamp_fx (B, HW, HW), clamp_value (B, HW, 1))."""
    assert x.dim() == 3 and x.shape == f_x.shape and x.shape[1] == x.shape[2]
    _check(x, f_x)
    x, f_x = _c(x), _c(f_x)
    B, hw = x.shape[0], x.shape[1]
    w1, b1, w2, b2, hid = _mlp_params(f_psi)
    assert w1.shape[1] == hw, "f_psi input width must equal HW (spatial_dims)"
    out = torch.empty_like(f_x)
    clamp = torch.empty((B, hw, 1), device=x.device, dtype=torch.float32)
    ws, nbytes = _lib.workspace("aea_clamp", x, B, hw, hid)
    _lib.call("rpst_aea_clamp", x.data_ptr(), f_x.data_ptr(), w1.data_ptr(), b1.data_ptr(),
              w2.data_ptr(), b2.data_ptr(), hid, mode, scale, from_value, interval,
              out.data_ptr(), clamp.data_ptr(), B, hw, ws.data_ptr(), nbytes, _stream(x))
    return out, clamp


def adaptive_attention(F: torch.Tensor, G: torch.Tensor, H: torch.Tensor,
                       content: torch.Tensor, style: torch.Tensor, f_psi, mode: int,
                       scale: float, from_value: float, interval: float,
                       keep_claims: bool = False):
    """AdaptiveSANet core (sanet.py:106-124): O = H AEA(affinity(c, s), softmax(F^T G))^T.
    Returns (O, claim_value (B, HW, 1), claim_before, claim_after); the (B, HW, HW) claim
    maps are materialised only when keep_claims (else None)."""
    assert F.dim() == 4 and F.shape == G.shape == H.shape == content.shape == style.shape
    _check(F, G, H, content, style)
    F, G, H, content, style = _c(F), _c(G), _c(H), _c(content), _c(style)
    B, C, h, w = F.shape
    hw = h * w
    w1, b1, w2, b2, hid = _mlp_params(f_psi)
    assert w1.shape[1] == hw, "f_psi input width must equal HW (spatial_dims)"
    out = torch.empty_like(F)
    claim = torch.empty((B, hw, 1), device=F.device, dtype=torch.float32)
    before = after = None
    if keep_claims:
        before = torch.empty((B, hw, hw), device=F.device, dtype=torch.float32)
        after = torch.empty_like(before)
    lib = _lib.load()
    per_img = lib.rpst_adaptive_attention_workspace_size(1, C, hw, hid)
    chunk = max(1, min(B, SANET_WS_CAP // max(per_img, 1)))
    ws, ws_bytes = _lib.workspace("adaptive_attention", F, chunk, C, hw, hid)
    for b0 in range(0, B, chunk):
        nb = min(chunk, B - b0)
        # S = F^T G and O = H Q^T (4 HW^2 C) + f_psi's first Linear without the affinity:
        # T = sn W1^T, Z = cn^T T (4 C hid HW); DESIGN.md §1 f3
        flops = nb * (4.0 * hw * hw * C + 4.0 * C * hid * hw)
        with _traced(f"adaptive_attention C{C} HW{hw} N{nb}", flops, 0.0):
            _lib.call("rpst_adaptive_attention", F[b0].data_ptr(), G[b0].data_ptr(),
                      H[b0].data_ptr(), content[b0].data_ptr(), style[b0].data_ptr(),
                      w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), hid, mode,
                      scale, from_value, interval, out[b0].data_ptr(), claim[b0].data_ptr(),
                      before[b0].data_ptr() if keep_claims else None,
                      after[b0].data_ptr() if keep_claims else None, nb, C, hw,
                      ws.data_ptr(), ws_bytes, _stream(F))
    return out, claim, before, after


def matrix_power_psd(A: torch.Tensor, p: float) -> torch.Tensor:
    """The reference's matrix_sqrt (p = 1/2) / matrix_inv_sqrt (p = -1/2) of fp64 (n,n) or
    (b,n,n) matrices (wct_rp.py:7-40): V diag(s^p) V^T of the SVD of A + 1e-4 I, truncated at
    s < 1e-5. Symmetric inputs whose smallest eigenvalue is provably >= 1e-5 take the
    Newton-Schulz launch (= A^p there); every other input (indefinite, non-symmetric, or
    near the truncation) takes the on-device one-sided Jacobi SVD. No host synchronisation."""
    assert p in (0.5, -0.5)
    _check(A, dtype=torch.float64)
    A = _c(A)
    n = A.shape[-1]
    assert A.shape[-2] == n
    batch = A.numel() // (n * n)
    out = torch.empty_like(A)
    res = torch.empty(batch, device=A.device, dtype=torch.float64)
    ws, nbytes = _lib.workspace("matrix_power", A, n, batch)
    _lib.call("rpst_matrix_power_psd_f64", A.data_ptr(), out.data_ptr(), n, batch,
              int(p < 0), res.data_ptr(), ws.data_ptr(), nbytes, _stream(A))
    return out


def whiten_and_color(cF: torch.Tensor, sF: torch.Tensor, method: str = 'closed-form',
                     status: bool = False):
    """WCTRPNet.whiten_and_color (wct_rp.py:82-114): (C,HW) fp64 -> fp64. method
    'closed-form' (Lu et al., :102-111) or 'original' (Li et al., :96-101: matrix_sqrt(Cs)
    matrix_inv_sqrt(Cc) in the reference's SVD form). status=True also returns the (1,)
    int32 device status word: rpst_whiten_and_color_status for 'closed-form'; for 'original'
    (whose Jacobi fallback recomputes any matrix Newton-Schulz could not take) RPST_WCT_NOCONV
    when the output is not finite (a device-side test, no host sync)."""
    assert cF.dim() == 2 and cF.shape == sF.shape
    assert method in ('closed-form', 'original'), method
    _check(cF, sF, dtype=torch.float64)
    cF, sF = _c(cF), _c(sF)
    C, hw = cF.shape
    out = torch.empty_like(cF)
    ws, nbytes = _lib.workspace("wct", cF, 1, C, hw)
    if method == 'original':
        _lib.call("rpst_whiten_and_color_original_f64", cF.data_ptr(), sF.data_ptr(),
                  out.data_ptr(), C, hw, ws.data_ptr(), nbytes, _stream(cF))
    else:
        res = torch.empty(2, device=cF.device, dtype=torch.float64)
        _lib.call("rpst_whiten_and_color_f64", cF.data_ptr(), sF.data_ptr(), out.data_ptr(), C,
                  hw, res.data_ptr(), ws.data_ptr(), nbytes, _stream(cF))
    if not status:
        return out
    st = torch.empty(1, device=cF.device, dtype=torch.int32)
    if method == 'original':
        st.copy_((~torch.isfinite(out)).any().reshape(1).to(torch.int32) * WCT_NOCONV)
    else:
        _lib.call("rpst_whiten_and_color_status", ws.data_ptr(), C, hw, st.data_ptr(),
                  _stream(cF))
    return out, st


def check_wct_status(status: torch.Tensor, what: str = "wct") -> None:
    """Host check of a WCT status vector (synchronises on it): raises RuntimeError naming
    the images whose matrices did not converge or whose persistent launch timed out (their
    outputs are NaN, never silently wrong). For callers that want failures surfaced (tests,
    train.py with RPST_WCT_CHECK=1); the inference path itself never synchronises."""
    st = status.cpu()
    bad = torch.nonzero(st).flatten().tolist()
    if bad:
        why = {i: "+".join(w for f, w in ((WCT_TIMEOUT, "timeout"), (WCT_NOCONV, "no-convergence"))
                           if int(st[i]) & f) for i in bad}
        raise RuntimeError(f"{what}: invalid WCT matrices for images {why} (outputs are NaN)")


class WCTStatusWatch:
    """Deferred check of the WCT status words without a host sync per call (the
    C side returns status codes and Python raises, no silent fallback). push() copies a call's
    device status to pinned host memory behind an event on the launch stream, then checks the
    PREVIOUS call's: that call's kernels were enqueued a whole call earlier, so the wait is
    normally already over, and the GPU has this call's work queued meanwhile -- a failed image
    raises RuntimeError at the latest during the following call. check() waits for and checks
    the last pushed call (end of a run, tests)."""

    def __init__(self):
        self._pending = None

    def push(self, status: torch.Tensor, what: str) -> None:
        host = torch.empty(status.shape, dtype=status.dtype, pin_memory=True)
        host.copy_(status, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(status.device))
        prev, self._pending = self._pending, (host, ev, what)
        if prev is not None:
            self._check(prev)

    def check(self) -> None:
        prev, self._pending = self._pending, None
        if prev is not None:
            self._check(prev)

    @staticmethod
    def _check(p) -> None:
        host, ev, what = p
        ev.synchronize()
        check_wct_status(host, what)


def _wct_status(ws: torch.Tensor, n: int, C: int, hwc: int, hws: int, dev) -> torch.Tensor:
    st = torch.empty(n, device=dev, dtype=torch.int32)
    _lib.call("rpst_wct_status_cs", ws.data_ptr(), n, C, hwc, hws, st.data_ptr(), _stream(st))
    return st


def _px(hwc: int, hws: int) -> str:  # trace name of a WCT launch's pixel counts
    return f"{hwc}px" if hwc == hws else f"{hwc}x{hws}px"


def wct_fuse(content: torch.Tensor, style: torch.Tensor, status: bool = False):
    """WCTRPNet.fuse (wct_rp.py:157-166): content (n,C,h,w), style (n,C,h',w') fp32 -> fp32 of
    the content's shape, fp64 internals; the style may have another size (each side is
    flattened on its own). The matrix functions iterate on the device (no host
    synchronisation); an image whose Newton-Schulz iteration cannot converge (non-finite
    features) or whose persistent launch timed out comes out NaN. status=True also returns the
    (n,) int32 per-image status (rpst_wct_status)."""
    _pair_shapes("wct_fuse", content, style)
    _check(content, style)
    content, style = _c(content), _c(style)
    n, C, h, w = content.shape
    hwc, hws = h * w, style.shape[2] * style.shape[3]
    out = torch.empty_like(content)
    res = torch.empty(2 * n, device=content.device, dtype=torch.float64)
    nbytes = _lib.load().rpst_wct_workspace_size_cs(n, C, hwc, hws)
    ws = _lib.scratch(nbytes, content)
    with _traced(f"wct_fuse C{C} {_px(hwc, hws)} N{n}", 2.0 * n * C * C * (2 * hwc + hws), 0.0):
        _lib.call("rpst_wct_fuse_cs", content.data_ptr(), style.data_ptr(), out.data_ptr(), n, C,
                  hwc, hws, res.data_ptr(), ws.data_ptr(), nbytes, _stream(content))
    if status:
        return out, _wct_status(ws, n, C, hwc, hws, content.device)
    return out


def wct_params(content: torch.Tensor, style: torch.Tensor, means: Optional[torch.Tensor] = None,
               status: bool = False):
    """The closed-form WCT matrices of every image without the product (wct_rp.py:85-109):
    returns (T (n,C,C) fp64, offset c = mu_s - T mu_c (n,C) fp64, residual (2n,) fp64), plus
    the (n,) int32 status with status=True (rpst_wct_status: 0 valid; NaN T / c otherwise).
    content (n,C,h,w) and style (n,C,h',w') share n and C only.
    means: optional (2n, C) fp32 row means, content rows first (the encoder epilogue's)."""
    _pair_shapes("wct_params", content, style)
    _check(content, style, means)
    content, style = _c(content), _c(style)
    n, C, h, w = content.shape
    hwc, hws = h * w, style.shape[2] * style.shape[3]
    if means is not None:
        means = _c(means)
        if means.numel() != 2 * n * C:
            raise ValueError(f"rpst: wct_params: means {tuple(means.shape)} is not (2n, C) = "
                             f"({2 * n}, {C})")
    T = torch.empty((n, C, C), device=content.device, dtype=torch.float64)
    c = torch.empty((n, C), device=content.device, dtype=torch.float64)
    res = torch.empty(2 * n, device=content.device, dtype=torch.float64)
    nbytes = _lib.load().rpst_wct_workspace_size_cs(n, C, hwc, hws)
    ws = _lib.scratch(nbytes, content)
    with _traced(f"wct_params C{C} {_px(hwc, hws)} N{n}", n * C * (C + 1) * (hwc + hws) * 1.0,
                 0.0):
        _lib.call("rpst_wct_params_cs", content.data_ptr(), style.data_ptr(), _ptr(means),
                  T.data_ptr(), c.data_ptr(), n, C, hwc, hws, res.data_ptr(), ws.data_ptr(),
                  nbytes, _stream(content))
    if status:
        return T, c, res, _wct_status(ws, n, C, hwc, hws, content.device)
    return T, c, res


def conv2d_mix(x: torch.Tensor, T: torch.Tensor, offset: torch.Tensor, packed: torch.Tensor,
               bias: Optional[torch.Tensor], cout: int, ksize: int, pad: int = PAD_ZERO,
               relu=False) -> torch.Tensor:
    """out = act(conv(pad(T_n x + c_n)) + bias) per image (include/rpst.h rpst_conv2d_mix):
    the WCT colour transform (wct_rp.py:109-113) applied inside the consumer conv."""
    x, (n, cin, h, w) = _conv_in(x, packed, bias)
    _check(T, offset, dtype=torch.float64)
    T, offset = _c(T), _c(offset)
    assert tuple(T.shape) == (n, cin, cin) and tuple(offset.shape) == (n, cin)
    out = _conv_out(x, (n, cout, h, w))
    ws, nbytes = _lib.workspace("conv2d_mix", x, n, cin, h, w, cout, ksize)
    with _conv_traced(x.shape, cout, ksize, IN_NONE, x.numel() + out.numel(),
                      _conv_name(ksize, cin, cout, h, w, n, IN_NONE).replace(" op0", " mix")):
        _lib.call("rpst_conv2d_mix", x.data_ptr(), T.data_ptr(), offset.data_ptr(),
                  packed.data_ptr(), _bias_ptr(bias), out.data_ptr(), n, cin, h, w, cout, ksize,
                  pad, _act(relu), ws.data_ptr(), nbytes, _stream(x))
    return out
