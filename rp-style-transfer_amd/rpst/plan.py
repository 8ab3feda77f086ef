"""Compile an nn.Sequential conv stack into fused rpst conv launches and run it.

The reference builds its stacks from plain layers (network/base.py:25-111,363-396,
sanet.py:162-192) and Conv2dBlocks (base.py:114-198): [MaxPool2d | Upsample] ->
[ReflectionPad2d | ZeroPad2d] -> Conv2d -> [ReLU | LeakyReLU(0.2)].
Convs are 1x1, 3x3 (pad 1) or 7x7 (pad 3: LDMSAdaINRPNet's big-receptive-field blocks,
adain_rp.py:513-514, one rpst_conv7 launch, no input operator).
Each such group becomes ONE rpst_conv2d launch: the pool/upsample and the padding are
applied by the conv kernel's tile loader and ReLU by its epilogue, so no intermediate
(padded, pooled or upsampled) tensor is ever written to HBM.

compile_layers / of group the layers into steps; lower() decides on the host which launch each
step becomes (Launch records; no tensor touched, every refusal raised there); run() performs
that list; conv() is the one mapping from a conv module to an ops call, for run() and for
single convs (SANet, rpst.autograd); packed_weight() caches the kernel-layout weights.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Iterable, List, Optional

import torch
import torch.nn as nn

from . import ops


@dataclass
class ConvStep:
    conv: nn.Conv2d
    pad: int
    in_op: int
    relu: int  # ops.ACT_* epilogue activation


@dataclass
class OpStep:
    in_op: int  # stand-alone MAXPOOL2 / UPSAMPLE2 with no conv after it


def _is_pad1(m: nn.Module) -> bool:
    return isinstance(m, (nn.ReflectionPad2d, nn.ZeroPad2d)) and tuple(m.padding) == (1, 1, 1, 1)


def _is_pad3(m: nn.Module) -> bool:
    return isinstance(m, (nn.ReflectionPad2d, nn.ZeroPad2d)) and tuple(m.padding) == (3, 3, 3, 3)


def block_layers(blk: nn.Module) -> List[nn.Module]:
    """The layer sequence of a Conv2dBlock (network/base.py:187-198): pad, conv, the 1x1
    inception convs, activation. Norm variants are rejected at construction by
    network.base.Conv2dBlock; an 'se' attention block runs after this plan
    (ops.se_bottleneck)."""
    layers = [blk.pad, blk.conv]
    if blk.inception is not None:
        layers += [seq[0] for seq in blk.inception]
    if blk.activation is not None:
        layers.append(blk.activation)
    return layers


def compile_layers(layers: Iterable[nn.Module]) -> List[object]:
    steps: List[object] = []
    in_op = ops.IN_NONE
    reflect = False
    zero_pad = False
    pad3 = False  # the pending pad layer is a pad-3 one: only a 7x7 conv may follow
    last_conv: Optional[ConvStep] = None
    for m in layers:
        if isinstance(m, (nn.ReLU, nn.LeakyReLU)):
            if last_conv is None or last_conv.relu:
                raise NotImplementedError("rpst plan: an activation must directly follow a Conv2d")
            if isinstance(m, nn.LeakyReLU) and m.negative_slope != 0.2:
                raise NotImplementedError(f"rpst plan: unsupported {m} (slope 0.2 only)")
            last_conv.relu = ops.ACT_RELU if isinstance(m, nn.ReLU) else ops.ACT_LRELU
            continue
        last_conv = None
        if isinstance(m, nn.MaxPool2d):
            k = m.kernel_size if isinstance(m.kernel_size, tuple) else (m.kernel_size,) * 2
            s = m.stride if isinstance(m.stride, tuple) else (m.stride,) * 2
            p = m.padding if isinstance(m.padding, tuple) else (m.padding,) * 2
            if tuple(k) != (2, 2) or tuple(s) != (2, 2) or tuple(p) != (0, 0) or not m.ceil_mode:
                raise NotImplementedError(f"rpst plan: unsupported {m}")
            if in_op != ops.IN_NONE or reflect:
                raise NotImplementedError("rpst plan: pool after pad/op")
            in_op = ops.IN_MAXPOOL2
        elif isinstance(m, nn.Upsample):
            if m.mode != "nearest" or float(m.scale_factor) != 2.0:
                raise NotImplementedError(f"rpst plan: unsupported {m}")
            if in_op != ops.IN_NONE or reflect:
                raise NotImplementedError("rpst plan: upsample after pad/op")
            in_op = ops.IN_UPSAMPLE2
        elif isinstance(m, (nn.ReflectionPad2d, nn.ZeroPad2d)):
            if not (_is_pad1(m) or _is_pad3(m)) or reflect or zero_pad:
                raise NotImplementedError(f"rpst plan: unsupported {m}")
            pad3 = _is_pad3(m)
            if isinstance(m, nn.ReflectionPad2d):
                reflect = True
            else:
                zero_pad = True
        elif isinstance(m, nn.Conv2d):
            k = tuple(m.kernel_size)
            if (tuple(m.stride) != (1, 1) or tuple(m.dilation) != (1, 1) or m.groups != 1
                    or k not in ((1, 1), (3, 3), (7, 7))):
                raise NotImplementedError(f"rpst plan: unsupported {m}")
            pad_t = tuple(m.padding)
            if pad3 != (k == (7, 7)):
                raise NotImplementedError(f"rpst plan: unsupported padding for {m}")
            if k == (7, 7):
                # ReflectionPad2d(3) / ZeroPad2d(3) + Conv2d(k=7): rpst_conv7, which has no
                # loader operator
                if pad_t != (0, 0) or in_op != ops.IN_NONE:
                    raise NotImplementedError(f"rpst plan: unsupported 7x7 conv {m}")
                pad = ops.PAD_REFLECT if reflect else ops.PAD_ZERO
            elif k == (3, 3):
                if reflect and pad_t == (0, 0):
                    pad = ops.PAD_REFLECT
                elif zero_pad and pad_t == (0, 0):
                    pad = ops.PAD_ZERO
                elif not reflect and not zero_pad and pad_t == (1, 1) and m.padding_mode == "zeros":
                    pad = ops.PAD_ZERO
                else:
                    raise NotImplementedError(f"rpst plan: unsupported padding for {m}")
            else:
                if reflect or zero_pad or pad_t != (0, 0) or in_op != ops.IN_NONE:
                    raise NotImplementedError(f"rpst plan: unsupported 1x1 conv {m}")
                pad = ops.PAD_ZERO
            step = ConvStep(m, pad, in_op, ops.ACT_NONE)
            steps.append(step)
            last_conv = step
            in_op, reflect, zero_pad, pad3 = ops.IN_NONE, False, False, False
        else:
            raise NotImplementedError(f"rpst plan: unsupported layer {type(m).__name__}")
    if reflect or zero_pad:
        raise NotImplementedError("rpst plan: trailing padding layer")
    if in_op != ops.IN_NONE:
        steps.append(OpStep(in_op))
    return steps


def _tensor_key(t: torch.Tensor):
    return (t.device, t.data_ptr(), t._version)


def cached(module: nn.Module, attr: str, key, make):
    """make() (run without grad), kept on the module as `attr` while `key` compares equal. Keys
    hold _tensor_key (device, data_ptr, _version) of every tensor the value derives from, so
    load_state_dict, .to() and in-place updates (optimizer step) refresh the value."""
    hit = getattr(module, attr, None)
    if hit is not None and hit[0] == key:
        return hit[1]
    with torch.no_grad():
        value = make()
    setattr(module, attr, (key, value))
    return value


def packed_weight(conv: nn.Conv2d, flip: bool = False, bf16: bool = False) -> torch.Tensor:
    """conv.weight in its kernel's K-major layout (rpst_conv7's for a 7x7 conv, else the conv /
    Winograd kernels'), cached on the module. flip: of the flip-transposed weights (Cin, Cout,
    k, k) instead, which are the weights of the conv's dgrad. bf16: conv2d_bf16's bf16 image
    instead, cached beside the fp32 one under the same key."""
    def make():
        w = conv.weight.detach()
        if bf16:
            return ops.pack_conv_weight_bf16(w)
        if flip:
            w = ops.conv_weight_flip(w)
        return (ops.pack_conv7_weight if w.shape[2] == 7 else ops.pack_conv_weight)(w)

    if bf16 and flip:
        raise NotImplementedError("rpst plan: no bf16 image of the flip-transposed weights")
    attr = "_rpst_packed_bf16" if bf16 else ("_rpst_flip_packed" if flip else "_rpst_packed")
    return cached(conv, attr, _tensor_key(conv.weight), make)


def fold_batchnorm(conv: nn.Conv2d, bn: nn.BatchNorm2d):
    """Eval-mode BatchNorm folded into the bias-free conv before it: -> (w', b') fp32 with
    w' = w * g and b' = beta - running_mean * g per output channel, g = gamma /
    sqrt(running_var + eps), formed in float64 and rounded once."""
    g = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    w = (conv.weight.detach().double() * g.view(-1, 1, 1, 1)).float().contiguous()
    b = (bn.bias.detach().double() - bn.running_mean.detach().double() * g).float().contiguous()
    return w, b


def se_folded(block: nn.Module):
    """The kernel operands of an SEBottleneck (network/attention.py:25-66) in eval mode:
    [(packed w1', b1'), (packed w2', b2'), (packed w3', b3'), w3' as a (C, C) matrix], every
    BatchNorm folded into its conv. Cached on the module like packed_weight, keyed on the
    device, data_ptr and _version of each conv weight and of its BatchNorm's weight, bias,
    running_mean and running_var, so load_state_dict, .to() and in-place updates refresh it."""
    pairs = ((block.conv1, block.bn1), (block.conv2, block.bn2), (block.conv3, block.bn3))
    key = tuple(_tensor_key(t) for conv, bn in pairs
                for t in (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var))
    key += tuple(bn.eps for _, bn in pairs)

    def fold():
        folded = []
        for conv, bn in pairs:
            if conv.bias is not None or not bn.affine or not bn.track_running_stats:
                raise NotImplementedError("rpst plan: SEBottleneck convs are bias-free and its "
                                          "BatchNorms affine with running statistics")
            w, b = fold_batchnorm(conv, bn)
            folded.append((ops.pack_conv_weight(w), b))
            if conv is block.conv3:
                folded.append(w.view(w.shape[0], w.shape[1]))
        return folded

    return cached(block, "_rpst_se", key, fold)


def of(module: nn.Module) -> List[object]:
    """The compiled steps of a KernelSequential / nn.Sequential (its children) or of a
    Conv2dBlock (block_layers); compiled per call, so a replaced child needs no invalidation."""
    return compile_layers(module.children() if isinstance(module, nn.Sequential)
                          else block_layers(module))


def is_k7(step) -> bool:
    return isinstance(step, ConvStep) and step.conv.kernel_size[0] == 7


def conv(step_or_conv, x: torch.Tensor, *, op: Optional[str] = None, pad=None, in_op=None,
         relu=None, flip: bool = False, **operands) -> torch.Tensor:
    """One conv launch: the only place a conv module is expanded into kernel-call arguments.
    step_or_conv: a ConvStep, or a bare nn.Conv2d (zero pad, no input operator, no activation);
    pad / in_op / relu override the step's. op: the ops wrapper that runs (default conv2d, or
    conv2d_k7 for a 7x7 conv); operands are that wrapper's own (aux, residual, out,
    out_channel_offset, x2, store_n, fold; content for conv2d_skip_adain, mix = (T, c) for
    conv2d_mix). flip: the conv's dgrad instead: flip-transposed weights, no bias. op
    "conv2d_bf16": the bf16 kernel on the bf16 weight image; operands aux / x2, and store_n
    (its presence asks for the statistics epilogue, its value may be None)."""
    s = step_or_conv if isinstance(step_or_conv, ConvStep) else ConvStep(
        step_or_conv, ops.PAD_ZERO, ops.IN_NONE, ops.ACT_NONE)
    c = s.conv
    pad = s.pad if pad is None else pad
    in_op = s.in_op if in_op is None else in_op
    relu = s.relu if relu is None else relu
    if op == "conv2d_bf16":
        return ops.conv2d_bf16(x, packed_weight(c, bf16=True), c.bias, c.out_channels, pad=pad,
                               in_op=in_op, relu=relu, aux=operands.get("aux"),
                               x2=operands.get("x2"), stats="store_n" in operands,
                               store_n=operands.get("store_n"))
    w = (packed_weight(c, flip),) + ((None, c.in_channels) if flip else (c.bias, c.out_channels))
    if c.kernel_size[0] == 7:
        if in_op != ops.IN_NONE or any(operands.get(k) is not None for k in ("aux", "residual")):
            raise NotImplementedError("rpst plan: a 7x7 conv has no input operator / residual")
        return ops.conv2d_k7(x, *w, pad=pad, act=relu, **operands)
    w += (c.kernel_size[0],)
    if op == "conv2d_pair":
        return ops.conv2d_pair(x, operands["x2"], *w, pad=pad, relu=relu)
    if op == "conv2d_mix":
        return ops.conv2d_mix(x, *operands["mix"], *w, pad=pad, relu=relu)
    if op == "conv2d_skip_adain":
        return ops.conv2d_skip_adain(x, operands["content"], operands["aux"], *w, pad=pad,
                                     relu=relu)
    return getattr(ops, op or "conv2d")(x, *w, pad=pad, in_op=in_op, relu=relu, **operands)


PRECISIONS = ("fp32", "bf16")


@dataclass
class Launch:
    """One record of lower()'s launch list."""
    op: str                          # the ops entry that runs; "cat": torch.cat([x, x2])
    step: Optional[ConvStep] = None  # the conv launches' step
    in_op: int = ops.IN_NONE         # the conv's effective input operator
    pooled: bool = False             # the conv's output comes out max-pooled (conv2d_pool)
    takes: tuple = ()                # run()'s operands it reads: aux content mix store_n x2


def lower(steps: List[object], shape, x2_shape=None, *, first_in_op=None,
          first_mix: bool = False, stats_last: bool = False,
          precision: str = "fp32") -> List[Launch]:
    """The launches run() performs for a compiled plan on an input of `shape` (over the batch
    [x; x2] with x2_shape), in order. Host only: no tensor, no device, the library's algorithm
    queries alone. Every refusal of run() is raised here, before any launch.
    precision "bf16": a plain, paired, AdaIN-loading or statistics conv step that
    ops.conv2d_bf16_supports accepts becomes op "conv2d_bf16" with the same operands (takes);
    every other step, and everything under "fp32", lowers as it always has."""
    if precision not in PRECISIONS:
        raise ValueError(f"rpst plan: precision must be one of {PRECISIONS}, got {precision!r}")
    n, cin, h, w = shape
    s0 = steps[0] if steps else None
    if is_k7(s0) and (first_in_op is not None or first_mix):
        raise NotImplementedError("rpst plan: a 7x7 conv has no AdaIN loader / colour mix")
    out: List[Launch] = []
    pair = False
    if x2_shape is not None:
        # a plain first conv reads x and x2 in place (rpst_conv7: two equal halves)
        pair = (isinstance(s0, ConvStep) and s0.in_op == ops.IN_NONE and not first_mix
                and first_in_op is None and not (stats_last and len(steps) == 1)
                and (not is_k7(s0) or tuple(shape) == tuple(x2_shape)))
        n += x2_shape[0]
        if not pair:
            out.append(Launch("cat"))
    if first_mix and not isinstance(s0, ConvStep):
        # the colour transform only fuses into a conv: skipping it would decode raw features
        raise NotImplementedError("rpst plan: first_mix needs a conv as the plan's first step")
    if first_in_op is not None and not isinstance(s0, ConvStep):
        raise NotImplementedError("rpst plan: first_in_op needs a conv as the plan's first step")
    for i, s in enumerate(steps):
        if not isinstance(s, ConvStep):
            pool = s.in_op == ops.IN_MAXPOOL2
            out.append(Launch("maxpool2x2_ceil" if pool else "upsample_nearest2x"))
            h, w = ops.conv_out_hw(h, w, s.in_op)
            continue
        cout, k = s.conv.out_channels, s.conv.kernel_size[0]
        last = stats_last and i == len(steps) - 1
        nxt = steps[i + 1] if i + 1 < len(steps) else None
        pooled_in = bool(out) and out[-1].pooled  # the conv before wrote its output pooled
        rec = Launch("conv2d_k7" if k == 7 else "conv2d", s, s.in_op)
        if i == 0 and pair:
            rec.op, rec.takes = rec.op if k == 7 else "conv2d_pair", ("x2",)
        elif i == 0 and first_mix:
            if s.in_op != ops.IN_NONE or last:
                raise NotImplementedError("rpst plan: mixed first conv with an input op / stats")
            rec.op, rec.takes = "conv2d_mix", ("mix",)
        elif k != 7:  # (a 7x7 conv has no statistics epilogue: calc_mean_std below)
            if i == 0 and first_in_op is not None:
                if s.in_op != ops.IN_NONE:
                    raise NotImplementedError("rpst plan: first conv already has an input op")
                rec.in_op, rec.takes = first_in_op, ("aux",)
            if rec.in_op == ops.IN_MAXPOOL2 and pooled_in:
                rec.in_op = ops.IN_NONE
            elif rec.in_op == ops.IN_MAXPOOL2 and ops.pool_pass_pays((n, cin, h, w), cout, k):
                # F(4x4,3x3) has no max-pool loader: a separate pool pass (one read of the
                # source, one write of the pooled map) + F(4x4) beats the fused F(2x2)
                out.append(Launch("maxpool2x2_ceil"))
                (h, w), rec.in_op = ops.conv_out_hw(h, w, ops.IN_MAXPOOL2), ops.IN_NONE
            if (isinstance(nxt, ConvStep) and nxt.in_op == ops.IN_MAXPOOL2 and not last
                    and rec.in_op in (ops.IN_NONE, ops.IN_UPSAMPLE2)
                    and ops.conv2d_pool_fuses((n, cin, h, w), cout, k, rec.in_op)
                    and ops.pool_pass_pays((n, cout, *ops.conv_out_hw(h, w, rec.in_op)),
                                           nxt.conv.out_channels, nxt.conv.kernel_size[0])):
                # this conv's output only feeds the next conv's pool pass: write it pooled
                # from the F(4x4) epilogue (never the full-resolution map)
                rec.op, rec.pooled, rec.takes = "conv2d_pool", True, ()
            elif rec.in_op == ops.IN_ADD_ADAIN:
                if last:
                    raise NotImplementedError("rpst plan: skip-AdaIN conv with statistics")
                rec.op, rec.takes = "conv2d_skip_adain", ("content", "aux")
            elif last:
                rec.op, rec.takes = "conv2d_stats", rec.takes + ("store_n",)
        if (precision == "bf16" and rec.op in ("conv2d", "conv2d_pair", "conv2d_stats")
                and ops.conv2d_bf16_supports(cout, cin, k, s.pad, rec.in_op)):
            rec.op = "conv2d_bf16"
        out.append(rec)
        cin, (h, w) = cout, ops.conv_out_hw(h, w, rec.in_op)
        if rec.pooled:
            h, w = ops.conv_out_hw(h, w, ops.IN_MAXPOOL2)
    if stats_last and not (out and "store_n" in out[-1].takes):
        out.append(Launch("calc_mean_std"))
    return out


def run(steps: List[object], x: torch.Tensor, first_aux=None, first_in_op=None,
        stats_last: bool = False, first_content=None, first_mix=None, store_n=None,
        x2: Optional[torch.Tensor] = None, precision: str = "fp32"):
    """Run a compiled plan: perform lower()'s launch list. first_in_op/first_aux override the
    first conv's input operator (e.g. RPST_IN_ADAIN to fuse AdaIN into the decoder's first
    conv; RPST_IN_ADD_ADAIN with first_content = the skip feature, for x + AdaIN(content));
    first_mix = (T, c) makes the first conv read T_n x + c_n (the WCT colour transform,
    rpst_conv2d_mix); stats_last makes the last conv also return calc_mean_std of its output
    -> (x, mean, std); with store_n that conv writes only images < store_n of x (the rest are
    needed only through their statistics; their part of x is unspecified). x2: the plan runs
    over the batch cat([x, x2]); a plain first conv reads both in place (rpst_conv2d_pair, or
    rpst_conv7's second input for a 7x7 conv over two equal halves), any other first step
    gets the concatenation. precision: lower()'s; "bf16" is for inference only."""
    given = dict(aux=first_aux, content=first_content, mix=first_mix, store_n=store_n, x2=x2)
    mean = std = None
    for rec in lower(steps, x.shape, None if x2 is None else x2.shape, first_in_op=first_in_op,
                     first_mix=first_mix is not None, stats_last=stats_last,
                     precision=precision):
        if rec.op == "cat":
            x = torch.cat([x, x2], dim=0)
        elif rec.op == "calc_mean_std":
            mean, std = ops.calc_mean_std(x)
        elif rec.step is None:
            x = getattr(ops, rec.op)(x)
        else:
            x = conv(rec.step, x, op=rec.op, in_op=rec.in_op,
                     **{k: given[k] for k in rec.takes})
            if "store_n" in rec.takes:
                x, mean, std = x
    return (x, mean, std) if stats_last else x


class KernelSequential(nn.Sequential):
    """nn.Sequential whose forward runs the fused rpst conv plan on the GPU.

    Children, indexing and state_dict keys are those of nn.Sequential, so reference
    checkpoints load unchanged; only the execution differs. CPU inputs raise.
    """

    def forward(self, x: torch.Tensor) -> torch.Tensor:  # noqa: D401
        return run(compile_layers(self.children()), x)
