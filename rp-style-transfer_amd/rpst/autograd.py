"""Training steps of the network families on the MI355X kernels.

A family's forward (adain_rp.py:110-138, wct_rp.py:168-194, sanet.py:248-275 / 347-382,
base.py:624-649, adain_rp.py:321-345) returns the loss dict and total_loss; train.py:186-189
then calls total_loss.backward() and optimizer.step(). Here each family's whole loss graph
is ONE torch.autograd.Function (a step): its forward runs the forward kernels and keeps the
activations the backward needs, its backward runs the backward kernels (csrc/rpst_train.hip,
csrc/rpst_train_sa.hip) and returns the gradients of the trained parameters, so an unchanged
train loop (backward + Adam) trains on the HIP path. The steps are built from shared pieces:

  conv stack   _run_steps_saving keeps every compiled plan.ConvStep's input / output;
               _stack_backward walks them last to first: activation backward (ReLU /
               LeakyReLU; a ReLU feeding a 3x3 conv directly is fused into that conv's dgrad
               as a mask), weight / bias gradient (3x3 with zero or reflect padding, 1x1 as
               a batched GEMM, the nearest x2 upsample of the conv's loader materialised for
               it) added into grads, dgrad conv (plan.conv(.., flip=True), zero pad) + reflect
               border fold, upsample backward.
  VGG losses   _vgg_saving runs the frozen VGG slices over a stylized batch keeping every
               conv input / output; _vgg_backward walks them from loss seeds at the taps
               (_seed: style mean / std terms and an MSE term): ReLU backward, dgrad,
               max-pool backward -> d stylized (no VGG weight grads). _VGGLoss is the
               relu1_1..relu4_1 style + relu4_1 content loss of the AdaIN-RP, WCT-RP,
               SourceNet and MultiScale steps; the SAModel step seeds three branches itself.
  statistics   _stats: the [mean | std | mean | std] vector of a feature pair, read by the
               loss-seed kernel and by the AdaIN backward (_adain_state, _adain_backward).
  SANet        _sanet_forward / _sanet_backward (plain and adaptive attention), under
               _transform_forward / _transform_backward.

Steps: _AdaINRPStep (RP encoder over [content; style], AdaIN, RP decoder), _WCTRPStep (the
RP decoder on a constant WCT feature), _SAModelStep (transform + decoder over three
branches), _SourceNetStep (decoder on AdaIN of frozen VGG features), _MultiScaleStep (block
encoder / decoder with an AdaIN per level: MultiScaleAdaINRPNet, and LDMSAdaINRPNet with its
two-branch levels and the 7x7 conv's backward kernels, csrc/rpst_conv7_train.hip); the
*_losses functions are their entry points.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib, ops, plan
from .ops import _stream


def relu_backward(g: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(g)
    _lib.call("rpst_relu_backward", g.data_ptr(), y.data_ptr(), out.data_ptr(), g.numel(),
              _stream(g))
    return out


def act_backward(g: torch.Tensor, y: torch.Tensor, act: int) -> torch.Tensor:
    """Backward of a conv epilogue activation from its output y (ops.ACT_*)."""
    if act == ops.ACT_RELU:
        return relu_backward(g, y)
    if act == ops.ACT_LRELU:
        out = torch.empty_like(g)
        _lib.call("rpst_leaky_relu_backward", g.data_ptr(), y.data_ptr(), out.data_ptr(),
                  g.numel(), 0.2, _stream(g))
        return out
    return g


def conv_dgrad(g: torch.Tensor, step: plan.ConvStep,
               mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gradient at the conv's input (after its input operator) from g at its output
    (pre-activation). mask: the conv's input when it is a ReLU output; the ReLU backward
    (relu_backward(dx, mask)) is then fused into the dgrad conv and the border fold, bit for
    bit (rpst_conv2d_masked, rpst_reflect_pad_border_grad_masked)."""
    c = step.conv
    k = c.kernel_size[0]
    if k == 7:
        return _conv7_dgrad(g, step)
    if mask is None:
        dx = plan.conv(c, g, flip=True)
    else:
        dx = ops.conv2d_masked(g, plan.packed_weight(c, flip=True), c.in_channels, k, mask)
    if k == 3 and step.pad == ops.PAD_REFLECT:
        n, _, h, w = g.shape
        wd = c.weight.detach().contiguous()
        ws, nbytes = _lib.workspace("reflect_pad_border_grad", g, n, c.in_channels, h, w)
        _lib.call("rpst_reflect_pad_border_grad_masked", g.data_ptr(), wd.data_ptr(),
                  None if mask is None else mask.data_ptr(), dx.data_ptr(), n, c.in_channels,
                  c.out_channels, h, w, ws.data_ptr(), nbytes, _stream(g))
    return dx


def _conv7_dgrad(g: torch.Tensor, step: plan.ConvStep) -> torch.Tensor:
    """7x7 pad-3 dgrad: rpst_conv7 with zero padding on the flip-transposed weights. Behind
    ReflectionPad2d(3) it runs on g embedded in zeros over the padded domain (H+6) x (W+6),
    which is the gradient of the padded input, and rpst_reflect_pad_backward sums every padded
    position into the pixel it mirrors (2.4 % more conv FLOPs at 512 x 512)."""
    c = step.conv
    if step.pad != ops.PAD_REFLECT:
        return plan.conv(c, g, flip=True)
    n, co, h, w = g.shape
    ge = torch.zeros((n, co, h + 6, w + 6), device=g.device, dtype=torch.float32)
    ge[:, :, 3:h + 3, 3:w + 3].copy_(g)
    gp = plan.conv(c, ge, flip=True)
    dx = torch.empty((n, c.in_channels, h, w), device=g.device, dtype=torch.float32)
    with ops._traced(f"reflect3 fold C{c.in_channels} {h}x{w} N{n}", 0.0,
                     4.0 * (gp.numel() + dx.numel())):
        _lib.call("rpst_reflect_pad_backward", gp.data_ptr(), dx.data_ptr(),
                  n * c.in_channels, h, w, 3, _stream(g))
    return dx


def _relu_mask(steps, saved, k: int, ok: bool = True) -> Optional[torch.Tensor]:
    """The ReLU output that step k's input gradient is thresholded by, when step k - 1 ends
    in a plain ReLU feeding step k, a 3x3 conv, directly (no input operator between) and ok;
    else None (the masked 1x1 dgrad is a kernel path no stack uses)."""
    if (not ok or k == 0 or steps[k - 1].relu != ops.ACT_RELU or steps[k].in_op != ops.IN_NONE
            or steps[k].conv.kernel_size[0] != 3):
        return None
    y = saved[k - 1][1]
    return y if y.is_contiguous() else None


def maxpool_backward(x: torch.Tensor, g: torch.Tensor, relu_mask: bool) -> torch.Tensor:
    n, c, h, w = x.shape
    dx = torch.empty_like(x)
    _lib.call("rpst_maxpool2x2_ceil_backward", x.data_ptr(), g.data_ptr(), dx.data_ptr(), n, c,
              h, w, int(relu_mask), _stream(x))
    return dx


def _upsample_backward(g: torch.Tensor) -> torch.Tensor:
    n, c, h2, w2 = g.shape
    dx = torch.empty((n, c, h2 // 2, w2 // 2), device=g.device, dtype=torch.float32)
    _lib.call("rpst_upsample_nearest2x_backward", g.data_ptr(), dx.data_ptr(), n * c, h2 // 2,
              w2 // 2, _stream(g))
    return dx


def conv_wgrad(x: torch.Tensor, g: torch.Tensor, conv: nn.Conv2d, pad: int = ops.PAD_ZERO):
    """3x3 conv weight / bias gradient; pad = ops.PAD_REFLECT for ReflectionPad2d(1) + conv
    (the reflection is read in the kernel's loader; equal to the zero-pad wgrad of
    _pad1(x, True) against _pad1(g, False))."""
    n, cin, h, w = x.shape
    cout = conv.out_channels
    assert conv.kernel_size == (3, 3) and tuple(g.shape) == (n, cout, h, w)
    dw = torch.empty_like(conv.weight, memory_format=torch.contiguous_format)
    db = torch.empty_like(conv.bias) if conv.bias is not None else None
    ws, nbytes = _lib.workspace("conv_wgrad", x, n, cin, h, w, cout)
    with ops._traced(f"wgrad3x3 {cin}->{cout} {h}x{w} N{n} op0{' reflect' if pad else ''}",
                     2.0 * n * cout * cin * 9 * h * w, 4.0 * (x.numel() + g.numel())):
        _lib.call("rpst_conv_wgrad_pad", x.data_ptr(), g.data_ptr(), dw.data_ptr(),
                  None if db is None else db.data_ptr(), n, cin, h, w, cout, int(pad),
                  ws.data_ptr(), nbytes, _stream(x))
    return dw, db


def conv_wgrad7(x: torch.Tensor, g: torch.Tensor, conv: nn.Conv2d, pad: int = ops.PAD_REFLECT):
    """7x7 pad-3 conv weight / bias gradient (rpst_conv7_wgrad); pad = ops.PAD_REFLECT for
    ReflectionPad2d(3) + conv, ops.PAD_ZERO for zero padding, read in the kernel's loader.
    The traced bytes count x and g once per kernel row (the kernel's blocks split the taps by
    row and each reads both)."""
    ops._check(x, g)
    n, cin, h, w = x.shape
    cout = conv.out_channels
    assert conv.kernel_size == (7, 7) and tuple(g.shape) == (n, cout, h, w)
    x, g = ops._c(x), ops._c(g)
    dw = torch.empty_like(conv.weight, memory_format=torch.contiguous_format)
    db = torch.empty_like(conv.bias) if conv.bias is not None else None
    ws, nbytes = _lib.workspace("conv7_wgrad", x, n, cin, h, w, cout)
    with ops._traced(f"wgrad7x7 {cin}->{cout} {h}x{w} N{n}{' reflect' if pad else ''}",
                     2.0 * n * cout * cin * 49 * h * w, 4.0 * (7 * x.numel() + 7 * g.numel())):
        _lib.call("rpst_conv7_wgrad", x.data_ptr(), g.data_ptr(), dw.data_ptr(),
                  None if db is None else db.data_ptr(), n, cin, h, w, cout, int(pad),
                  ws.data_ptr(), nbytes, _stream(x))
    return dw, db


def _lin_grads(dY, X):
    """1x1 conv weight / bias gradient over a batch: sum_n dY_n X_n^T (rpst_conv1x1_wgrad:
    per-image gemm_f32_kernel products and a fixed-order batch sum)."""
    b, co = dY.shape[:2]
    ci = X.shape[1]
    hw = X[0, 0].numel()
    dY, X = dY.contiguous(), X.contiguous()
    dw = torch.empty((co, ci, 1, 1), device=X.device, dtype=torch.float32)
    db = torch.empty(co, device=X.device, dtype=torch.float32)
    ws, nbytes = _lib.workspace("conv1x1_wgrad", X, b, ci, co)
    _lib.call("rpst_conv1x1_wgrad", X.data_ptr(), dY.data_ptr(), dw.data_ptr(), db.data_ptr(),
              b, ci, hw, co, ws.data_ptr(), nbytes, _stream(X))
    return dw, db


# kernel size -> (x, g, conv, pad) -> (dw, db): the weight-gradient kernel of a conv step
_WGRAD = {1: lambda x, g, conv, pad: _lin_grads(g, x), 3: conv_wgrad, 7: conv_wgrad7}


def _acc(grads: Dict[int, torch.Tensor], p: torch.Tensor, g: torch.Tensor) -> None:
    if g is None:
        return
    k = id(p)
    if k in grads:
        grads[k].add_(g)
    else:
        grads[k] = g


def sq_diff_mean(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """nn.MSELoss()(a, b) (mean reduction) as a 0-dim device tensor."""
    out = torch.empty((), device=a.device, dtype=torch.float32)
    ws, nbytes = _lib.workspace("sq_diff", a)
    _lib.call("rpst_sq_diff_sum", a.data_ptr(), b.data_ptr(), a.numel(), 1.0 / a.numel(),
              out.data_ptr(), ws.data_ptr(), nbytes, _stream(a))
    return out


# ---- conv stacks -------------------------------------------------------------------------
def _run_steps_saving(steps, x):
    """Run conv steps keeping (input, output) of each."""
    saved = []
    for s in steps:
        assert isinstance(s, plan.ConvStep)
        y = plan.conv(s, x)
        saved.append((x, y))
        x = y
    return x, saved


def _stack_backward(steps, saved, g, grads: Dict[int, torch.Tensor], need_input_grad: bool):
    """Backward through compiled conv steps from g at the last output: 3x3 convs with zero or
    reflect padding (wgrad kernel, the reflection read in its loader; dgrad + reflect border
    fold), optionally behind a nearest x2 upsample (sanet.py:162-192: fused into the conv's
    loader forward, materialised for the wgrad), 7x7 convs with zero or reflect padding 3
    (LDMSAdaINRPNet's big branch: conv_wgrad7, _conv7_dgrad), and 1x1 convs (Conv2dBlock's
    inception convs, base.py:166-171: weight gradient as a batched GEMM), each with its ReLU /
    LeakyReLU(0.2) epilogue. Parameter gradients add into grads; returns d input (None when
    not needed)."""
    masked = False  # g already thresholded by step k's ReLU (fused into the dgrad above)
    for k in range(len(steps) - 1, -1, -1):
        s = steps[k]
        x_in, y = saved[k]
        if not masked:
            g = act_backward(g, y, s.relu)
        up = s.in_op == ops.IN_UPSAMPLE2
        if not up and s.in_op != ops.IN_NONE:
            raise NotImplementedError("rpst autograd: conv stack input operator")
        x = ops.upsample_nearest2x(x_in) if up else x_in
        dw, db = _WGRAD[s.conv.kernel_size[0]](x, g, s.conv, s.pad)
        _acc(grads, s.conv.weight, dw)
        _acc(grads, s.conv.bias, db if s.conv.bias is not None else None)
        if k == 0 and not need_input_grad:
            return None
        mask = _relu_mask(steps, saved, k)
        g = conv_dgrad(g, s, mask)
        masked = mask is not None
        if up:
            g = _upsample_backward(g)
    return g


# ---- statistics vectors, loss seeds, the frozen VGG --------------------------------------
def _cat4(*parts: torch.Tensor) -> torch.Tensor:
    return torch.cat([p.reshape(-1) for p in parts])


def _stats(F: torch.Tensor, T: torch.Tensor) -> torch.Tensor:
    """[mean(F) | std(F) | mean(T) | std(T)] (planes each): the stats of the loss-seed kernel
    and (F, T = content, style features) of the AdaIN backward."""
    return _cat4(*ops.calc_mean_std(F), *ops.calc_mean_std(T))


def _style_stats(F: torch.Tensor, T: torch.Tensor):
    """(_stats(F, T), calc_style_loss(F, T)) from one pair of statistics launches."""
    mu, sd = ops.calc_mean_std(F)
    mt, st = ops.calc_mean_std(T)
    return _cat4(mu, sd, mt, st), sq_diff_mean(mu, mt) + sq_diff_mean(sd, st)


def _seed(F, target, stats, wts, out, acc: bool):
    """wts[0] * d calc_style_loss(F, target) + wts[1] * d mse(F, target) (target = None: no
    MSE term) into out (acc: added)."""
    planes = F.shape[0] * F.shape[1]
    hw = F.shape[2] * F.shape[3]
    _lib.call("rpst_style_content_loss_grad", F.data_ptr(),
              None if target is None else target.data_ptr(), stats.data_ptr(), wts.data_ptr(),
              out.data_ptr(), planes, hw, int(acc), _stream(F))


def _vgg_saving(model, x, levels=5):
    steps, saved, taps = [], [], []
    for i in range(levels):
        st = plan.of(getattr(model, f"enc_{i + 1}"))
        x, sv = _run_steps_saving(st, x)
        steps += st
        saved += sv
        taps.append(len(steps) - 1)
    return steps, saved, taps


def _vgg_backward(steps, saved, taps, seed_fn):
    """d input from seeds at the taps: seed_fn(level, F, g) returns the tap gradient with
    the level's loss terms added into g (g None: a fresh tensor)."""
    g = None
    masked = False
    for k in range(len(steps) - 1, -1, -1):
        x_in, y = saved[k]
        if k in taps:
            g = seed_fn(taps.index(k), y, g)
        if g is None:
            continue
        s = steps[k]
        if s.relu and not masked:
            g = relu_backward(g, y)
        # (a tap's loss seed is added before its ReLU backward: no fusion into a tap)
        mask = _relu_mask(steps, saved, k, ok=(k - 1) not in taps)
        g = conv_dgrad(g, s, mask)
        masked = mask is not None
        if s.in_op == ops.IN_MAXPOOL2:
            g = maxpool_backward(x_in, g, relu_mask=False)
        elif s.in_op != ops.IN_NONE:
            raise NotImplementedError("rpst autograd: VGG input operator")
    return g


class _VGGLoss:
    """calc_style_loss on relu1_1..relu4_1 + calc_content_loss on relu4_1 of a stylized
    batch (adain_rp.py:120-138, wct_rp.py:176-194) against the VGG features of the style
    and content batches: forward keeps what the backward needs, backward returns
    d total / d stylized through the frozen VGG."""

    def __init__(self, model, stylized, content, style, cw, sw, targets=None,
                 content_target=None):
        """targets: the VGG relu1_1..relu4_1 features of [style; content] when the caller
        already has them; content_target: the relu4_1 target of the content loss (default
        the content's relu4_1; SourceNet's is the AdaIN feature t, base.py:636)."""
        n = stylized.shape[0]
        self.steps, self.saved, self.taps = _vgg_saving(model, stylized, levels=4)
        if targets is None:
            # the targets are constants of the step (no gradient flows into them): F(4x4)
            ref = torch.cat([style, content], dim=0)
            targets = []
            with ops.precise_convs(on=False):
                for i in range(4):
                    ref = getattr(model, f"enc_{i + 1}")(ref)
                    targets.append(ref)
        self.stats, self.ls = [], None
        for i, k in enumerate(self.taps):
            st, term = _style_stats(self.saved[k][1], targets[i][:n])
            self.stats.append(st)
            self.ls = term if self.ls is None else self.ls + term
        self.content4 = (targets[3][n:] if content_target is None else content_target).contiguous()
        self.lc = sq_diff_mean(self.saved[self.taps[3]][1], self.content4)
        self.total = cw * self.lc + sw * self.ls
        self.cw, self.sw = cw, sw

    def backward(self, g_total, g_ls, g_lc) -> torch.Tensor:
        zero = torch.zeros((), device=self.content4.device)
        g_total = zero if g_total is None else g_total
        w_s = g_total * self.sw + (zero if g_ls is None else g_ls)
        w_c = g_total * self.cw + (zero if g_lc is None else g_lc)
        wts = torch.stack([w_s, w_c]).to(torch.float32).contiguous()

        def seed(i, F, g):  # style terms at every tap, the content MSE at relu4_1 (the first)
            if g is None:
                g = torch.empty_like(F)
            _seed(F, self.content4 if i == 3 else None, self.stats[i], wts, g, i != 3)
            return g

        g = _vgg_backward(self.steps, self.saved, self.taps, seed)
        self.saved = None
        return g


def _adain_state(cf: torch.Tensor, sf: torch.Tensor):
    return cf, sf, _stats(cf, sf)


def _adain_backward(g: torch.Tensor, state) -> torch.Tensor:
    """d AdaIN(cf, sf) -> [d cf; d sf] stacked along the batch (the shared encoder's
    [content; style] layout)."""
    cf, sf, st = state
    n = cf.shape[0]
    d = torch.empty((2 * n,) + tuple(cf.shape[1:]), device=g.device, dtype=torch.float32)
    planes = cf.shape[0] * cf.shape[1]
    hw = cf.shape[2] * cf.shape[3]
    ws = torch.empty(2 * planes, device=g.device, dtype=torch.float32)
    _lib.call("rpst_adain_backward", g.data_ptr(), cf.data_ptr(), sf.data_ptr(), st.data_ptr(),
              d[:n].data_ptr(), d[n:].data_ptr(), planes, hw, ws.data_ptr(), ws.numel() * 4,
              _stream(g))
    return d


# ---- the steps ---------------------------------------------------------------------------
# Every step is Step.apply(content, style, model, cfg, *params): cfg the loss weights
# (_losses), params the trained parameters, whose gradients its backward returns in order
# (_MultiScaleStep takes its _Family between cfg and params).
# Forward and backward both enter precise_convs(family): the autograd engine runs the
# backward on its own thread.

def _losses(step, model, content: torch.Tensor, style: torch.Tensor,
            params: List[torch.Tensor], extra: Tuple[str, ...] = (), family=None
            ) -> Tuple[Dict[str, torch.Tensor], torch.Tensor]:
    """Run a step on detached inputs with the float weights of model.config: the loss dict
    ({'style_loss', 'content_loss', f'{extra}_loss'.., 'total_loss'}) and total_loss."""
    ops._check(content, style)
    cfg = tuple(float(model.config[f'{k}_weight']) for k in ('content', 'style') + extra)
    total, ls, lc, *rest = step.apply(content.detach().contiguous(), style.detach().contiguous(),
                                      model, cfg, *(() if family is None else (family,)), *params)
    losses = {'style_loss': ls, 'content_loss': lc}
    losses.update(zip((f'{k}_loss' for k in extra), rest))
    losses['total_loss'] = total
    return losses, total


class _AdaINRPStep(torch.autograd.Function):
    """AdaINRPNet.forward (adain_rp.py:110-138): the RP encoder over [content; style] (2N),
    AdaIN (materialised: it is the decoder's first wgrad input), the RP decoder, VGG losses;
    backward = VGG dgrad, decoder, AdaIN backward, encoder."""

    @staticmethod
    def forward(ctx, content, style, model, cfg, *params):
        with ops.precise_convs("adain"):
            n = content.shape[0]
            enc_steps = plan.of(model.rp_shared_encoder)
            dec_steps = plan.of(model.rp_decoder)
            feats, enc_saved = _run_steps_saving(enc_steps, torch.cat([content, style], dim=0))
            ctx.adain = _adain_state(feats[:n], feats[n:])
            t = ops.adaptive_instance_normalization(feats[:n], feats[n:])
            stylized, dec_saved = _run_steps_saving(dec_steps, t)
            loss = _VGGLoss(model, stylized, content, style, *cfg)
        ctx.loss, ctx.params = loss, params
        ctx.enc, ctx.dec = (enc_steps, enc_saved), (dec_steps, dec_saved)
        return loss.total, loss.ls, loss.lc

    @staticmethod
    def backward(ctx, g_total, g_ls, g_lc):
        with ops.precise_convs("adain"):
            g = ctx.loss.backward(g_total, g_ls, g_lc)
            grads: Dict[int, torch.Tensor] = {}
            g = _stack_backward(*ctx.dec, g, grads, need_input_grad=True)
            # the encoder's [content; style] batch: its weight grads sum both halves
            _stack_backward(*ctx.enc, _adain_backward(g, ctx.adain), grads,
                            need_input_grad=False)
        ctx.enc = ctx.dec = None
        return (None, None, None, None, *[grads.get(id(p)) for p in ctx.params])


class _WCTRPStep(torch.autograd.Function):
    """WCTRPNet.forward (wct_rp.py:168-194): fuse() detaches the encoder features
    (wct_rp.py:161-162), so the WCT feature is a constant of the step and only the RP
    decoder is trained: forward = encoder + fp64 WCT without grad (the inference
    kernels), decoder with kept activations, VGG losses; backward = VGG dgrad, decoder
    wgrad / dgrad."""

    @staticmethod
    def forward(ctx, content, style, model, cfg, *params):
        with ops.precise_convs("wct"):
            n = content.shape[0]
            with ops.precise_convs(on=False):  # fuse() detaches: a constant of the step
                feats = plan.run(plan.of(model.rp_shared_encoder), torch.cat([content, style]))
            # per-image WCT status (device): train.py checks it after the step's loss sync
            t, model._wct_status = ops.wct_fuse(feats[:n], feats[n:], status=True)
            dec_steps = plan.of(model.rp_decoder)
            stylized, dec_saved = _run_steps_saving(dec_steps, t)
            loss = _VGGLoss(model, stylized, content, style, *cfg)
        ctx.loss, ctx.dec, ctx.params = loss, (dec_steps, dec_saved), params
        return loss.total, loss.ls, loss.lc

    @staticmethod
    def backward(ctx, g_total, g_ls, g_lc):
        with ops.precise_convs("wct"):
            g = ctx.loss.backward(g_total, g_ls, g_lc)
            grads: Dict[int, torch.Tensor] = {}
            _stack_backward(*ctx.dec, g, grads, need_input_grad=False)
        ctx.dec = None
        return (None, None, None, None, *[grads.get(id(p)) for p in ctx.params])


def adain_rp_losses(model, content: torch.Tensor, style: torch.Tensor):
    """AdaINRPNet.forward with autograd: ({'style_loss', 'content_loss', 'total_loss'},
    total_loss), differentiable w.r.t. the RP encoder / decoder parameters."""
    return _losses(_AdaINRPStep, model, content, style,
                   list(model.rp_shared_encoder.parameters()) + list(model.rp_decoder.parameters()))


def _same_size(what: str, content: torch.Tensor, style: torch.Tensor) -> None:
    """The training steps run content and style as one batch: a style of another size is an
    inference feature (test()), refused here at entry."""
    if content.shape != style.shape:
        raise ValueError(f"rpst.autograd.{what}: content {tuple(content.shape)} and style "
                         f"{tuple(style.shape)} must have one shape (a style of another size is "
                         "supported by test() only)")


def wct_rp_losses(model, content: torch.Tensor, style: torch.Tensor):
    """WCTRPNet.forward with autograd: the loss dict and total_loss, differentiable w.r.t.
    the RP decoder parameters (the only ones the reference's graph reaches)."""
    _same_size("wct_rp_losses", content, style)
    return _losses(_WCTRPStep, model, content, style, list(model.rp_decoder.parameters()))


# ---- SAModel (sanet.py:248-275) ----------------------------------------------------------
# The transform (two SANet modules + merge conv) and the VGG-style decoder train; the VGG
# encoder is frozen and the transform's inputs are its (constant) features. Three branches
# share the transform and decoder: g_t = decoder(transform(c, s)) with style (relu1..5_1)
# and mean_variance_norm content (relu4_1, relu5_1) losses, and the identity reconstructions
# Icc / Iss with l_identity1 (image MSE) and l_identity2 (feature MSE at relu1..5_1). The
# backward walks each branch: loss seeds -> VGG dgrad -> decoder (reflect-pad wgrad via
# rpst_pad1, upsample backward) -> merge conv -> SANet (1x1 convs, attention: S and dP
# GEMMs on rocBLAS, row-softmax backward kernel). Parameter gradients add over branches.

def _pad1(x: torch.Tensor, reflect: bool) -> torch.Tensor:
    n, c, h, w = x.shape
    out = torch.empty((n, c, h + 2, w + 2), device=x.device, dtype=torch.float32)
    _lib.call("rpst_pad1", x.data_ptr(), out.data_ptr(), n * c, h, w, int(reflect), _stream(x))
    return out


def _is_adaptive(m) -> bool:
    return hasattr(m, "attention_layer")


def _sanet_forward(m, c, s):
    """SANet.forward (sanet.py:82-99) / AdaptiveSANet.forward (sanet.py:106-131) keeping
    what the backward needs."""
    Fn = ops.mean_variance_norm(c)
    Gn = ops.mean_variance_norm(s)
    F = plan.conv(m.f, Fn)
    G = plan.conv(m.g, Gn)
    H = plan.conv(m.h, s)
    if _is_adaptive(m):
        al = m.attention_layer
        O, m.claim_value, _, _ = ops.adaptive_attention(
            F, G, H, c, s, al.f_psi, al.mode, float(al.scale_value), float(al.from_value),
            float(al.value_interval))
    else:
        O = ops.sanet_attention(F, G, H)
    return plan.conv(m.out_conv, O, residual=c), (Fn, Gn, s, F, G, H, O, c)


def _sanet_backward(m, saved, d_out, grads):
    """SANet / AdaptiveSANet parameter gradients (f, g, h, out_conv and the adaptive one's
    AEA f_psi MLP) from d_out (the residual's content and both inputs are constants of the
    step)."""
    Fn, Gn, s, F, G, H, O, c = saved
    b, ch, hc, wc = F.shape
    hwc, hws = hc * wc, G.shape[2] * G.shape[3]
    dw, db = _lin_grads(d_out, O)
    _acc(grads, m.out_conv.weight, dw)
    _acc(grads, m.out_conv.bias, db)
    dO = plan.conv(m.out_conv, d_out, flip=True).contiguous()
    dF, dG, dH = torch.empty_like(F), torch.empty_like(G), torch.empty_like(H)
    if _is_adaptive(m):
        # rpst_adaptive_attention_backward forms P and the clamped attention Q from the
        # logits where staged; the affinity of the (constant) VGG features feeds f_psi only
        al = m.attention_layer
        w1, b1, w2, b2, hid = ops._mlp_params(al.f_psi)
        dw1, db1 = torch.empty_like(w1), torch.empty_like(b1)
        dw2, db2 = torch.empty_like(w2), torch.empty_like(b2)
        ws, nbytes = _lib.workspace("adaptive_attention_backward", F, b, ch, hwc, hid)
        _lib.call("rpst_adaptive_attention_backward", F.data_ptr(), G.data_ptr(), H.data_ptr(),
                  c.data_ptr(), s.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                  b2.data_ptr(), hid, al.mode, float(al.scale_value), float(al.from_value),
                  float(al.value_interval), dO.data_ptr(), dF.data_ptr(), dG.data_ptr(),
                  dH.data_ptr(), dw1.data_ptr(), db1.data_ptr(), dw2.data_ptr(), db2.data_ptr(),
                  b, ch, hwc, ws.data_ptr(), nbytes, _stream(F))
        l1, l2 = al.f_psi[0], al.f_psi[2]
        for p, dp in ((l1.weight, dw1), (l1.bias, db1), (l2.weight, dw2), (l2.bias, db2)):
            _acc(grads, p, dp)
    else:
        # rpst_sanet_attention_backward_chunked: S = F^T G and dP for 2048 queries at a time
        # on gemm_f32_kernel, the softmax probabilities formed while S is staged,
        # dS = P (dP - rowsum(dP P)) -- no B x HW x HW workspace
        ws, nbytes = _lib.workspace("sanet_attention_backward_chunked", F, b, ch, hwc, hws)
        _lib.call("rpst_sanet_attention_backward_chunked", F.data_ptr(), G.data_ptr(),
                  H.data_ptr(), dO.data_ptr(), dF.data_ptr(), dG.data_ptr(), dH.data_ptr(), b,
                  ch, hwc, hws, ws.data_ptr(), nbytes, _stream(F))
    for conv, dY, X in ((m.f, dF, Fn), (m.g, dG, Gn), (m.h, dH, s)):
        dw, db = _lin_grads(dY, X)
        _acc(grads, conv.weight, dw)
        _acc(grads, conv.bias, db)


def _transform_forward(tr, c4, s4, c5, s5):
    a, sa = _sanet_forward(tr.sanet4_1, c4, s4)
    b, sb = _sanet_forward(tr.sanet5_1, c5, s5)
    out = plan.conv(tr.merge_conv, a, pad=ops.PAD_REFLECT, in_op=ops.IN_ADD_UPSAMPLE2, aux=b)
    z = a + ops.upsample_nearest2x(b)  # merge conv input, for its weight gradient
    return out, (sa, sb, z)


def _transform_backward(tr, saved, g, grads):
    sa, sb, z = saved
    c = tr.merge_conv
    dw, db = conv_wgrad(z, g, c, ops.PAD_REFLECT)
    _acc(grads, c.weight, dw)
    _acc(grads, c.bias, db)
    dz = conv_dgrad(g, plan.ConvStep(conv=c, pad=ops.PAD_REFLECT, in_op=ops.IN_NONE,
                                     relu=ops.ACT_NONE))
    _sanet_backward(tr.sanet4_1, sa, dz, grads)
    _sanet_backward(tr.sanet5_1, sb, _upsample_backward(dz), grads)


class _SAModelStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, content, style, model, cfg, *params):
        with ops.precise_convs("sanet"):
            n = content.shape[0]
            # frozen VGG of the inputs: constants of the step, but they feed the
            # differentiated transforms, so they stay precise like the rest of the step: on
            # F(4x4) the AdaptiveSAModel's style loss moves 2.85e-4 against its 2.73e-4 bar
            # (profiles/r04f) and SAModel's sanet5_1.h.weight gradient 1.06e-4 against 1e-4
            # (profiles/r04g). F(4x4) on the first slice (relu1_1) alone passes the tests
            # for +0.5 %, on two it already moves sanet4_1.h.weight's gradient to 3.5e-4
            # against 1e-4 (profiles/r04/sam_f4.log)
            feats = []
            x = torch.cat([style, content], dim=0)
            for i in range(5):
                x = getattr(model, f"enc_{i + 1}")(x)
                feats.append(x)
            sf = [f[:n].contiguous() for f in feats]
            cf = [f[n:].contiguous() for f in feats]
            dec_steps = plan.of(model.decoder)
            tr = model.transform
            br = {}
            for name, (a4, b4, a5, b5) in (("gt", (cf[3], sf[3], cf[4], sf[4])),
                                           ("cc", (cf[3], cf[3], cf[4], cf[4])),
                                           ("ss", (sf[3], sf[3], sf[4], sf[4]))):
                t, tsv = _transform_forward(tr, a4, b4, a5, b5)
                img, dsv = _run_steps_saving(dec_steps, t)
                vs, vsv, taps = _vgg_saving(model, img)
                br[name] = (tsv, dsv, (vs, vsv, taps), img)
            gtf = [br["gt"][2][1][k][1] for k in br["gt"][2][2]]
            ls = None
            sstats = []
            for i in range(5):
                st, term = _style_stats(gtf[i], sf[i])
                sstats.append(st)
                ls = term if ls is None else ls + term
            mvn = {}
            lc = None
            for i in (3, 4):
                y = ops.mean_variance_norm(gtf[i])
                yt = ops.mean_variance_norm(cf[i])
                mvn[i] = (y, yt, ops.calc_mean_std(gtf[i])[1].reshape(-1).contiguous(),
                          _stats(y, yt))
                term = sq_diff_mean(y, yt)
                lc = term if lc is None else lc + term
            icc, iss = br["cc"][3], br["ss"][3]
            l1 = sq_diff_mean(icc, content) + sq_diff_mean(iss, style)
            fcc = [br["cc"][2][1][k][1] for k in br["cc"][2][2]]
            fss = [br["ss"][2][1][k][1] for k in br["ss"][2][2]]
            l2 = None
            for i in range(5):
                term = sq_diff_mean(fcc[i], cf[i]) + sq_diff_mean(fss[i], sf[i])
                l2 = term if l2 is None else l2 + term
            total = (cfg[0] * lc + cfg[1] * ls + cfg[2] * l1 + cfg[3] * l2)
        ctx.save = (model, dec_steps, br, sf, cf, sstats, mvn, content, style, cfg, params)
        return total, ls, lc, l1, l2

    @staticmethod
    def backward(ctx, g_total, g_ls, g_lc, g_l1, g_l2):
        model, dec_steps, br, sf, cf, sstats, mvn, content, style, cfg, params = ctx.save
        zero = torch.zeros((), device=content.device)

        def w(g_part, k):
            gt = zero if g_total is None else g_total
            return gt * cfg[k] + (zero if g_part is None else g_part)

        w_c, w_s, w_1, w_2 = w(g_lc, 0), w(g_ls, 1), w(g_l1, 2), w(g_l2, 3)
        wt = lambda a, b: torch.stack([a, b]).to(torch.float32).contiguous()  # noqa: E731
        w_style, w_mse_c, w_mse_2, w_mse_1 = wt(w_s, zero), wt(zero, w_c), wt(zero, w_2), wt(zero, w_1)
        grads: Dict[int, torch.Tensor] = {}

        def gt_seed(i, F, g):
            fresh = g is None
            if fresh:
                g = torch.empty_like(F)
            if i in mvn:  # content loss: mse(mvn(F), mvn(Fc)) -> through mean_variance_norm
                y, yt, sd, st = mvn[i]
                dy = torch.empty_like(y)
                _seed(y, yt, st, w_mse_c, dy, False)
                _lib.call("rpst_mean_variance_norm_backward", y.data_ptr(), dy.data_ptr(),
                          sd.data_ptr(), g.data_ptr(), F.shape[0] * F.shape[1],
                          F.shape[2] * F.shape[3], int(not fresh), _stream(F))
                fresh = False
            _seed(F, None, sstats[i], w_style, g, not fresh)
            return g

        def id_seed(targets):
            def fn(i, F, g):
                st = _stats(F, targets[i])
                acc = g is not None
                if not acc:
                    g = torch.empty_like(F)
                _seed(F, targets[i], st, w_mse_2, g, acc)
                return g
            return fn

        with ops.precise_convs("sanet"):
            for name, seed_fn, img_target in (("gt", gt_seed, None), ("cc", id_seed(cf), content),
                                              ("ss", id_seed(sf), style)):
                tsv, dsv, (vs, vsv, taps), img = br[name]
                g = _vgg_backward(vs, vsv, taps, seed_fn)
                if img_target is not None:  # l_identity1 on the reconstructed image
                    _seed(img, img_target, _stats(img, img_target), w_mse_1, g, True)
                g = _stack_backward(dec_steps, dsv, g, grads, need_input_grad=True)
                _transform_backward(model.transform, tsv, g, grads)
        ctx.save = None
        return (None, None, None, None, *[grads.get(id(p)) for p in params])


def samodel_losses(model, content: torch.Tensor, style: torch.Tensor):
    """SAModel.forward with autograd: the loss dict of sanet.py:248-275 and total_loss,
    differentiable w.r.t. the transform and decoder parameters. AdaptiveSAModel.forward
    (sanet.py:347-382: the same losses around an AdaptiveTransform) runs through the same
    step, its AdaptiveSANets (and their f_psi MLPs) on rpst_adaptive_attention_backward."""
    _same_size("samodel_losses", content, style)
    return _losses(_SAModelStep, model, content, style,
                   list(model.transform.parameters()) + list(model.decoder.parameters()),
                   extra=('l_identity1', 'l_identity2'))


# ---- SourceNet (base.py:624-649) and MultiScaleAdaINRPNet (adain_rp.py:321-345) -----------
class _SourceNetStep(torch.autograd.Function):
    """SourceNet.forward (base.py:624-649): VGG relu1_1..relu4_1 of content and style (frozen,
    constants of the step), t = AdaIN(c4, s4), g_t = decoder(t); style loss at the four taps,
    content loss of g_t's relu4_1 against t. Only the decoder trains."""

    @staticmethod
    def forward(ctx, content, style, model, cfg, *params):
        with ops.precise_convs("source"):
            n = content.shape[0]
            ref, targets = torch.cat([style, content], dim=0), []
            with ops.precise_convs(on=False):  # frozen VGG of the inputs: constants
                for i in range(4):
                    ref = getattr(model, f"enc_{i + 1}")(ref)
                    targets.append(ref)
            t = ops.adaptive_instance_normalization(targets[3][n:], targets[3][:n])
            dec_steps = plan.of(model.decoder)
            stylized, dec_saved = _run_steps_saving(dec_steps, t)
            loss = _VGGLoss(model, stylized, content, style, *cfg, targets=targets,
                            content_target=t)
        ctx.loss, ctx.dec, ctx.params = loss, (dec_steps, dec_saved), params
        return loss.total, loss.ls, loss.lc

    @staticmethod
    def backward(ctx, g_total, g_ls, g_lc):
        with ops.precise_convs("source"):
            g = ctx.loss.backward(g_total, g_ls, g_lc)
            grads: Dict[int, torch.Tensor] = {}
            _stack_backward(*ctx.dec, g, grads, need_input_grad=False)
        ctx.dec = None
        return (None, None, None, None, *[grads.get(id(p)) for p in ctx.params])


class _Family(NamedTuple):
    """What _MultiScaleStep needs to know of a multi-scale AdaIN family."""
    levels: list          # per encoder level its Conv2dBlocks: one, or branches concatenated
    decoder: list         # decoder blocks, the first on the top level
    content_is_y: bool    # block k >= 1 adds AdaIN(y, s_level) (LD), not AdaIN(c_level, s_level)
    f4: str               # the ops.precise_convs (TRAIN_F4) family
    params: list          # the trained parameters


class _MultiScaleStep(torch.autograd.Function):
    """MultiScaleAdaINRPNet.forward (adain_rp.py:321-345) for the constant / deeper stacks and
    LDMSAdaINRPNet's loss graph (adain_rp.py:484-567 under the same forward), told apart by
    fam (_Family).

    Forward: the encoder over [content; style] level by level, every conv's input / output
    kept; a level is its block's output, or its branches' outputs (LD: 3x3 small, 7x7 big;
    level 0 two 3x3) concatenated. Decoder block 0 on AdaIN(level L-1), block k on
    y_{k-1} + AdaIN(c, s_{L-1-k}) with c the level's content half (adain_rp.py:291-302) or,
    for LD, y_{k-1} itself (adain_rp.py:550); the sums and AdaIN outputs are materialised,
    they are the blocks' wgrad inputs. VGG losses on the stylized batch.
    Backward: VGG dgrad -> decoder blocks (LeakyReLU, 1x1 / reflect 3x3 wgrad + dgrad); the
    gradient g at each block input goes through AdaIN backward to [d content; d style] of the
    level and on to the previous block's output: unchanged, or for LD as g + d content, the
    level keeping d style alone (its content halves below the top level reach the loss only
    through the level above). The encoder walks back with each level's gradient added at its
    output; a two-branch level splits it at the channel midpoint, each branch goes through
    _stack_backward, and the two input gradients are summed."""

    @staticmethod
    def forward(ctx, content, style, model, cfg, fam, *params):
        with ops.precise_convs(fam.f4):
            n = content.shape[0]
            x, enc, levels = torch.cat([content, style], dim=0), [], []
            for blocks in fam.levels:
                branches, outs = [], []
                for blk in blocks:
                    st = plan.of(blk)
                    y, sv = _run_steps_saving(st, x)
                    branches.append((st, sv))
                    outs.append(y)
                enc.append(branches)
                x = outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)
                levels.append(x)
            L = len(levels)
            dec, states = [], []
            y = None
            for k, blk in enumerate(fam.decoder):
                lv = levels[L - 1 - k]
                cf = y if k and fam.content_is_y else lv[:n]
                states.append(_adain_state(cf, lv[n:]))
                z = ops.adaptive_instance_normalization(cf, lv[n:])
                if k:
                    z.add_(y)
                st = plan.of(blk)
                y, sv = _run_steps_saving(st, z)
                dec.append((st, sv))
                if k == L - 1:
                    break
            loss = _VGGLoss(model, y, content, style, *cfg)
        ctx.loss, ctx.enc, ctx.dec, ctx.states, ctx.fam = loss, enc, dec, states, fam
        return loss.total, loss.ls, loss.lc

    @staticmethod
    def backward(ctx, g_total, g_ls, g_lc):
        fam = ctx.fam
        with ops.precise_convs(fam.f4):
            g = ctx.loss.backward(g_total, g_ls, g_lc)
            grads: Dict[int, torch.Tensor] = {}
            L = len(ctx.enc)
            n = g.shape[0]
            dlev = [None] * L
            for k in range(len(ctx.dec) - 1, -1, -1):
                g = _stack_backward(*ctx.dec[k], g, grads, need_input_grad=True)
                d = _adain_backward(g, ctx.states[k])  # [d content; d style]
                if k and fam.content_is_y:
                    g = g + d[:n]   # the skip and AdaIN's own content, both the block below
                    d[:n].zero_()
                dlev[L - 1 - k] = d
            ge = None
            for i in range(L - 1, -1, -1):
                if dlev[i] is not None:
                    ge = dlev[i] if ge is None else ge.add_(dlev[i])
                if ge is None:
                    continue
                if len(ctx.enc[i]) == 1:
                    ge = _stack_backward(*ctx.enc[i][0], ge, grads, need_input_grad=i > 0)
                    continue
                c = ge.shape[1] // 2
                dx = None
                for (st, sv), gb in zip(ctx.enc[i], (ge[:, :c], ge[:, c:])):
                    d = _stack_backward(st, sv, gb.contiguous(), grads, need_input_grad=i > 0)
                    dx = d if dx is None else dx.add_(d)
                ge = dx
        ctx.enc = ctx.dec = ctx.states = None
        return (None, None, None, None, None, *[grads.get(id(p)) for p in fam.params])


def ld_losses(model, content: torch.Tensor, style: torch.Tensor):
    """LDMSAdaINRPNet's training entry (its forward() with autograd enabled): the loss dict of
    the reference's forward ({'style_loss', 'content_loss', 'total_loss'}) and total_loss,
    differentiable w.r.t. every rp_enc* / rp_dec* parameter (the VGG is frozen)."""
    model._kernel_path_check()
    params = [p for name, p in model.named_parameters() if name.startswith(("rp_enc", "rp_dec"))]
    L = model.layer_num
    fam = _Family([model._level_blocks(i) for i in range(L)], [model._dec(k) for k in range(L)],
                  True, "ld", params)
    return _losses(_MultiScaleStep, model, content, style, params, family=fam)


def sourcenet_losses(model, content: torch.Tensor, style: torch.Tensor):
    """SourceNet.forward with autograd: the loss dict and total_loss, differentiable w.r.t.
    the decoder parameters."""
    return _losses(_SourceNetStep, model, content, style, list(model.decoder.parameters()))


def multiscale_losses(model, content: torch.Tensor, style: torch.Tensor):
    """MultiScaleAdaINRPNet.forward with autograd: the loss dict and total_loss,
    differentiable w.r.t. the RP encoder / decoder parameters."""
    params = list(model.rp_shared_encoder.parameters()) + list(model.rp_decoder.parameters())
    fam = _Family([[blk] for blk in model.rp_shared_encoder], list(model.rp_decoder), False,
                  "multiscale", params)
    return _losses(_MultiScaleStep, model, content, style, params, family=fam)
