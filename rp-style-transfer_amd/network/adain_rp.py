"""Drop-in AdaINRPNet (reference network/adain_rp.py:15-138) and MultiScaleAdaINRPNet
(adain_rp.py:141-345) on MI355X kernels.

Constructor, attribute names, state_dict keys and the test()/forward()/save()
signatures follow the reference. test() runs the shared RP encoder ONCE over the
concatenated [content; style] batch (the encoder weights are shared,
adain_rp.py:96-97), AdaIN with the HIP statistics kernels, then the RP decoder.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from rpst import ops, plan
from rpst.plan import KernelSequential

from .base import (BaseNet, Conv2dBlock, SourceNet, StackType,  # noqa: F401 (star exports)
                   config_precision,
                   adaptive_instance_normalization, build_decrease_depth_rp_blocks,
                   build_increase_depth_rp_blocks, calc_mean_std, masked_adain_batch, mse,
                   rp_constant_conv_blocks, segment_maps,
                   rp_deeper_conv_blocks, rp_shallower_conv_blocks)
from .base import adaptive_instance_normalization as AdaIN  # noqa: F401 (reference alias)


# RPST_FUSE_ADAIN=0 disables the fused path (A/B measurements, debugging)
FUSED_ADAIN = os.environ.get("RPST_FUSE_ADAIN", "1") != "0"
# RPST_ADAIN_STORE_ALL=1 writes the style half of the encoder output too (A/B)
STORE_ALL = os.environ.get("RPST_ADAIN_STORE_ALL", "0") == "1"


def adain_rp_fused(encoder, decoder, content, style, precision="fp32"):
    """enc -> AdaIN -> dec with AdaIN fused into its neighbours (adain_rp.py:94-101):
    the encoder's last conv emits calc_mean_std of its output from its epilogue, and the
    decoder's first conv applies ((c - mu_c)/sigma_c)*sigma_s + mu_s while loading its
    input tile, so the AdaIN feature is never written to HBM. The style half of the encoder
    output is consumed only through its statistics: that conv writes the content half alone
    (store_n = n; adain_rp.py:94-101 reads style_feat only via calc_mean_std).
    precision "bf16": both plans send the conv steps ops.conv2d_bf16_supports accepts to the
    bf16 kernel (plan.lower)."""
    n = content.shape[0]
    assert content.size() == style.size()
    feats, mean, std = plan.run(plan.of(encoder), content, x2=style, stats_last=True,
                                store_n=None if STORE_ALL else n, precision=precision)
    aux = ops.adain_params(mean[:n], std[:n], mean[n:], std[n:])
    return plan.run(plan.of(decoder), feats[:n], first_aux=aux, first_in_op=ops.IN_ADAIN,
                    precision=precision)


def encode_both(encoder, content, style):
    """Run a shared encoder over content and style in one pass of 2N images; a style of
    another size than the content takes a pass of its own (the reference encodes the two
    separately, adain_rp.py / wct_rp.py test())."""
    if content.shape != style.shape:
        return encoder(content), encoder(style)
    n = content.shape[0]
    feats = encoder(torch.cat([content, style], dim=0))
    return feats[:n], feats[n:]


class AdaINRPNet(BaseNet):
    def __init__(self, config, vgg_encoder) -> None:
        super().__init__()
        enc_layers = list(vgg_encoder.children())
        self.config = config
        # test() alone reads it (adain_rp_fused); forward() and training stay fp32. The
        # subclasses have no bf16 path: they raise here
        self.precision = config_precision(config, type(self).__name__,
                                          bf16_ok=type(self) is AdaINRPNet)
        self.enc_1 = KernelSequential(*enc_layers[:4])    # input -> relu1_1
        self.enc_2 = KernelSequential(*enc_layers[4:11])  # relu1_1 -> relu2_1
        self.enc_3 = KernelSequential(*enc_layers[11:18])  # relu2_1 -> relu3_1
        self.enc_4 = KernelSequential(*enc_layers[18:31])  # relu3_1 -> relu4_1
        for name in ['enc_1', 'enc_2', 'enc_3', 'enc_4']:
            for param in getattr(self, name).parameters():
                param.requires_grad = False
        assert self.config['rp_blocks'] - 2 >= 0
        self.encoder_out_dim = self.config['hidden_dim'] * 2 ** (self.config['rp_blocks'] - 1)
        self.rp_shared_encoder = build_increase_depth_rp_blocks(
            self.config['rp_blocks'], 3, self.config['hidden_dim'], self.encoder_out_dim)
        self.decoder_in_dim = self.encoder_out_dim
        self.decoder_hidden_dim = self.decoder_in_dim // 2
        self.rp_decoder = build_decrease_depth_rp_blocks(
            self.config['rp_blocks'], self.decoder_in_dim, self.decoder_hidden_dim, 3)
        self.mse_loss = nn.MSELoss()

    def encode_with_intermediate(self, input):
        results = [input]
        for i in range(4):
            results.append(getattr(self, 'enc_{:d}'.format(i + 1))(results[-1]))
        return results[1:]

    def encode(self, input):
        for i in range(4):
            input = getattr(self, 'enc_{:d}'.format(i + 1))(input)
        return input

    def calc_content_loss(self, input, target):
        return mse(input, target)

    def calc_style_loss(self, input, target):
        input_mean, input_std = calc_mean_std(input)
        target_mean, target_std = calc_mean_std(target)
        return mse(input_mean, target_mean) + mse(input_std, target_std)

    def fuse(self, content_feats, style_feats):
        return adaptive_instance_normalization(content_feats, style_feats)

    def test(self, content, style, iterations=0, bid=0, c_mask_path=None, s_mask_path=None):
        with torch.no_grad():
            if type(self).fuse is AdaINRPNet.fuse and FUSED_ADAIN:
                return adain_rp_fused(self.rp_shared_encoder, self.rp_decoder, content, style,
                                      self.precision)
            if self.precision != "fp32":
                raise NotImplementedError("AdaINRPNet: precision 'bf16' runs on the fused "
                                          "test() path only (RPST_FUSE_ADAIN=0 disables it)")
            content_feat, style_feat = encode_both(self.rp_shared_encoder, content, style)
            fusion_feat = self.fuse(content_feat, style_feat)
            return self.rp_decoder(fusion_feat)

    def save(self, save_path, iterations=0):
        torch.save({'encoder': self.rp_shared_encoder.state_dict(),
                    'decoder': self.rp_decoder.state_dict()}, save_path)

    def forward(self, content, style, alpha=1.0):
        """Loss dict of adain_rp.py:110-138. With autograd enabled and trainable RP
        parameters the losses come from rpst.autograd (one autograd.Function over the
        forward and backward kernels), so total_loss.backward() fills the RP encoder /
        decoder gradients as in train.py:186-189; under no_grad it is evaluated op by op."""
        assert 0 <= alpha <= 1
        if type(self) is AdaINRPNet and torch.is_grad_enabled() and any(
                p.requires_grad for p in self.parameters()):
            from rpst.autograd import adain_rp_losses
            return adain_rp_losses(self, content, style)
        content_feat, style_feat = encode_both(self.rp_shared_encoder, content, style)
        stylized = self.rp_decoder(AdaIN(content_feat, style_feat))
        # the three VGG passes (adain_rp.py:123-125) as one pass over [stylized; style;
        # content]: the same per-image results (the kernels are batch-invariant bit for bit,
        # tests/test_gpu_timed.py), one launch sequence and 3x the grid at relu4_1's 64^2
        n = content.shape[0]
        feats = self.encode_with_intermediate(torch.cat([stylized, style, content], dim=0))
        down_stylized_feats, down_style_feats, down_content_feats = (
            [f[j * n:(j + 1) * n] for f in feats] for j in range(3))
        loss_s = self.calc_style_loss(down_stylized_feats[0], down_style_feats[0])
        for i in range(1, 4):
            loss_s += self.calc_style_loss(down_stylized_feats[i], down_style_feats[i])
        loss_c = self.calc_content_loss(down_stylized_feats[-1], down_content_feats[-1])
        total_loss = self.config['content_weight'] * loss_c + self.config['style_weight'] * loss_s
        return {'style_loss': loss_s, 'content_loss': loss_c, 'total_loss': total_loss}, total_loss


def _encode_se_block(blk, x, x2, n, stats):
    """One encoder block with SE attention over the [content; style] batch of 2n: the conv
    plan without statistics, then the SE block, whose gated conv emits calc_mean_std of the
    block's output when `stats`. blk.attention_map becomes the style half's gates, as after
    the reference's content-then-style encoding (adain_rp.py:286-290)."""
    x = plan.run(plan.of(blk), x, x2=x2)
    res = ops.se_bottleneck(x, blk.attention_block, stats=stats)
    gate = res[1][n:]
    blk.attention_block.attention_map = blk.attention_block.se.attention_map = gate
    blk.attention_map = gate
    return (res[0], res[2], res[3]) if stats else res[0]


class MultiScaleAdaINRPNet(AdaINRPNet):
    """Multi-scale AdaIN-RP (adain_rp.py:141-345): every encoder
    block's output is kept; decoding starts from AdaIN of the deepest level and, before
    each next decoder block, adds AdaIN of the next shallower level (adain_rp.py:291-302).
    Constant ('constant') and deeper/shallower ('deeper') stacks of Conv2dBlocks
    (reflect pad, LeakyReLU 0.2). shuffle / sort are not on the kernel path. attention 'se'
    (constant stack: an SEBottleneck after every encoder block, adain_rp.py:160-168) runs in
    test() / decode() only: BatchNorm's batch statistics have no kernel, so forward() raises.

    test() runs the shared encoder once over [content; style]; each encoder block emits
    calc_mean_std of its output from its last conv's epilogue; the decoder's first conv
    applies AdaIN while staging its input and every later block's first conv forms
    stylized + AdaIN(c_i, s_i) in its loader (RPST_IN_ADD_ADAIN), so no AdaIN or sum
    tensor is ever written.

    use_mask (test / decode only, adain_rp.py:286-319): every level's AdaIN is taken per
    segmentation label (masks resized to the image size, which every level shares, so the
    label counts and validity are planned once); the masked kernels write stylized +
    AdaINSeg(c_i, s_i) once per level and the decoder block reads it as a plain input. The
    encoder then emits no epilogue statistics.

    test() (the unfused, masked and fused routes, one exit), decode() with its masked loop and
    forward() serve the whole family: LDMSAdaINRPNet overrides only the hooks listed below
    _kernel_path_check."""

    def __init__(self, config, vgg_encoder) -> None:
        super().__init__(config, vgg_encoder)
        self.config = config
        self.rp_shared_encoder = None
        self.rp_decoder = None
        self._shuffle = self.config['shuffle']
        self._shuffle_layers = self.config['shuffle_layers']
        self._sort = self.config['sort']
        self.layer_num = self.config['rp_blocks']
        self._stylized_layers = self.config['stylized_layers']
        if self.config['enc_stack_way'] == StackType.Deeper:
            self.rp_shared_encoder = rp_deeper_conv_blocks(
                self.config['rp_blocks'], 3, self.config['hidden_dim'], self.encoder_out_dim,
                inception_num=self.config['inception_num'])
            self.rp_decoder = rp_shallower_conv_blocks(
                self.config['rp_blocks'], self.decoder_in_dim, self.decoder_hidden_dim, 3)
        elif self.config['enc_stack_way'] == StackType.Constant:
            self.encoder_out_dim = self.config['hidden_dim']
            self.rp_shared_encoder = rp_constant_conv_blocks(
                self.config['rp_blocks'], 3, self.config['hidden_dim'], self.encoder_out_dim,
                inception_num=self.config['inception_num'], attention=self.config['attention'])
            self.decoder_in_dim = self.encoder_out_dim
            self.rp_decoder = rp_constant_conv_blocks(
                self.config['rp_blocks'], self.decoder_in_dim, self.config['hidden_dim'], 3)
        if self.config['resume']:
            checkpoint_path = self.config['checkpoint_path']
            self.begin = int(os.path.splitext(os.path.basename(checkpoint_path))[0])
            state_dict = torch.load(checkpoint_path, weights_only=True)
            self.rp_shared_encoder.load_state_dict(state_dict['encoder'])
            self.rp_decoder.load_state_dict(state_dict['decoder'])

    def _kernel_path_check(self):
        if self._sort or self._shuffle:
            raise NotImplementedError(
                "MultiScaleAdaINRPNet: shuffle / sort have no rpst kernel path")

    # What a family of this shape defines (LDMSAdaINRPNet overrides these and nothing else of
    # test() / decode() / forward()): the rpst.autograd entry point of forward(), the blocks of
    # encoder level i, decoder block k, a level over the [content; style] pair
    # (_encode_level), the fused decode (_decode_fused) and the unmasked skip rule of decode()
    # (_decode_skip).
    _losses_entry = 'multiscale_losses'

    def _level_blocks(self, i):
        return [self.rp_shared_encoder[i]]

    def _dec(self, k):
        return self.rp_decoder[k]

    def _has_attention(self):
        return any(blk.attention_block is not None
                   for i in range(self.layer_num) for blk in self._level_blocks(i))

    def encode_rp_intermediate(self, input):
        results = [input]
        for i in range(len(self.rp_shared_encoder)):
            results.append(self.rp_shared_encoder[i](results[-1]))
        return results[1:]

    def _encode_level(self, i, x, x2, n, stats):
        """Encoder level i over the [content; style] batch of 2n, given as x (or as x and x2,
        read in place: no concat); stats: -> (feature, mean, std), calc_mean_std of the
        feature from the last conv's epilogue."""
        blk = self.rp_shared_encoder[i]
        if blk.attention_block is not None:
            return _encode_se_block(blk, x, x2, n, stats)
        return plan.run(plan.of(blk), x, stats_last=stats, x2=x2)

    def _encode_pair(self, content, style, stats=False):
        """Every level over [content; style], the encoder run once."""
        x, x2, levels = content, style, []
        for i in range(self.layer_num):
            levels.append(self._encode_level(i, x, x2, content.shape[0], stats))
            x, x2 = (levels[-1][0] if stats else levels[-1]), None
        return levels

    def test(self, content, style, iterations=0, bid=0, c_mask_path=None, s_mask_path=None):
        self.eval()
        with torch.no_grad():
            self._kernel_path_check()
            use_mask = self.config['use_mask']
            n = content.shape[0]
            if not FUSED_ADAIN:
                content_feats = self.encode_rp_intermediate(content)
                style_feats = self.encode_rp_intermediate(style)
                y = self.decode(content_feats, style_feats, use_mask=use_mask,
                                c_mask_path=c_mask_path, s_mask_path=s_mask_path)
            elif use_mask:
                feats = self._encode_pair(content, style)  # no epilogue statistics
                y = self.decode([f[:n] for f in feats], [f[n:] for f in feats], True,
                                c_mask_path, s_mask_path)
            else:
                y = self._decode_fused(content, style, n)
        self.train()
        return y

    def _decode_fused(self, content, style, n):
        """test() without masks: every level's statistics come from its encoder epilogue and
        every AdaIN (and skip sum) is formed in a decoder block's first conv loader."""
        levels = self._encode_pair(content, style, stats=True)  # (feature over 2n, mean, std)

        def params(lv):
            _, m, s = lv
            return ops.adain_params(m[:n], s[:n], m[n:], s[n:])

        y = plan.run(plan.of(self._dec(0)), levels[-1][0][:n],
                     first_aux=params(levels[-1]), first_in_op=ops.IN_ADAIN)
        for i, lv in enumerate(levels[:-1][::-1]):
            y = plan.run(plan.of(self._dec(i + 1)), y, first_aux=params(lv),
                         first_in_op=ops.IN_ADD_ADAIN, first_content=lv[0][:n])
        return y

    def decode(self, content_feats, style_feats, use_mask=False, c_mask_path=None, s_mask_path=None):
        """adain_rp.py:291-302 (LDMSAdaINRPNet: 538-553), op by op: AdaIN kernels, then each
        block with the skip sum formed in its first conv's loader (_decode_skip). use_mask:
        per-label AdaIN of (c_i, s_i) at every level (do_mask_stylized), the skip sum formed by
        the masked apply kernel."""
        self._kernel_path_check()
        pairs = list(zip(content_feats[:-1], style_feats[:-1]))[::-1]
        if use_mask:
            # all levels share H x W: decode the masks and plan the labels once
            n, dev = content_feats[-1].shape[0], content_feats[-1].device
            c_seg = segment_maps(c_mask_path, n, content_feats[-1].shape[2:], dev)
            s_seg = segment_maps(s_mask_path, n, style_feats[-1].shape[2:], dev)
            stylized, seg_plan = masked_adain_batch(content_feats[-1], style_feats[-1], c_seg,
                                                    s_seg)
            stylized = self._dec(0)(stylized)
            for i, (content_feat, style_feat) in enumerate(pairs):
                fused, _ = masked_adain_batch(content_feat, style_feat, c_seg, s_seg,
                                              skip=stylized, plan=seg_plan)
                stylized = self._dec(i + 1)(fused)
            return stylized
        stylized = self._dec(0)(AdaIN(content_feats[-1], style_feats[-1]))
        for i, (content_feat, style_feat) in enumerate(pairs):
            stylized = self._decode_skip(i + 1, stylized, content_feat, style_feat)
        return stylized

    def _decode_skip(self, k, stylized, content_feat, style_feat):
        """Decoder block k on stylized + AdaIN(content_feat, style_feat)."""
        cm, cs = calc_mean_std(content_feat)
        sm, ss = calc_mean_std(style_feat)
        return plan.run(plan.of(self._dec(k)), stylized,
                        first_aux=ops.adain_params(cm, cs, sm, ss),
                        first_in_op=ops.IN_ADD_ADAIN, first_content=content_feat)

    def forward(self, content, style, alpha=1.0):
        """Loss dict of adain_rp.py:322-345. With autograd enabled and trainable RP
        parameters the losses come from rpst.autograd._MultiScaleStep through the family's
        entry point (forward and backward kernels; total_loss.backward() fills the RP encoder /
        decoder gradients); under no_grad it is evaluated op by op."""
        assert 0 <= alpha <= 1
        if self._has_attention():
            raise NotImplementedError(
                "MultiScaleAdaINRPNet: 'se' attention is inference only (test / decode): "
                "training-mode BatchNorm and the SE block's backward have no rpst kernel")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            self._kernel_path_check()
            from rpst import autograd
            return getattr(autograd, self._losses_entry)(self, content, style)
        content_feats = self.encode_rp_intermediate(content)
        style_feats = self.encode_rp_intermediate(style)
        stylized = self.decode(content_feats, style_feats)
        down_stylized_feats = self.encode_with_intermediate(stylized)
        down_style_feats = self.encode_with_intermediate(style)
        down_content_feats = self.encode_with_intermediate(content)
        loss_s = self.calc_style_loss(down_stylized_feats[0], down_style_feats[0])
        for i in range(1, 4):
            loss_s += self.calc_style_loss(down_stylized_feats[i], down_style_feats[i])
        loss_c = self.calc_content_loss(down_stylized_feats[-1], down_content_feats[-1])
        total_loss = self.config['content_weight'] * loss_c + self.config['style_weight'] * loss_s
        return {'style_loss': loss_s, 'content_loss': loss_c, 'total_loss': total_loss}, total_loss


class LDMSAdaINRPNet(MultiScaleAdaINRPNet):
    """Large-receptive-field multi-scale AdaIN-RP (adain_rp.py:484-567; `network: ld_adain`).
    Every encoder level runs two Conv2dBlocks on the previous level and
    concatenates them: rp_enc{i}_small_revf (3x3) and rp_enc{i}_big_revf (level 0: 3x3, 3 -> h;
    level i >= 1: 7x7 pad 3, h 2^i -> h 2^i, the rpst_conv7 kernel), so level i has h 2^(i+1)
    channels. decode() starts from rp_dec0(AdaIN(c[-1], s[-1])) and before every later block
    adds AdaIN(stylized, s_i), whose content statistics are stylized's own (adain_rp.py:550);
    use_mask takes the per-label AdaIN of (c_i, s_i) instead, as the parent does.

    test() runs the encoder once over [content; style]; per level the 7x7 branch's kernel
    writes the upper channel half of the level tensor in place and the 3x3 branch's half is
    copied in (one strided copy: the 3x3 kernels have no channel-offset output). The decoder's
    first conv applies AdaIN in its loader (RPST_IN_ADAIN) and every later block's first conv
    forms stylized + AdaIN(stylized, s_i) in its loader (RPST_IN_ADD_ADAIN with the block
    input as its own content and the statistics of the previous block's epilogue).

    Deviations from the reference, both where it cannot run: stylized_layers < ld_layer_num
    raises ValueError at construction (the reference adds a Python list to a tensor in decode),
    and `resume: True` builds the modules and then loads the checkpoint that save() writes
    (torch.save(self.state_dict())) strictly, begin taken from the file name (the reference
    loads into the parent's encoder, which is None for this family).

    test(), decode() (its masked loop included) and forward() are the parent's: this class
    defines the family's hooks only (two blocks per level, rp_dec{k}, _encode_level,
    _decode_fused, _decode_skip). forward() with autograd enabled returns
    rpst.autograd.ld_losses(self, content, style), so train.py trains it like every other
    family."""

    def __init__(self, config, vgg_encoder) -> None:
        super().__init__(dict(config, resume=False), vgg_encoder)
        self.config = config
        self.hidden_dim = self.config['hidden_dim']
        self.inception_num = config['inception_num']
        self.layer_num = config['ld_layer_num']
        self.stylized_layers = config['stylized_layers']
        self._check_stylized_layers()
        self.build_encoders()
        self.build_decoders()
        if self.config['resume']:
            checkpoint_path = self.config['checkpoint_path']
            self.begin = int(os.path.splitext(os.path.basename(checkpoint_path))[0])
            self.load_state_dict(torch.load(checkpoint_path, weights_only=True), strict=True)

    def _check_stylized_layers(self):
        if self.stylized_layers < self.layer_num:
            raise ValueError(
                f"LDMSAdaINRPNet: stylized_layers ({self.stylized_layers}) < ld_layer_num "
                f"({self.layer_num}) cannot be decoded (adain_rp.py:543-552 adds a list to a "
                "tensor)")

    def build_encoders(self):
        hidden_dim = self.hidden_dim
        for name in ('small', 'big'):
            setattr(self, f'rp_enc0_{name}_revf',
                    Conv2dBlock(3, hidden_dim, 3, 1, 1, inception_num=self.inception_num))
        for i in range(self.layer_num - 1):
            hidden_dim *= 2
            setattr(self, f'rp_enc{i + 1}_small_revf',
                    Conv2dBlock(hidden_dim, hidden_dim, 3, 1, 1, inception_num=self.inception_num))
            setattr(self, f'rp_enc{i + 1}_big_revf',
                    Conv2dBlock(hidden_dim, hidden_dim, 7, 1, 3, inception_num=self.inception_num))
        self.encoder_out_dim = hidden_dim

    def build_decoders(self):
        # stylized_layers >= ld_layer_num: every block reads a level-wide (2 x hidden) input
        hidden_dim = self.encoder_out_dim
        for i in range(self.layer_num - 1):
            setattr(self, f'rp_dec{i}',
                    Conv2dBlock(hidden_dim * 2, hidden_dim, 3, 1, 1,
                                inception_num=self.inception_num))
            hidden_dim //= 2
        setattr(self, f'rp_dec{self.layer_num - 1}',
                Conv2dBlock(hidden_dim * 2, 3, 3, 1, 1, inception_num=self.inception_num))

    _losses_entry = 'ld_losses'

    def _enc(self, i, name):
        return getattr(self, f'rp_enc{i}_{name}_revf')

    def _level_blocks(self, i):
        return [self._enc(i, 'small'), self._enc(i, 'big')]

    def _dec(self, k):
        return getattr(self, f'rp_dec{k}')

    def encode_rp_intermediate(self, input):
        results = [input]
        for i in range(self.layer_num):
            results.append(self._encode_level(i, results[-1]))
        return results[1:]

    def _encode_level(self, i, x, x2=None, n=None, stats=False):
        """Level i over x (or the batch [x; x2]): cat([small(x), big(x)], dim=1) without the
        cat. A 7x7 big branch whose block is the conv and its activation alone writes the upper
        half of the level tensor from its kernel; otherwise (level 0, inception 1x1s) the
        branch's output is copied in like the small one's. No level has epilogue statistics
        (a level is two kernels' output): _decode_fused takes them from the level."""
        assert not stats
        small = plan.run(plan.of(self._enc(i, 'small')), x, x2=x2)
        b, c, h, w = small.shape
        level = torch.empty((b, 2 * c, h, w), device=small.device, dtype=torch.float32)
        level[:, :c].copy_(small)
        steps = plan.of(self._enc(i, 'big'))
        if len(steps) == 1 and plan.is_k7(steps[0]):
            plan.conv(steps[0], x, out=level, out_channel_offset=c, x2=x2)
        else:
            level[:, c:].copy_(plan.run(steps, x, x2=x2))
        return level

    def _skip_block(self, i, stylized, stats, style_stats, want_stats=False):
        """rp_dec{i}(stylized + AdaIN(stylized, style)) with the sum formed in the block's
        first conv loader; stats = calc_mean_std(stylized), style_stats that of the style
        level. want_stats: also calc_mean_std of the result (from the last conv's epilogue
        unless that conv is the skip-AdaIN one, which has none) -> (y, mean, std)."""
        steps = plan.of(self._dec(i))
        aux = ops.adain_params(stats[0], stats[1], style_stats[0], style_stats[1])
        epilogue = want_stats and len(steps) > 1
        y = plan.run(steps, stylized, first_aux=aux, first_in_op=ops.IN_ADD_ADAIN,
                     first_content=stylized, stats_last=epilogue)
        if want_stats and not epilogue:
            return (y,) + tuple(ops.calc_mean_std(y))
        return y

    def _decode_fused(self, content, style, n):
        feats = self._encode_pair(content, style)
        mean, std = ops.calc_mean_std(feats[-1])
        last = self.layer_num == 1
        y = plan.run(plan.of(self.rp_dec0), feats[-1][:n],
                     first_aux=ops.adain_params(mean[:n], std[:n], mean[n:], std[n:]),
                     first_in_op=ops.IN_ADAIN, stats_last=not last)
        for i, f in enumerate(feats[:-1][::-1]):
            y, ym, ys = y
            y = self._skip_block(i + 1, y, (ym, ys), ops.calc_mean_std(f[n:]),
                                 want_stats=i < self.layer_num - 2)
        return y

    def _decode_skip(self, k, stylized, content_feat, style_feat):
        """rp_dec{k}(stylized + AdaIN(stylized, style_feat)) (adain_rp.py:550)."""
        return self._skip_block(k, stylized, calc_mean_std(stylized), calc_mean_std(style_feat))

    def save(self, save_path, iterations=0):
        torch.save(self.state_dict(), save_path)


class LDMSAdaINRPNet4(LDMSAdaINRPNet):
    """Two-encoder multi-scale AdaIN-RP with a concat decoder (adain_rp.py:711-819; `network:
    ld_adain4`). A fine chain of Conv2dBlocks (rp_enc{i}_small_revf, 3 -> h -> h ...) keeps the
    image size; a coarse chain of Sequentials (rp_enc{i}_big_revf: conv1x1, two reflect 3x3 +
    ReLU, ceil-mode 2x2 max-pool) halves it per level; the chains never mix. Level i is
    cat([fine_i, nearest(coarse_i -> H x W)]), 2h channels. decode() starts from
    rp_dec0(F(c[-1], s[-1])) and feeds every later block cat([stylized, F(c_i, s_i)]), F being
    AdaIN or, with use_mask, the per-label AdaIN. stylized_layers sets the decoder widths only
    (build_decoders); every 1 <= stylized_layers <= ld_layer_num decodes.

    test() without masks runs both chains once over [content; style]; the fine blocks emit
    their statistics from the last conv's epilogue, every coarse level's come from
    ops.resized_mean_std (the small map weighted by its replication counts), and ops.ld4_fuse
    writes each decoder block's whole input in one pass: no level tensor, no resized coarse
    map, no AdaIN output and no concatenation is written on the way. encode_rp_intermediate(),
    decode() and the masked route build the levels (fine half copied, coarse half written by
    ops.resize_nearest) and concatenate in front of each block.

    Deviations from the reference, where it cannot run: stylized_layers outside
    [1, ld_layer_num] raises ValueError at construction (it builds decoder widths that decode()
    cannot feed), `resume` as in LDMSAdaINRPNet. Inference only: forward() with autograd
    enabled raises."""

    def _check_stylized_layers(self):
        if not 1 <= self.stylized_layers <= self.layer_num:
            raise ValueError(
                f"LDMSAdaINRPNet4: stylized_layers ({self.stylized_layers}) outside "
                f"[1, ld_layer_num = {self.layer_num}] builds decoder widths that decode() cannot "
                "feed (adain_rp.py:751-798)")

    def build_encoders(self):
        hidden_dim = self.hidden_dim
        for i in range(self.layer_num):
            in_dim = 3 if i == 0 else hidden_dim
            setattr(self, f'rp_enc{i}_small_revf',
                    Conv2dBlock(in_dim, hidden_dim, 3, 1, 1, inception_num=self.inception_num))
            setattr(self, f'rp_enc{i}_big_revf', nn.Sequential(
                nn.Conv2d(in_dim, hidden_dim, (1, 1)),
                nn.ReflectionPad2d((1, 1, 1, 1)), nn.Conv2d(hidden_dim, hidden_dim, (3, 3)),
                nn.ReLU(),
                nn.ReflectionPad2d((1, 1, 1, 1)), nn.Conv2d(hidden_dim, hidden_dim, (3, 3)),
                nn.ReLU(),
                nn.MaxPool2d((2, 2), (2, 2), (0, 0), ceil_mode=True)))
        self.encoder_out_dim = hidden_dim

    def build_decoders(self):
        # block k reads what block k - 1 writes plus a level (2h); blocks before
        # stylized_layers - 1 write 2h channels, the later ones h, the last one the image
        h, prev = self.encoder_out_dim, 0
        for k in range(self.layer_num):
            out = 3 if k == self.layer_num - 1 else (2 * h if k < self.stylized_layers - 1 else h)
            setattr(self, f'rp_dec{k}',
                    Conv2dBlock(prev + 2 * h, out, 3, 1, 1, inception_num=self.inception_num))
            prev = out

    def _has_attention(self):
        return False

    def _chains(self, x, x2=None, stats=False):
        """Both encoder chains over x (or the batch [x; x2], read in place) -> per level
        (fine, coarse), or with stats (fine, mean, std, coarse): calc_mean_std of fine from its
        last conv's epilogue."""
        fine, coarse, f2, c2, out = x, x, x2, x2, []
        for i in range(self.layer_num):
            fine = plan.run(plan.of(self._enc(i, 'small')), fine, x2=f2, stats_last=stats)
            coarse = plan.run(plan.of(self._enc(i, 'big')), coarse, x2=c2)
            out.append((*fine, coarse) if stats else (fine, coarse))
            if stats:
                fine = fine[0]
            f2 = c2 = None
        return out

    def _levels(self, x, x2=None):
        """cat([fine_i, interpolate(coarse_i, size)], dim=1) per level without the cat: the fine
        half is one strided copy, the coarse half is written by the resize kernel."""
        levels = []
        for fine, coarse in self._chains(x, x2):
            b, c, h, w = fine.shape
            level = torch.empty((b, 2 * c, h, w), device=fine.device, dtype=torch.float32)
            level[:, :c].copy_(fine)
            levels.append(ops.resize_nearest(coarse, (h, w), out=level, out_channel_offset=c))
        return levels

    def encode_rp_intermediate(self, input):
        return self._levels(input)

    def _encode_pair(self, content, style, stats=False):
        assert not stats
        return self._levels(content, style)

    def _decode_fused(self, content, style, n):
        size = content.shape[2:]
        y = None
        for k, (fine, fm, fs, coarse) in enumerate(self._chains(content, style, stats=True)[::-1]):
            cm, cs = ops.resized_mean_std(coarse, size)
            y = ops.ld4_fuse(y, fine, coarse, ops.adain_params(fm[:n], fs[:n], fm[n:], fs[n:]),
                             ops.adain_params(cm[:n], cs[:n], cm[n:], cs[n:]), n=n)
            y = plan.run(plan.of(self._dec(k)), y)
        return y

    def decode(self, content_feats, style_feats, use_mask=False, c_mask_path=None, s_mask_path=None):
        """adain_rp.py:780-799, op by op: AdaIN (or the per-label AdaIN) of every level, then
        each block on cat([stylized, that])."""
        self._kernel_path_check()
        if use_mask:
            # all levels share H x W: decode the masks and plan the labels once
            n, dev = content_feats[-1].shape[0], content_feats[-1].device
            c_seg = segment_maps(c_mask_path, n, content_feats[-1].shape[2:], dev)
            s_seg = segment_maps(s_mask_path, n, style_feats[-1].shape[2:], dev)
            seg_plan = ops.segment_plan(c_seg, s_seg)

            def fuse(c, s):
                return masked_adain_batch(c, s, c_seg, s_seg, plan=seg_plan)[0]
        else:
            fuse = AdaIN
        stylized = self._dec(0)(fuse(content_feats[-1], style_feats[-1]))
        pairs = list(zip(content_feats[:-1], style_feats[:-1]))[::-1]
        for i, (content_feat, style_feat) in enumerate(pairs):
            stylized = self._dec(i + 1)(torch.cat([stylized, fuse(content_feat, style_feat)],
                                                  dim=1))
        return stylized

    def forward(self, content, style, alpha=1.0):
        """The loss dict of adain_rp.py:322-345 under no_grad, op by op through
        encode_rp_intermediate / decode; with autograd enabled and trainable parameters it
        raises: ld_adain4 training is not built."""
        self._kernel_path_check()
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError(
                "LDMSAdaINRPNet4: ld_adain4 training is not built (inference only: test / "
                "decode / forward under torch.no_grad())")
        return super().forward(content, style, alpha)
