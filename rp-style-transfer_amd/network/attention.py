"""Drop-in for the reference's network/attention.py SE modules, on MI355X kernels.

  SELayer        network/attention.py:5-22
  SEBottleneck   network/attention.py:25-66
Same constructors, attribute names and state_dict keys (conv1/bn1/conv2/bn2/conv3/bn3,
se.fc.0 / se.fc.2). The kernel path is the inference one: the BatchNorms use their running
statistics and fold into the convs before them (rpst.plan.se_folded), and the block runs as
three conv launches plus the gate (rpst.ops.se_bottleneck). Training-mode BatchNorm (batch
statistics, running-stat updates) has no rpst kernel and raises. SKLayer / SKBottleneck are
not built.
"""
from __future__ import annotations

import torch.nn as nn

from rpst import ops


class SELayer(nn.Module):
    """Squeeze-and-excitation gate (attention.py:5-22). Inside an SEBottleneck its pool and
    its two Linear layers run in rpst_se_gate and its scaling in the gated conv's epilogue;
    called on its own it has no kernel."""

    def __init__(self, channel, reduction=16):
        super(SELayer, self).__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Sequential(
            nn.Linear(channel, channel // reduction, bias=False),
            nn.ReLU(inplace=True),
            nn.Linear(channel // reduction, channel, bias=False),
            nn.Sigmoid()
        )
        self.attention_map = None

    def forward(self, x):
        raise NotImplementedError(
            "SELayer: the stand-alone layer has no rpst kernel; it runs fused inside "
            "SEBottleneck (rpst.ops.se_bottleneck)")


class SEBottleneck(nn.Module):
    """conv1x1-bn-relu, conv3x3-bn-relu, conv1x1-bn, SE gate, + x, relu (attention.py:25-66)
    with inplanes == planes, stride 1, no downsample: the form Conv2dBlock builds
    (base.py:177-179)."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1,
                 base_width=64, dilation=1, norm_layer=None,
                 *, reduction=16):
        super(SEBottleneck, self).__init__()
        if inplanes != planes or stride != 1 or downsample is not None:
            raise NotImplementedError(
                "SEBottleneck: only inplanes == planes, stride 1, no downsample has an rpst "
                "kernel (the form Conv2dBlock(attention='se') builds)")
        if planes // reduction < 1:
            raise NotImplementedError(
                f"SEBottleneck: {planes} channels give a zero-width squeeze (planes // "
                f"{reduction} == 0, every gate exactly 0.5); it has no rpst kernel")
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride,
                               padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.se = SELayer(planes, reduction)
        self.downsample = downsample
        self.stride = stride
        self.attention_map = None

    def forward(self, x):
        if self.training:
            raise NotImplementedError(
                "SEBottleneck: training-mode BatchNorm (batch statistics) has no rpst kernel; "
                "the SE path is inference only (call .eval(), as test() does)")
        out, gate = ops.se_bottleneck(x, self)
        self.se.attention_map = gate
        self.attention_map = gate
        return out
