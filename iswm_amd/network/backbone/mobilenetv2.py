"""Dilated MobileNetV2 backbone on the HIP execution layer.

The reference has no MobileNet: the module tree, the [t, c, n, s] table and the stride-to-dilation rule
are those of the public MobileNetV2 / DeepLabV3Plus-Pytorch definition, so the widely used checkpoints of that family
load by key.  Forward / backward run as libiswm_hip.so kernels through ``_hip.cba_fwd`` / ``cba_bwd``; the depthwise
3x3 -> BatchNorm -> ReLU6 stage is csrc/dwconv3.hip.  The final 1x1 conv to 1280 channels and the ImageNet classifier
are not part of a segmentation backbone and are not built.
"""
import torch.nn as nn

from .. import _hip
from ... import ops
from ...ops import Act

__all__ = ['MobileNetV2', 'InvertedResidual', 'mobilenet_v2']

SETTINGS = [
    # t, c, n, s
    [1, 16, 1, 1],
    [6, 24, 2, 2],
    [6, 32, 3, 2],
    [6, 64, 4, 2],
    [6, 96, 3, 1],
    [6, 160, 3, 2],
    [6, 320, 1, 1],
]


class PointwiseConv2d(_hip.Conv2d):
    """1x1 conv of an inverted-residual block.  Its input buffer is the stage in front of it as that stage wrote it
    (a BatchNorm over exactly in_channels channels), so the input is padded to groups of 4 only -- never to the next
    multiple of 32 as _hip.pad_cin does for the decoder's concatenation buffer (144 hidden channels stay 144)."""

    @property
    def cin_p(self):
        return _hip.pad4(self.in_channels)


class InvertedResidual(_hip.HipModule):
    """conv = [1x1 expand, BN, ReLU6]? + [3x3 depthwise (stride, padding = dilation), BN, ReLU6] + [1x1 project, BN];
    the input is added (no activation) when stride == 1 and inp == oup"""

    def __init__(self, inp, oup, stride, dilation, expand_ratio):
        super(InvertedResidual, self).__init__()
        if stride not in (1, 2):
            raise ValueError("stride must be 1 or 2")
        self.stride = stride
        self.use_res_connect = stride == 1 and inp == oup
        hidden = int(round(inp * expand_ratio))
        layers = []
        if expand_ratio != 1:
            layers += [PointwiseConv2d(inp, hidden, 1, 1, 0, bias=False), _hip.BatchNorm2d(hidden), _hip.ReLU6(inplace=True)]
        layers += [
            _hip.DepthwiseConv2d(hidden, hidden, 3, stride, dilation, dilation=dilation, groups=hidden, bias=False),
            _hip.BatchNorm2d(hidden),
            _hip.ReLU6(inplace=True),
            PointwiseConv2d(hidden, oup, 1, 1, 0, bias=False),
            _hip.BatchNorm2d(oup),
        ]
        self.conv = nn.Sequential(*layers)
        self.expand = expand_ratio != 1
        self._saved = None

    def _stages(self):
        m = list(self.conv)
        st = []
        if self.expand:
            st.append(_hip.Stage("cba", m[0], m[1], Act.RELU6))
            m = m[3:]
        st.append(_hip.Stage("cba", m[0], m[1], Act.RELU6))
        st.append(_hip.Stage("cba", m[3], m[4], Act.NONE))
        return st

    def fwd(self, x, save):
        st = self._stages()
        ctxs = []
        h = x
        for k, s in enumerate(st):
            last = k == len(st) - 1
            # the depthwise kernels read fp32; the depthwise stage's own output goes pre-split to the projection when the
            # planes kernels take it, and the block's output follows its channel count (the next block's 1x1 reads it)
            fmt = "f32" if (not last and isinstance(st[k + 1].conv, _hip.DepthwiseConv2d)) else None
            h, c = _hip.cba_fwd(s.conv, s.bn, s.act, h, save, residual=x if (last and self.use_res_connect) else None,
                                out_fmt=fmt)
            ctxs.append(c)
        _hip.keep(self, save, ctxs)
        return h

    def bwd(self, dout, sink):
        ctxs = _hip.take(self, sink)
        dres = None
        if self.use_res_connect:
            # no activation after the add: the gradient of the identity branch IS the incoming gradient (the last stage is asked
            # for none, want_dres=False); the first stage's data gradient accumulates into it
            dout = dres = ops.as_f32(dout)
        d = dout
        for k in range(len(ctxs) - 1, 0, -1):
            d, _ = _hip.cba_bwd(ctxs[k], d, sink, want_dres=False)
        dx, _ = _hip.cba_bwd(ctxs[0], d, sink, dx=dres, accumulate=dres is not None)
        return dx

    def out_channels_of(self, cin):
        return list(self.conv)[-2].out_channels


class MobileNetV2(_hip.HipModule):
    def __init__(self, output_stride=8, width_mult=1.0):
        super(MobileNetV2, self).__init__()
        if width_mult != 1.0:
            raise NotImplementedError("HIP MobileNetV2 covers width_mult == 1")
        if output_stride not in (8, 16):
            raise ValueError("output_stride must be 8 or 16")
        self.output_stride = output_stride
        input_channel = 32
        current_stride = 1
        features = [_hip.HipSequential(_hip.Conv2d(3, input_channel, 3, 2, 1, bias=False), _hip.BatchNorm2d(input_channel),
                                       _hip.ReLU6(inplace=True))]
        current_stride *= 2
        dilation = 1
        for t, c, n, s in SETTINGS:
            previous_dilation = dilation
            if current_stride == output_stride:
                stride = 1
                dilation *= s
            else:
                stride = s
                current_stride *= s
            for i in range(n):
                if i == 0:
                    features.append(InvertedResidual(input_channel, c, stride, previous_dilation, t))
                else:
                    features.append(InvertedResidual(input_channel, c, 1, dilation, t))
                input_channel = c
        self.features = _hip.HipSequential(*features)
        self.out_channels = input_channel

        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out')
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)

    def forward(self, x):
        raise NotImplementedError("the ImageNet classification head is not on the segmentation hot path; wrap the "
                                  "backbone in network.utils.IntermediateLayerGetter")


def mobilenet_v2(pretrained=False, progress=True, **kwargs):
    model = MobileNetV2(**kwargs)
    if pretrained:
        # the public definition downloads ImageNet weights here; there is no network in this deployment
        raise RuntimeError("pretrained=True needs a download; load a checkpoint with load_state_dict instead")
    return model
