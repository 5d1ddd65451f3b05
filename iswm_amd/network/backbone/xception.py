"""Dilated Xception backbone on the HIP execution layer -- counterpart of the reference's network/backbone/xception.py
(the DeepLab form: four replace_stride_with_dilation entries, a dilation per Block), same module tree and state_dict keys.

A unit is [ReLU-on-load?] depthwise 3x3 -> pointwise 1x1 -> BatchNorm (-> ReLU):
  * the depthwise half is iswm_dwconv3x3_pre_fwd / _pre_bwd (csrc/dwconv3.hip): it rectifies on load where the unit opens a
    block (the residual stream itself stays un-rectified for the skip path), writes the pointwise conv's operand pre-split
    at the pointwise conv's input pitch with the padding columns zeroed, and its one-launch backward masks dx by x > 0;
  * pointwise -> BatchNorm (-> ReLU, + residual) is the fused stage of _hip.cba_fwd; the ReLU behind a BatchNorm inside
    `rep` belongs to that BatchNorm's apply pass.
The block's sum rides on a BatchNorm apply pass: the last unit's in identity blocks, `skipbn`'s (taking the main branch,
max-pooled in strided blocks) otherwise.  Backward: the skip gradient is the incoming gradient and the first unit's masked
data gradient accumulates into it.

728 channels: the pointwise convs read a 768-wide buffer (12 x 64: the planes kernels gather 64 channels per chunk; 736
would leave them to the fp32-operand kernels), so the depthwise kernel's quads cover 192 columns, no idle-lane fallback.
conv3 / conv4 pad by 1 under dilation 2 (output stride 16) or 4 (output stride 8), as the public definition does: the map
shrinks by 2 (dil - 1) per convolution and checkpoints depend on it.
"""
import torch.nn as nn

from .. import _hip
from ... import ops
from ...ops import Act
from .resnet import MaxPool2d as _StemMaxPool2d

__all__ = ['Xception', 'Block', 'SeparableConv2d', 'xception']


class PointwiseConv2d(_hip.Conv2d):
    """1x1 conv behind a depthwise conv: its input buffer is written by the depthwise kernel, which zero-fills up to the
    pitch -- wide inputs go up to the next multiple of 64 so that the planes kernels take them (728 -> 768)"""

    @property
    def cin_p(self):
        c = self.in_channels
        return _hip.pad4(c) if c < 128 else (c + 63) // 64 * 64


class SkipConv2d(_hip.Conv2d):
    """1x1 conv of a block's skip path: it reads the residual stream as the block in front wrote it (exactly in_channels
    channels), so its input is padded to groups of 4 only"""

    @property
    def cin_p(self):
        return _hip.pad4(self.in_channels)


class MaxPool2d(_StemMaxPool2d):
    """the 3x3 / stride 2 / pad 1 pool that ends a strided block; its output is the residual operand of skipbn's apply
    pass, which reads fp32"""

    def fwd(self, x, save):
        if (self.kernel_size, self.stride, self.padding) != (3, 2, 1):
            raise NotImplementedError("HIP max-pool is 3x3 / stride 2 / pad 1")
        y, idx = ops.maxpool_fwd(x, planes=False)
        if _hip.POOL_RECORDER is not None:
            _hip.POOL_RECORDER[self] = idx
        _hip.keep(self, save, (idx, tuple(x.shape)))
        return y


class SeparableConv2d(_hip.HipModule):
    """conv1 (depthwise 3x3, stride 1, 1 <= padding <= dilation) -> pointwise (1x1), no bias"""

    def __init__(self, in_channels, out_channels, kernel_size=1, stride=1, padding=0, dilation=1, bias=False):
        super(SeparableConv2d, self).__init__()
        if kernel_size != 3 or stride != 1 or bias or not 1 <= padding <= dilation:
            raise NotImplementedError("HIP SeparableConv2d covers 3x3, stride 1, 1 <= padding <= dilation, no bias")
        self.conv1 = _hip.DepthwiseConv2d(in_channels, in_channels, kernel_size, stride, padding, dilation,
                                          groups=in_channels, bias=bias)
        self.pointwise = PointwiseConv2d(in_channels, out_channels, 1, 1, 0, 1, 1, bias=bias)
        self._saved = None

    def dw_fwd(self, x, save, relu_in):
        """the depthwise half: the pointwise conv's operand [N, Ho, Wo, pointwise.cin_p], pre-split when its kernel takes planes"""
        dw, pw = self.conv1, self.pointwise
        x = ops.as_f32(x)
        c, cp = dw.in_channels, pw.cin_p
        if x.shape[3] != c:
            raise ValueError("separable conv over %d channels got a %d-channel buffer" % (c, x.shape[3]))
        g = ops.ConvGeom(x, c, 3, 3, 1, dw.padding[0], dw.dilation[0])
        if g.ho < 1 or g.wo < 1:
            raise ValueError("a %d x %d map has no output under dilation %d, padding %d" % (g.h, g.w, g.dil, g.pad))
        if ops.planes_conv_ok(cp, pw.cout_p, 0):
            mid = ops.new_planes(g.n, g.ho, g.wo, cp, x.device)
        else:
            mid = ops.new_act(g.n, g.ho, g.wo, cp, x.device)
        ops.dwconv3x3_pre_fwd(x, dw.weight.contiguous(), g, relu_in, out=mid[..., 0:c] if cp > c else mid)
        _hip.keep(dw, save, (x, g, relu_in))
        return mid

    def dw_bwd(self, dmid, sink, need_dx=True, dx=None, accumulate=False):
        """backward of dw_fwd from the gradient of the pointwise conv's operand: the depthwise weight gradient into the sink,
        returns dx (masked by x > 0 where the forward rectified on load; accumulating into `dx` when asked)"""
        dw = self.conv1
        x, g, relu_in = _hip.take(dw, sink)
        c = dw.in_channels
        dmid = ops.as_f32(dmid)
        dy = dmid[..., :c] if dmid.shape[3] > c else dmid
        need_dw, buf, tgt = dw.weight.requires_grad, None, None
        if need_dw:
            buf = sink.target(dw.weight)
            tgt = buf if buf.is_contiguous() else None
        if not (need_dx or need_dw):
            return None
        dx, dwg = ops.dwconv3x3_pre_bwd(x, dy, dw.weight.contiguous(), g, c, relu_in, dx, accumulate, tgt, need_dx, need_dw)
        if need_dw:
            if tgt is None:
                buf.copy_(dwg)
            sink.done(dw.weight)
        return dx

    # -- the bare separable conv (conv4: no BatchNorm behind it inside the segmentation backbone) ------------------------
    def fwd(self, x, save):
        return self.pointwise.fwd(self.dw_fwd(x, save, False), save)

    def bwd(self, dy, sink, need_dx=True, dx=None, accumulate=False):
        return self.dw_bwd(self.pointwise.bwd(ops.as_f32(dy), sink), sink, need_dx, dx, accumulate)

    def out_channels_of(self, cin):
        return self.pointwise.out_channels


def unit_fwd(sep, bn, act, x, save, relu_in=False, residual=None):
    """[ReLU-on-load?] depthwise -> pointwise -> BatchNorm (+ residual) (-> act): (out fp32, stage context)"""
    return _hip.cba_fwd(sep.pointwise, bn, act, sep.dw_fwd(x, save, relu_in), save, residual=residual, out_fmt="f32")


def unit_bwd(sep, ctx, dout, sink, need_dx=True, dx=None, accumulate=False):
    dmid, _ = _hip.cba_bwd(ctx, dout, sink, want_dres=False)
    return sep.dw_bwd(dmid, sink, need_dx, dx, accumulate)


class Block(_hip.HipModule):
    """`reps` units (rep: [ReLU, SeparableConv2d, BatchNorm2d] each, the first ReLU dropped when not start_with_relu, a
    MaxPool2d(3, strides, 1) appended when strides != 1) plus the skip path (skip 1x1 conv at `strides` + skipbn) when the
    shape changes, the identity otherwise; the two are added with no activation behind the sum"""

    def __init__(self, in_filters, out_filters, reps, strides=1, start_with_relu=True, grow_first=True, dilation=1):
        super(Block, self).__init__()
        if strides not in (1, 2):
            raise ValueError("strides must be 1 or 2")
        if out_filters != in_filters or strides != 1:
            self.skip = SkipConv2d(in_filters, out_filters, 1, stride=strides, bias=False)
            self.skipbn = _hip.BatchNorm2d(out_filters)
        else:
            self.skip = None
        same = [(out_filters, out_filters) if grow_first else (in_filters, in_filters)] * (reps - 1)
        widths = [(in_filters, out_filters)] + same if grow_first else same + [(in_filters, out_filters)]
        rep = []
        for k, (cin, cout) in enumerate(widths):
            if k > 0 or start_with_relu:
                rep.append(_hip.ReLU(inplace=k > 0))
            rep.append(SeparableConv2d(cin, cout, 3, stride=1, padding=dilation, dilation=dilation, bias=False))
            rep.append(_hip.BatchNorm2d(cout))
        if strides != 1:
            rep.append(MaxPool2d(3, strides, 1))
        self.rep = nn.Sequential(*rep)
        self._saved = None

    def _units(self):
        """([(SeparableConv2d, BatchNorm2d, Act behind the BatchNorm)], the ReLU module the first unit rectifies on load with or
        None, the MaxPool2d or None)"""
        units, first_relu, pool, pending = [], None, None, None
        for m in self.rep:
            if isinstance(m, nn.ReLU):
                pending = m
            elif isinstance(m, SeparableConv2d):
                if pending is not None and units:
                    units[-1][2] = Act.RELU                  # the ReLU between two units: the BatchNorm apply pass in front of it
                elif pending is not None:
                    first_relu = pending
                pending = None
                units.append([m, None, Act.NONE])
            elif isinstance(m, nn.BatchNorm2d):
                units[-1][1] = m
            elif isinstance(m, nn.MaxPool2d):
                pool = m
            else:
                raise NotImplementedError("no HIP implementation for %s inside a Block" % type(m).__name__)
        return units, first_relu, pool

    def fwd(self, x, save):
        units, first_relu, pool = self._units()
        x = ops.as_f32(x)
        if _hip.MASK_RECORDER is not None and first_relu is not None:
            _hip.MASK_RECORDER[first_relu] = x > 0
        h, ctxs = x, []
        for k, (sep, bn, act) in enumerate(units):
            res = x if (k == len(units) - 1 and self.skip is None) else None
            h, c = unit_fwd(sep, bn, act, h, save, relu_in=(k == 0 and first_relu is not None), residual=res)
            ctxs.append(c)
        cs = None
        if self.skip is not None:
            if pool is not None:
                h = pool.fwd(h, save)
            h, cs = _hip.cba_fwd(self.skip, self.skipbn, Act.NONE, x, save, residual=h, out_fmt="f32")
        _hip.keep(self, save, (units, pool, ctxs, cs))
        return h

    def bwd(self, dout, sink, need_dx=True):
        units, pool, ctxs, cs = _hip.take(self, sink)
        dout = ops.as_f32(dout)
        d = dout
        if cs is not None and pool is not None:
            d = pool.bwd(d, sink)
        for k in range(len(units) - 1, 0, -1):
            d = unit_bwd(units[k][0], ctxs[k], d, sink)
        if cs is None:
            # the gradient of the identity path IS the incoming gradient; the first unit's masked dx accumulates into it
            return unit_bwd(units[0][0], ctxs[0], d, sink, True, dout, True)
        dx = unit_bwd(units[0][0], ctxs[0], d, sink, need_dx)
        dx, _ = _hip.cba_bwd(cs, dout, sink, need_dx=need_dx, dx=dx, accumulate=dx is not None, want_dres=False)
        return dx

    def out_channels_of(self, cin):
        return self._units()[0][-1][0].pointwise.out_channels


class Xception(_hip.HipModule):
    """conv1 bn1 relu1 conv2 bn2 relu2 block1..block12 conv3 bn3 relu3 conv4 bn4 (no fc: the ImageNet classifier is not part
    of a segmentation backbone).  network.utils.IntermediateLayerGetter walks the children through walk_fwd / walk_bwd."""

    def __init__(self, replace_stride_with_dilation=None):
        super(Xception, self).__init__()
        self.dilation = 1
        if replace_stride_with_dilation is None:
            replace_stride_with_dilation = [False, False, False, False]
        if len(replace_stride_with_dilation) != 4:
            raise ValueError("replace_stride_with_dilation should be None "
                             "or a 4-element tuple, got {}".format(replace_stride_with_dilation))
        r = replace_stride_with_dilation
        self.conv1 = _hip.Conv2d(3, 32, 3, 2, 0, bias=False)
        self.bn1 = _hip.BatchNorm2d(32)
        self.relu1 = _hip.ReLU(inplace=True)
        self.conv2 = _hip.Conv2d(32, 64, 3, bias=False)
        self.bn2 = _hip.BatchNorm2d(64)
        self.relu2 = _hip.ReLU(inplace=True)
        self.block1 = self._make_block(64, 128, 2, 2, start_with_relu=False, grow_first=True, dilate=r[0])
        self.block2 = self._make_block(128, 256, 2, 2, start_with_relu=True, grow_first=True, dilate=r[1])
        self.block3 = self._make_block(256, 728, 2, 2, start_with_relu=True, grow_first=True, dilate=r[2])
        for k in range(4, 12):
            setattr(self, "block%d" % k, self._make_block(728, 728, 3, 1, start_with_relu=True, grow_first=True, dilate=r[2]))
        self.block12 = self._make_block(728, 1024, 2, 2, start_with_relu=True, grow_first=False, dilate=r[3])
        self.conv3 = SeparableConv2d(1024, 1536, 3, 1, 1, dilation=self.dilation)
        self.bn3 = _hip.BatchNorm2d(1536)
        self.relu3 = _hip.ReLU(inplace=True)
        self.conv4 = SeparableConv2d(1536, 2048, 3, 1, 1, dilation=self.dilation)
        self.bn4 = _hip.BatchNorm2d(2048)

    def _make_block(self, in_filters, out_filters, reps, strides=1, start_with_relu=True, grow_first=True, dilate=False):
        if dilate:
            self.dilation *= strides
            strides = 1
        return Block(in_filters, out_filters, reps, strides, start_with_relu=start_with_relu, grow_first=grow_first,
                     dilation=self.dilation)

    def forward(self, x):
        raise NotImplementedError("the ImageNet classification head is not on the segmentation hot path; wrap the "
                                  "backbone in network.utils.IntermediateLayerGetter")


FUSED_INTO = {"bn1": "conv1", "relu1": "conv1", "bn2": "conv2", "relu2": "conv2", "bn3": "conv3", "relu3": "conv3"}


def walk_fwd(getter, x, save):
    """IntermediateLayerGetter.fwd over an Xception's children: the stem stages conv1 / conv2 (+ BatchNorm + ReLU), the blocks,
    conv3 / bn3 / relu3 as one unit, conv4 as a bare separable conv.  A feature tapped at a fused child (relu2, bn3, ...) is
    the output of the stage it belongs to only where that stage ends there; the DeepLab heads tap block1 and conv4."""
    out, ctxs = {}, {}
    for name, module in getter.named_children():
        if name in ("conv1", "conv2"):
            x, ctxs[name] = _hip.cba_fwd(module, getter["bn" + name[-1]], Act.RELU, x, save, out_fmt="f32")
        elif name == "conv3":
            x, ctxs[name] = unit_fwd(module, getter["bn3"], Act.RELU, x, save)
        elif name in FUSED_INTO:
            pass
        else:
            x = module.fwd(x, save)
        if name in getter.return_layers:
            if name in FUSED_INTO and name[:4] != "relu":
                raise NotImplementedError("cannot tap %s: it is fused with the ReLU behind it" % name)
            if name in ("conv1", "conv2", "conv3"):
                raise NotImplementedError("cannot tap %s: it is fused with the BatchNorm behind it" % name)
            out[getter.return_layers[name]] = x
    return out, ctxs


def walk_bwd(getter, ctxs, dfeats, sink, need_dx):
    """backward of walk_fwd; need_dx: whether the image gradient is wanted (the stem's first conv computes none otherwise)"""
    inv = {v: k for k, v in getter.return_layers.items()}
    tap = {inv[k]: g for k, g in dfeats.items() if g is not None}
    dy = None
    for name in reversed([n for n, _ in getter.named_children()]):
        if name in tap:
            g = ops.as_f32(tap.pop(name))
            dy = g if dy is None else ops.add_inplace(dy, g)
        if name in FUSED_INTO:
            continue
        module = getter[name]
        if name == "conv1":
            dy, _ = _hip.cba_bwd(ctxs[name], dy, sink, need_dx=need_dx)
        elif name == "conv2":
            dy, _ = _hip.cba_bwd(ctxs[name], dy, sink)
        elif name == "conv3":
            dy = unit_bwd(module, ctxs[name], dy, sink)
        else:
            dy = module.bwd(dy, sink)
    return dy


def xception(pretrained=False, progress=True, **kwargs):
    model = Xception(**kwargs)
    if pretrained:
        # the public definition downloads ImageNet weights here; there is no network in this deployment
        raise RuntimeError("pretrained=True needs a download; load a checkpoint with load_state_dict instead")
    return model
