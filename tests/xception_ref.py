"""Stock-torch restatement of the Xception DeepLab models, the parity reference of tests/test_xception_*.py.

Written from the specification of the public dilated Xception (the DeepLab form the reference ships in
network/backbone/xception.py) in plain ``nn.Conv2d`` / ``nn.BatchNorm2d`` / ``nn.MaxPool2d``-equivalent modules, any dtype
(the tests run it in float64 on the CPU), and not from iswm_amd's modules:

  * stem: conv1 3->32 3x3 stride 2 pad 0, bn1, relu1; conv2 32->64 3x3 pad 0, bn2, relu2;
  * separable conv(cin, cout, pad, dil): `conv1` depthwise 3x3 (groups = cin, stride 1, padding pad, dilation dil) then
    `pointwise` 1x1, neither biased;
  * block(cin, cout, reps, stride, start_with_relu, grow_first, dil): `rep` = reps x [ReLU, separable(pad = dil), BatchNorm]
    with widths cin->cout, cout->cout.. (grow_first) or cin->cin.., cin->cout (not), the first ReLU dropped when not
    start_with_relu, MaxPool(3, stride, 1) appended when stride != 1; `skip` 1x1 conv at the stride + `skipbn` when
    cin != cout or stride != 1, else the identity; output = rep(x) + skip path, no activation.  The first ReLU does NOT
    rectify the tensor the skip path reads;
  * dilation rule: dilation = 1; a block built with dilate=True multiplies dilation by its stride and takes stride 1;
    blocks: 1 (64->128, 2 reps, stride 2, no leading ReLU, dilate r[0]); 2 (128->256, 2, 2, r[1]); 3 (256->728, 2, 2, r[2]);
    4..11 (728->728, 3 reps, stride 1, r[2]); 12 (728->1024, 2, 2, not grow_first, r[3]);
  * conv3 = separable(1024, 1536, pad 1, dil = dilation), bn3, relu3; conv4 = separable(1536, 2048, pad 1, dil = dilation):
    padding stays 1 under dilation 2 / 4, so each shrinks the map by 2 (dil - 1);
  * the segmentation model taps block1 (128 channels, 'low_level') and conv4 itself ('out': no bn4, no ReLU);
    r = [F, F, F, T] with ASPP rates 6/12/18 at output stride 16, [F, F, T, T] with 12/24/36 at output stride 8.

Every ReLU is a "site": one behind a BatchNorm is named after that BatchNorm, a block's leading ReLU after itself.  Every
max-pool is a site named after itself.  ``Control`` (tests/mobilenet_ref.py) records pre-activations / pooled windows and
imposes another implementation's ReLU patterns and window choices.

The state comes from a deterministic numpy rule (numpy_state), so that a script outside this repository's Python
environment rebuilds the same weights from the list of names and shapes alone.
"""
import functools

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.mobilenet_ref import Control, HeadV3, HeadV3Plus, ReLU, synth_images, synth_labels, weighted_ce  # noqa: F401

# The state's seed.  Chosen on the CPU, from this restatement alone: of seeds 1..6 the one whose float32 evaluation stays closest
# to the float64 one in train mode on the GPU tests' inputs -- running statistics within 1.7e-6 / 5.9e-7 / 9.8e-7 for the three
# model cases (deeplabv3plus os 16, deeplabv3 os 16, deeplabv3plus os 8), six times under the tests' 1e-5, logits within
# 1.3e-5 / 5.9e-6 / 1.1e-5, and 5 / 2 / 8 of 5.1 / 4.2 / 12.4 million ReLU decisions differing; seed 2 gives 8.1e-6 / 1.2e-5 /
# 2.6e-6 on the statistics (torch's default thread count; the float32 sums depend on it).  tests/test_xception_cpu.py measures the
# first case again on one thread: 2.2e-6.
SEED = 5


class MaxPool(nn.Module):
    """3x3 / stride 2 / pad 1 max-pool that records which tap (kh * 3 + kw) it took per output element and, with
    ctl.pools, takes the imposed tap instead"""
    ctl, site = None, None

    def forward(self, x):
        n, c, h, w = x.shape
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        win = F.unfold(F.pad(x, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(n, c, 9, ho, wo)
        ctl = self.ctl
        own = win.argmax(2)
        if ctl is not None and ctl.preact is not None:
            ctl.preact[self.site] = win.detach()
        idx = own if (ctl is None or getattr(ctl, "pools", None) is None) else ctl.pools[self.site].long()
        return win.gather(2, idx.unsqueeze(2)).squeeze(2)


class Separable(nn.Module):
    def __init__(self, cin, cout, pad, dil):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cin, 3, 1, pad, dil, groups=cin, bias=False)
        self.pointwise = nn.Conv2d(cin, cout, 1, bias=False)

    def forward(self, x):
        return self.pointwise(self.conv1(x))


class Block(nn.Module):
    def __init__(self, cin, cout, reps, stride, start_with_relu, grow_first, dil):
        super().__init__()
        self.has_skip = cin != cout or stride != 1
        if self.has_skip:
            self.skip = nn.Conv2d(cin, cout, 1, stride, bias=False)
            self.skipbn = nn.BatchNorm2d(cout)
        widths = [(cin, cout)] + [(cout, cout)] * (reps - 1) if grow_first else [(cin, cin)] * (reps - 1) + [(cin, cout)]
        rep = []
        for a, b in widths:
            rep += [ReLU(inplace=False), Separable(a, b, dil, dil), nn.BatchNorm2d(b)]
        if not start_with_relu:
            rep = rep[1:]
        if stride != 1:
            rep.append(MaxPool())
        self.rep = nn.Sequential(*rep)

    def forward(self, x):
        return self.rep(x) + (self.skipbn(self.skip(x)) if self.has_skip else x)


class Backbone(nn.Module):
    def __init__(self, output_stride):
        super().__init__()
        r = [False, False, True, True] if output_stride == 8 else [False, False, False, True]
        self.conv1, self.bn1, self.relu1 = nn.Conv2d(3, 32, 3, 2, 0, bias=False), nn.BatchNorm2d(32), ReLU(inplace=False)
        self.conv2, self.bn2, self.relu2 = nn.Conv2d(32, 64, 3, bias=False), nn.BatchNorm2d(64), ReLU(inplace=False)
        dil = 1
        table = [(64, 128, 2, 2, False, True, r[0]), (128, 256, 2, 2, True, True, r[1]), (256, 728, 2, 2, True, True, r[2])] + \
                [(728, 728, 3, 1, True, True, r[2])] * 8 + [(728, 1024, 2, 2, True, False, r[3])]
        for k, (cin, cout, reps, stride, swr, grow, dilate) in enumerate(table):
            if dilate:
                dil, stride = dil * stride, 1
            setattr(self, "block%d" % (k + 1), Block(cin, cout, reps, stride, swr, grow, dil))
        self.conv3, self.bn3, self.relu3 = Separable(1024, 1536, 1, dil), nn.BatchNorm2d(1536), ReLU(inplace=False)
        self.conv4 = Separable(1536, 2048, 1, dil)

    def forward(self, x):
        x = self.relu2(self.bn2(self.conv2(self.relu1(self.bn1(self.conv1(x))))))
        low = x = self.block1(x)
        for k in range(2, 13):
            x = getattr(self, "block%d" % k)(x)
        return low, self.conv4(self.relu3(self.bn3(self.conv3(x))))


class RefDeepLab(nn.Module):
    """arch 'deeplabv3plus' | 'deeplabv3' over the Xception backbone; dropout p = 0 (the tests compare deterministic steps)"""

    def __init__(self, arch, num_classes, output_stride):
        super().__init__()
        rates = [12, 24, 36] if output_stride == 8 else [6, 12, 18]
        self.backbone = Backbone(output_stride)
        self.classifier = HeadV3Plus(2048, 128, num_classes, rates) if arch == 'deeplabv3plus' else HeadV3(2048, num_classes, rates)
        self.ctl = Control()
        self.ctl.pools = None
        names = {m: n for n, m in self.named_modules()}
        for k in (1, 2, 3):
            act = getattr(self.backbone, "relu%d" % k)
            act.site, act.ctl = "backbone.bn%d" % k, self.ctl
        for seq in self.modules():
            if isinstance(seq, nn.Sequential):
                ch = list(seq)
                for a, b in zip([None] + ch, ch):
                    if isinstance(b, ReLU):
                        b.site, b.ctl = (names[a] if isinstance(a, nn.BatchNorm2d) else names[b]), self.ctl
                    elif isinstance(b, MaxPool):
                        b.site, b.ctl = names[b], self.ctl
        self.tops = {m.site: None for m in self.modules() if isinstance(m, ReLU)}
        self.pool_sites = [m.site for m in self.modules() if isinstance(m, MaxPool)]
        assert None not in self.tops
        for m in self.modules():
            if isinstance(m, nn.Dropout):
                m.p = 0.0

    def forward(self, x):
        low, out = self.backbone(x)
        return F.interpolate(self.classifier(low, out), size=x.shape[2:], mode='bilinear', align_corners=False)


# ---- the state: a numpy rule over (name, shape) in state_dict order -------------------------------------------------------------------
def numpy_state(entries, seed, gamma=(0.6, 0.9)):
    """{name: float32 / int64 array} for the (name, shape) list of a state_dict, each entry from its own
    np.random.default_rng([seed, index]): a conv weight N(0, 1.6 / fan_in); BatchNorm weight gamma[0] + gamma[1] U, bias
    -0.3 + 0.8 U, running_mean 0.2 N, running_var 0.6 + 0.8 U, num_batches_tracked 0; a conv bias 0.1 N"""
    out, shapes = {}, {n: tuple(s) for n, s in entries}
    for i, (name, shape) in enumerate(entries):
        rng = np.random.default_rng([seed, i])
        shape = tuple(shape)
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            v = np.zeros(shape, dtype=np.int64)
        elif len(shape) == 4:
            v = rng.standard_normal(shape) * (1.6 / (shape[1] * shape[2] * shape[3])) ** 0.5
        elif leaf == "running_mean":
            v = 0.2 * rng.standard_normal(shape)
        elif leaf == "running_var":
            v = 0.6 + 0.8 * rng.random(shape)
        elif leaf == "weight":
            v = gamma[0] + gamma[1] * rng.random(shape)
        elif leaf == "bias" and len(shapes[name[:-4] + "weight"]) == 4:
            v = 0.1 * rng.standard_normal(shape)
        else:
            v = -0.3 + 0.8 * rng.random(shape)
        out[name] = v if v.dtype == np.int64 else v.astype(np.float32)
    return out


def entries_of(module):
    return [(k, tuple(v.shape)) for k, v in module.state_dict().items()]


@functools.lru_cache(maxsize=None)
def _synth_state(arch, num_classes, output_stride, seed):
    m = RefDeepLab(arch, num_classes, output_stride)
    sd = {k: torch.from_numpy(v) for k, v in numpy_state(entries_of(m), seed).items()}
    m.load_state_dict(sd, strict=True)
    m = m.double()
    # running statistics = one batch's own statistics spread by the rule's draws (scaled), so that eval mode sees activations
    # of the scale training sees: 26 stacked residual units with random running statistics would not
    rule = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.momentum = 1.0
        m.train()(synth_images(2, 131, 115, seed + 7).double())
        for name, mod in m.named_modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.running_mean.add_(mod.running_var.sqrt() * 0.5 * rule[name + ".running_mean"])
                mod.running_var.mul_(0.9 + 0.25 * (rule[name + ".running_var"] - 0.6))
                mod.num_batches_tracked.zero_()
    return {k: (v.float() if v.is_floating_point() else v.clone()) for k, v in m.state_dict().items()}


def synth_state(arch='deeplabv3plus', num_classes=2, output_stride=16, seed=SEED):
    return {k: v.clone() for k, v in _synth_state(arch, num_classes, output_stride, seed).items()}


def build(arch, num_classes, output_stride, sd, dtype=torch.float64):
    m = RefDeepLab(arch, num_classes, output_stride)
    m.load_state_dict(sd, strict=True)
    return m.to(dtype)
