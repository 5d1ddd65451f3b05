"""Stock-torch restatement of the MobileNetV2 DeepLab models, the parity reference of tests/test_mobilenet_*.py.

The reference project has no MobileNet, so nothing pins this model from outside: this file restates the public
MobileNetV2 / DeepLabV3(+) definition in plain ``nn.Conv2d`` / ``nn.BatchNorm2d`` / ``nn.ReLU6`` / ``nn.ReLU`` (any
dtype: the tests run it in float64 on the CPU), written from the specification and not from iswm_amd's modules:

  * features[0] = conv 3->32 3x3 stride 2, BN, ReLU6; then inverted-residual blocks from the table [t, c, n, s] below;
  * block(inp, oup, stride, dilation, t): [1x1 expand to inp*t, BN, ReLU6 (only when t != 1)], 3x3 depthwise (stride,
    padding = dilation), BN, ReLU6, 1x1 project, BN; the input is added, with no activation, when stride == 1 and inp == oup;
  * stride rule: current_stride = 2 after features[0], dilation = 1; per table row previous_dilation = dilation, and when
    current_stride == output_stride the row's stride becomes 1 and dilation *= s, else current_stride *= s; the row's first
    block gets (stride, previous_dilation), the others (1, dilation);
  * the segmentation model taps features[0:4] (24 channels, 'low_level') and features[4:] (320 channels, 'out').

Every activation follows a BatchNorm and is named after it (its "site").  ``Control`` lets a test record each site's
pre-activation and impose another implementation's activation pattern (see Act).
"""
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

GAMMA = (1.0, 2.4)      # BatchNorm gamma = GAMMA[0] + GAMMA[1] * U(0, 1)
# The state's seed.  The ASPP image-pooling branch normalises TWO samples per channel at the tests' batch of 2, which
# amplifies rounding by up to 1 / sqrt(eps) wherever the two pooled values nearly coincide; how badly depends on the draw.
# Chosen on the CPU, from this restatement alone: of seeds 11..22 the one whose float32 evaluation stays closest to the float64
# one in train mode on the tests' input (running statistics within 9e-7 / 2e-6 / 1.2e-6 for the three model cases, five
# times under the tests' 1e-5; seed 11 gives 6e-6 .. 1.3e-5).  All 34 ReLU6 sites reach the clamp at 6 on > 1 % of their elements.
SEED = 20
TABLE = [[1, 16, 1, 1], [6, 24, 2, 2], [6, 32, 3, 2], [6, 64, 4, 2], [6, 96, 3, 1], [6, 160, 3, 2], [6, 320, 1, 1]]


class Control(object):
    def __init__(self):
        self.preact = None      # dict -> {site: pre-activation} recorded on every forward
        self.masks = None       # dict {site: bool NCHW "pass" pattern} imposed on every activation


class _Act(object):
    """mixin of the two activations.  With ctl.masks: the output is z where the imposed pattern passes; elsewhere a ReLU
    gives 0 and a ReLU6 gives 0 or 6, whichever clamp this evaluation's own pre-activation is nearer to (a clamped site
    carries no gradient either way)."""
    ctl, site, top = None, None, None

    def forward(self, z):
        ctl = self.ctl
        if ctl is not None and ctl.preact is not None:
            ctl.preact[self.site] = z.detach()
        if ctl is None or ctl.masks is None:
            return F.relu(z) if self.top is None else F.hardtanh(z, 0.0, self.top)
        m = ctl.masks[self.site]
        out = z * m.to(z.dtype)
        if self.top is not None:
            out = out + ((~m) & (z.detach() > self.top / 2)).to(z.dtype) * self.top
        return out


class ReLU6(_Act, nn.ReLU6):
    top = 6.0


class ReLU(_Act, nn.ReLU):
    pass


def _cbr(cin, cout, k, stride=1, pad=0, dil=1, groups=1, act=ReLU6):
    m = [nn.Conv2d(cin, cout, k, stride, pad, dil, groups, bias=False), nn.BatchNorm2d(cout)]
    if act is not None:
        m.append(act(inplace=False))
    return m


class Block(nn.Module):
    def __init__(self, inp, oup, stride, dilation, t):
        super().__init__()
        hidden = inp * t
        self.add = stride == 1 and inp == oup
        m = []
        if t != 1:
            m += _cbr(inp, hidden, 1)
        m += _cbr(hidden, hidden, 3, stride, dilation, dilation, groups=hidden)
        m += _cbr(hidden, oup, 1, act=None)
        self.conv = nn.Sequential(*m)

    def forward(self, x):
        return x + self.conv(x) if self.add else self.conv(x)


def features(output_stride):
    f = [nn.Sequential(*_cbr(3, 32, 3, 2, 1))]
    cin, current_stride, dilation = 32, 2, 1
    for t, c, n, s in TABLE:
        previous_dilation = dilation
        if current_stride == output_stride:
            stride = 1
            dilation *= s
        else:
            stride = s
            current_stride *= s
        for i in range(n):
            f.append(Block(cin, c, stride if i == 0 else 1, previous_dilation if i == 0 else dilation, t))
            cin = c
    return f


class Backbone(nn.Module):
    def __init__(self, output_stride, plus):
        super().__init__()
        f = features(output_stride)
        # children keep their index in the full feature list
        self.low_level_features = nn.Sequential()
        self.high_level_features = nn.Sequential()
        for i, m in enumerate(f):
            (self.low_level_features if i < 4 else self.high_level_features).add_module(str(i), m)
        self.plus = plus

    def forward(self, x):
        low = self.low_level_features(x)
        return low, self.high_level_features(low)


class ASPPPooling(nn.Sequential):
    def __init__(self, cin, cout):
        super().__init__(nn.AdaptiveAvgPool2d(1), *_cbr(cin, cout, 1, act=ReLU))

    def forward(self, x):
        return F.interpolate(super().forward(x), size=x.shape[-2:], mode='bilinear', align_corners=False)


class ASPP(nn.Module):
    def __init__(self, cin, rates):
        super().__init__()
        self.convs = nn.ModuleList([nn.Sequential(*_cbr(cin, 256, 1, act=ReLU))] +
                                   [nn.Sequential(*_cbr(cin, 256, 3, 1, r, r, act=ReLU)) for r in rates] +
                                   [ASPPPooling(cin, 256)])
        self.project = nn.Sequential(*_cbr(5 * 256, 256, 1, act=ReLU), nn.Dropout(0.1))

    def forward(self, x):
        return self.project(torch.cat([c(x) for c in self.convs], dim=1))


class HeadV3Plus(nn.Module):
    def __init__(self, cin, clow, num_classes, rates):
        super().__init__()
        self.project = nn.Sequential(*_cbr(clow, 48, 1, act=ReLU))
        self.aspp = ASPP(cin, rates)
        self.classifier = nn.Sequential(*_cbr(304, 256, 3, 1, 1, act=ReLU), *_cbr(256, 256, 3, 1, 1, act=ReLU),
                                        nn.Conv2d(256, num_classes, 1))

    def forward(self, low, out):
        low = self.project(low)
        out = F.interpolate(self.aspp(out), size=low.shape[2:], mode='bilinear', align_corners=False)
        return self.classifier(torch.cat([low, out], dim=1))


class HeadV3(nn.Module):
    def __init__(self, cin, num_classes, rates):
        super().__init__()
        self.classifier = nn.Sequential(ASPP(cin, rates), *_cbr(256, 256, 3, 1, 1, act=ReLU), nn.Conv2d(256, num_classes, 1))

    def forward(self, low, out):
        return self.classifier(out)


class RefDeepLab(nn.Module):
    """arch 'deeplabv3plus' | 'deeplabv3' over the MobileNetV2 backbone; dropout p = 0 (the tests compare deterministic steps)"""

    def __init__(self, arch, num_classes, output_stride):
        super().__init__()
        rates = [12, 24, 36] if output_stride == 8 else [6, 12, 18]
        self.backbone = Backbone(output_stride, arch == 'deeplabv3plus')
        self.classifier = HeadV3Plus(320, 24, num_classes, rates) if arch == 'deeplabv3plus' else HeadV3(320, num_classes, rates)
        self.ctl = Control()
        names = {m: n for n, m in self.named_modules()}
        for seq in self.modules():
            if isinstance(seq, nn.Sequential):
                ch = list(seq)
                for a, b in zip(ch, ch[1:]):
                    if isinstance(b, _Act):
                        assert isinstance(a, nn.BatchNorm2d)
                        b.site, b.ctl = names[a], self.ctl
        self.tops = {m.site: m.top for m in self.modules() if isinstance(m, _Act)}      # site -> 6.0 (ReLU6) | None (ReLU)
        for m in self.modules():
            if isinstance(m, nn.Dropout):
                m.p = 0.0

    def forward(self, x):
        low, out = self.backbone(x)
        return F.interpolate(self.classifier(low, out), size=x.shape[2:], mode='bilinear', align_corners=False)


def synth_images(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, h, w, generator=g) * 0.8 + 0.3


def synth_labels(n, h, w, seed, ignore_index=255):
    """blocky labels with class 1 and ignore_index present"""
    g = torch.Generator().manual_seed(seed + 1)
    coarse = torch.rand(n, 1, (h + 7) // 8, (w + 7) // 8, generator=g)
    u = F.interpolate(coarse, size=(h, w), mode='nearest')[:, 0]
    lab = (u > 0.7).long()
    lab[u < 0.06] = ignore_index
    return lab


@functools.lru_cache(maxsize=None)
def _synth_state(arch, num_classes, output_stride, seed):
    g = torch.Generator().manual_seed(seed)
    m = RefDeepLab(arch, num_classes, output_stride).double()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.Conv2d):
                fan_in = mod.weight[0].numel()
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g, dtype=torch.float64) * (1.6 / fan_in) ** 0.5)
                if mod.bias is not None:
                    mod.bias.copy_(torch.randn(mod.bias.shape, generator=g, dtype=torch.float64) * 0.1)
            elif isinstance(mod, nn.BatchNorm2d):
                # wide gamma / positive beta: normalised values x up to 3 reach the clamp at 6 on a few per cent of the elements
                mod.weight.copy_(GAMMA[0] + GAMMA[1] * torch.rand(mod.weight.shape, generator=g, dtype=torch.float64))
                mod.bias.copy_(-0.5 + 2.0 * torch.rand(mod.bias.shape, generator=g, dtype=torch.float64))
                mod.momentum = 1.0
        # running statistics = one batch's own statistics, then spread by up to 10 % / 0.1 sigma, so that eval mode sees
        # activations of the scale training sees (random running statistics would saturate every ReLU6 after a few blocks)
        m.train()(synth_images(2, 97, 81, seed + 7).double())
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.running_mean.add_(mod.running_var.sqrt() * 0.1 * torch.randn(mod.running_mean.shape, generator=g, dtype=torch.float64))
                mod.running_var.mul_(0.9 + 0.2 * torch.rand(mod.running_var.shape, generator=g, dtype=torch.float64))
                mod.num_batches_tracked.zero_()
    return {k: (v.float() if v.is_floating_point() else v.clone()) for k, v in m.state_dict().items()}


def synth_state(arch='deeplabv3plus', num_classes=2, output_stride=16, seed=SEED):
    """seeded fp32 state dict (a fresh copy) whose BatchNorm parameters keep the ReLU6 clamp at 6 live"""
    return {k: v.clone() for k, v in _synth_state(arch, num_classes, output_stride, seed).items()}


def build(arch, num_classes, output_stride, sd, dtype=torch.float64):
    m = RefDeepLab(arch, num_classes, output_stride)
    m.load_state_dict(sd, strict=True)
    return m.to(dtype)


def weighted_ce(logits, labels, weight, ignore_index=255):
    return F.cross_entropy(logits, labels, weight=weight.to(logits.dtype), ignore_index=ignore_index)


def saturated_sites(model, frac=0.01):
    """ReLU6 sites of a RefDeepLab whose recorded pre-activations reach the clamp at 6 on at least `frac` of the elements"""
    return [s for s, z in model.ctl.preact.items() if model.tops[s] is not None and float((z >= 6).double().mean()) >= frac]
