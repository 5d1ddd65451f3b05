"""Xception DeepLab models: what can be checked without a GPU -- the constructors and their --model choices, the module tree
against the list of names and shapes recorded from the reference's own class (tests/golden/xception_keys.json), the
depthwise geometries, the stock-torch restatement of tests/xception_ref.py against features recorded from the reference's
class (tests/golden/xception_features.npz), and the conditioning of the synthetic state the GPU tests use.

The two fixtures are written by tools/xception_fixtures.py from a checkout of the reference; no test runs it."""
import json
import os

import numpy as np
import pytest
import torch

from tests import dw3_pre_ref as D
from tests import xception_ref as R
from tests.util import rel_err

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _keys():
    with open(os.path.join(GOLDEN, "xception_keys.json")) as f:
        return [(k, tuple(s)) for k, s in json.load(f)]


def test_constructors_exist_and_are_model_choices():
    from iswm_amd import predict, train
    from iswm_amd.network import modeling
    assert callable(modeling.deeplabv3plus_xception) and callable(modeling.deeplabv3_xception)
    for parser in (train.get_argparser(), predict.get_argparser()):
        choices = next(a.choices for a in parser._actions if "--model" in a.option_strings)
        assert "deeplabv3plus_xception" in choices and "deeplabv3_xception" in choices


def test_load_model_still_refuses_xception_and_pretrained_raises():
    from iswm_amd.network import modeling
    from iswm_amd.network.backbone import xception
    with pytest.raises(NotImplementedError):
        modeling._load_model('deeplabv3plus', 'xception', 3, 16, False)
    for ctor in (modeling.deeplabv3plus_xception, modeling.deeplabv3_xception):
        with pytest.raises(RuntimeError, match="download"):
            ctor(num_classes=2, output_stride=16, pretrained_backbone=True)
    with pytest.raises(ValueError):
        xception.Xception(replace_stride_with_dilation=[False, False, True])
    with pytest.raises(NotImplementedError):
        modeling._segm_xception('fcn', 'xception', 2, 16, False)


@pytest.mark.parametrize("os_", [16, 8])
def test_module_tree_is_the_reference_one(os_):
    """backbone state-dict keys, in order, and shapes: the recorded list (269 entries; the dilation does not change it)"""
    from iswm_amd.network import modeling
    from iswm_amd.network.backbone import xception
    keys = _keys()
    assert len(keys) == 269
    m = modeling.deeplabv3plus_xception(num_classes=2, output_stride=os_)
    got = [(k, tuple(v.shape)) for k, v in m.backbone.state_dict().items()]
    assert got == keys
    assert not any(k.startswith("bn4") or k.startswith("fc") for k, _ in got)                   # conv4 is the last child taken
    full = xception.Xception()
    assert [n for n, _ in full.named_children()] == ["conv1", "bn1", "relu1", "conv2", "bn2", "relu2"] + \
        ["block%d" % k for k in range(1, 13)] + ["conv3", "bn3", "relu3", "conv4", "bn4"]
    assert [n for n, _ in full.block1.named_children()] == ["skip", "skipbn", "rep"] and full.block5.skip is None
    assert [n for n, _ in full.conv3.named_children()] == ["conv1", "pointwise"]
    # the whole model against the restatement, both heads
    for arch in ("deeplabv3plus", "deeplabv3"):
        m = getattr(modeling, arch + "_xception")(num_classes=2, output_stride=os_)
        ref = R.RefDeepLab(arch, 2, os_)
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
        assert list(m.backbone.return_layers.values()) == (['out', 'low_level'] if arch == "deeplabv3plus" else ['out'])


@pytest.mark.parametrize("os_,expect", [(16, D.DIL_PAD_OS16), (8, D.DIL_PAD_OS8)])
def test_depthwise_geometries(os_, expect):
    from iswm_amd.network import _hip, modeling
    from iswm_amd.network.backbone import xception
    m = modeling.deeplabv3plus_xception(num_classes=2, output_stride=os_)
    dws = [d for d in m.backbone.modules() if isinstance(d, _hip.DepthwiseConv2d)]
    assert len(dws) == 34 and all(d.kernel_size == (3, 3) and d.stride == (1, 1) and d.bias is None for d in dws)
    assert {(d.dilation[0], d.padding[0]) for d in dws} == expect
    assert {d.in_channels for d in dws} == {64, 128, 256, 728, 1024, 1536}
    ref = [c for c in R.RefDeepLab("deeplabv3plus", 2, os_).backbone.modules() if isinstance(c, torch.nn.Conv2d) and c.groups > 1]
    assert [(c.in_channels, c.dilation[0], c.padding[0]) for c in ref] == [(d.in_channels, d.dilation[0], d.padding[0]) for d in dws]
    # the pitch of the pointwise operand: 728 -> 768 (the planes kernels gather 64 channels per chunk), the others as they are
    pws = [s.pointwise for s in m.backbone.modules() if isinstance(s, xception.SeparableConv2d)]
    assert {(p.in_channels, p.cin_p) for p in pws} == {(64, 64), (128, 128), (256, 256), (728, 768), (1024, 1024), (1536, 1536)}
    assert all(D.layout(p.cin_p)[3] is False for p in pws)                                       # never the idle-lane fallback
    # which units rectify on load: the first of every block but block1
    first = {n: b._units()[1] is not None for n, b in m.backbone.named_children() if isinstance(b, xception.Block)}
    assert first == dict({"block%d" % k: True for k in range(2, 13)}, block1=False)
    acts = [[u[2].name for u in b._units()[0]] for b in m.backbone.children() if isinstance(b, xception.Block)]
    assert acts[0] == ["RELU", "NONE"] and acts[4] == ["RELU", "RELU", "NONE"] and acts[11] == ["RELU", "NONE"]


def test_restatement_reproduces_the_reference_features():
    """the float64 restatement, given the fixture's input and the numpy-rule weights, against `out` / `low_level` recorded from
    the reference's class: float32 storage rounding, 1e-6 of the feature's max"""
    fx = np.load(os.path.join(GOLDEN, "xception_features.npz"))
    assert fx["input"].shape == (1, 3, 131, 99) and fx["out"].shape == (1, 2048, 4, 2) and fx["low_level"].shape == (1, 128, 32, 24)
    assert all(fx[k].dtype == np.float32 for k in fx.files)
    b = R.Backbone(16)
    assert R.entries_of(b) == _keys()
    b.load_state_dict({k: torch.from_numpy(v) for k, v in R.numpy_state(_keys(), 1).items()}, strict=True)
    b = b.double().eval()
    with torch.no_grad():
        low, out = b(torch.from_numpy(fx["input"]).double())
    e_low, e_out = rel_err(low, fx["low_level"]), rel_err(out, fx["out"])
    print("restatement against the recorded features: low_level %.2e  out %.2e" % (e_low, e_out))
    assert e_low <= 1e-6 and e_out <= 1e-6


def test_feature_sizes():
    """513^2: out 28 x 28 at output stride 16 and 52 x 52 at output stride 8, low_level 127 x 127 in both (computed from the
    layer arithmetic the restatement uses); the GPU tests' inputs; the smallest width with an output at output stride 8"""
    def sizes(n, os_):
        n = (n - 3) // 2 + 1 - 2                                 # conv1 (stride 2, pad 0), conv2 (pad 0)
        low = n = (n - 1) // 2 + 1                               # block1
        n = (n - 1) // 2 + 1                                     # block2
        if os_ == 16:
            n = (n - 1) // 2 + 1                                 # block3
        dil = 2 if os_ == 16 else 4
        return low, n - 4 * (dil - 1)                            # conv3, conv4: pad 1 under dilation dil
    assert sizes(513, 16) == (127, 28) and sizes(513, 8) == (127, 52)
    assert (sizes(131, 16), sizes(99, 16)) == ((32, 4), (24, 2))
    assert (sizes(131, 8), sizes(115, 8)) == ((32, 4), (28, 2))
    assert sizes(103, 8)[1] == 1 and sizes(102, 8)[1] <= 0       # (103 is the smallest width with an output; the tests use 115)
    with torch.no_grad():
        low, out = R.Backbone(8).eval()(torch.zeros(1, 3, 131, 115))
    assert tuple(low.shape[2:]) == (32, 28) and tuple(out.shape[2:]) == (4, 2)


def test_synthetic_state_is_well_conditioned():
    """the GPU tests' state (xception_ref.SEED), float32 against float64 restatement on the CPU (one thread: the float32 sums depend
    on the thread count), train mode, first model case: the running statistics agree at least three times closer than the GPU
    tests' 1e-5 and fewer than 1e-5 of the ReLU decisions differ -- what the GPU comparison can be expected to hold"""
    from tests.conv_ref import one_thread
    arch, os_, n, h, w = "deeplabv3plus", 16, 2, 131, 99
    sd = R.synth_state(arch, 2, os_)
    x = R.synth_images(n, h, w, 5)
    got = {}
    for dt in (torch.float64, torch.float32):
        m = R.build(arch, 2, os_, sd, dt).train()
        m.ctl.preact = {}
        with torch.no_grad(), one_thread():
            lg = m(x.to(dt))
        got[dt] = (lg, {k: v.clone() for k, v in m.state_dict().items() if "running" in k}, m.ctl.preact)
    (lg64, st64, pre64), (lg32, st32, pre32) = got[torch.float64], got[torch.float32]
    worst = max(rel_err(st32[k], st64[k]) for k in st64)
    relu = [s for s in pre64 if pre64[s].dim() == 4]
    flips = sum(int(((pre64[s] > 0) != (pre32[s] > 0)).sum()) for s in relu)
    total = sum(pre64[s].numel() for s in relu)
    alive = min(float((pre64[s] > 0).double().mean()) for s in relu)
    print("seed %d: running statistics %.2e  logits %.2e  ReLU decisions %d of %d differ; least active site passes %.0f %%" %
          (R.SEED, worst, rel_err(lg32, lg64), flips, total, 100 * alive))
    assert R.SEED == 5 and worst <= 1e-5 / 3 and rel_err(lg32, lg64) <= 1e-4 and flips <= 1e-5 * total and alive > 0.02
