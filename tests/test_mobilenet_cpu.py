"""MobileNetV2 DeepLab models: what can be checked without a GPU -- the constructors, the state_dict against the stock-torch
restatement (tests/mobilenet_ref.py), the 17 depthwise geometries, _load_model's routing and the host-side queries of the
depthwise 3x3 kernels."""
import ctypes

import pytest
import torch

from tests import mobilenet_ref as R

# (channels, stride, dilation) of the 17 depthwise layers, from the [t, c, n, s] table and the stride rule
DW_OS16 = [(32, 1, 1), (96, 2, 1), (144, 1, 1), (144, 2, 1), (192, 1, 1), (192, 1, 1), (192, 2, 1)] + [(384, 1, 1)] * 4 + \
          [(576, 1, 1)] * 3 + [(960, 1, 2)] * 3
DW_OS8 = [(32, 1, 1), (96, 2, 1), (144, 1, 1), (144, 2, 1), (192, 1, 1), (192, 1, 1), (192, 1, 1)] + [(384, 1, 2)] * 4 + \
         [(576, 1, 2)] * 3 + [(960, 1, 4)] * 3


def test_constructors_exist_and_are_model_choices():
    from iswm_amd import train
    from iswm_amd.network import modeling
    assert callable(modeling.deeplabv3plus_mobilenet) and callable(modeling.deeplabv3_mobilenet)
    choices = next(a.choices for a in train.get_argparser()._actions if "--model" in a.option_strings)
    assert "deeplabv3plus_mobilenet" in choices and "deeplabv3_mobilenet" in choices


@pytest.mark.parametrize("arch", ["deeplabv3plus", "deeplabv3"])
@pytest.mark.parametrize("os_", [16, 8])
def test_state_dict_matches_restatement(arch, os_):
    from iswm_amd.network import modeling
    m = getattr(modeling, arch + "_mobilenet")(num_classes=2, output_stride=os_)
    ref = R.RefDeepLab(arch, 2, os_)
    sd, rsd = m.state_dict(), ref.state_dict()
    assert list(sd) == list(rsd)
    assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in rsd.values()]
    assert sum(k.startswith("backbone.") for k in sd) == 306
    assert "backbone.low_level_features.3.conv.7.weight" in sd and "backbone.high_level_features.17.conv.0.weight" in sd
    m.load_state_dict(R.synth_state(arch, 2, os_), strict=True)


@pytest.mark.parametrize("os_,expect", [(16, DW_OS16), (8, DW_OS8)])
def test_depthwise_geometries(os_, expect):
    from iswm_amd.network import _hip, modeling
    m = modeling.deeplabv3plus_mobilenet(num_classes=2, output_stride=os_)
    got = [(d.in_channels, d.stride[0], d.dilation[0]) for d in m.modules() if isinstance(d, _hip.DepthwiseConv2d)]
    assert got == expect
    assert all(d.padding[0] == d.dilation[0] and d.is_dw3x3() for d in m.modules() if isinstance(d, _hip.DepthwiseConv2d))
    ref = [(c.in_channels, c.stride[0], c.dilation[0]) for c in R.RefDeepLab("deeplabv3plus", 2, os_).modules()
           if isinstance(c, torch.nn.Conv2d) and c.groups > 1]
    assert ref == expect


def test_init_and_pretrained():
    from iswm_amd.network import modeling
    from iswm_amd.network.backbone import mobilenetv2
    bb = mobilenetv2.mobilenet_v2(output_stride=16)
    bns = [m for m in bb.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(bns) == 51 and all(bool((b.weight == 1).all()) and bool((b.bias == 0).all()) for b in bns)
    with pytest.raises(RuntimeError, match="download"):
        modeling.deeplabv3plus_mobilenet(num_classes=2, output_stride=16, pretrained_backbone=True)
    with pytest.raises(ValueError):
        mobilenetv2.MobileNetV2(output_stride=32)


def test_load_model_routes_backbones():
    from iswm_amd.network import modeling
    m = modeling._load_model('deeplabv3plus', 'mobilenetv2', 3, 16, False)
    assert m.classifier.num_classes == 3 and list(m.backbone.return_layers.values()) == ['out', 'low_level']
    m3 = modeling._load_model('deeplabv3', 'mobilenetv2', 3, 8, False)
    assert list(m3.backbone.return_layers.values()) == ['out']
    with pytest.raises(NotImplementedError):
        modeling._load_model('deeplabv3plus', 'xception', 3, 16, False)


def test_tile_and_workspace_queries_are_host_functions():
    """no device is touched: the statistic tiling and the backward workspace follow from the descriptor alone"""
    from iswm_amd import _lib
    lib = _lib.load()
    for n, h, w, c, s in [(16, 257, 257, 96, 2), (16, 129, 129, 144, 1), (16, 33, 33, 960, 1), (2, 19, 23, 32, 1), (1, 1, 9, 144, 1)]:
        ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
        d = _lib.ConvDesc(n, h, w, c, ho, wo, c, 3, 3, s, 1, 1, c, c)
        tr, nt = lib.iswm_dwconv3x3_stat_tile_rows(ctypes.byref(d)), lib.iswm_dwconv3x3_stat_tiles(ctypes.byref(d))
        p = n * ho * wo
        assert tr > 0 and nt == (p + tr - 1) // tr
        ws = lib.iswm_dwconv3x3_bwd_workspace(ctypes.byref(d))
        assert ws % (9 * c * 4) == 0 and 0 < ws // (9 * c * 4) <= 2048
        # the partials are small next to the tensors they summarise
        assert 2 * nt * c * 4 <= 0.1 * p * c * 4 + 4096 and ws <= 0.1 * p * c * 4 + 9 * c * 4
