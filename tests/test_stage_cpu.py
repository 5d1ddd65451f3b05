"""The typed records of the fused conv -> BatchNorm -> activation path (ops.Act, _hip.Stage, _hip.StageCtx): modules are built
on the CPU and nothing is launched."""
import pytest
import torch.nn as nn

from iswm_amd import ops
from iswm_amd.network import _deeplab, _hip
from iswm_amd.network.backbone import mobilenetv2
from iswm_amd.ops import Act


class _OtherInt(int):
    """an int subclass that is not Act: the value alone does not make an activation"""


@pytest.mark.parametrize("value,want", [(Act.NONE, Act.NONE), (Act.RELU, Act.RELU), (Act.RELU6, Act.RELU6), (None, Act.NONE),
                                        (False, Act.NONE), (0, Act.NONE), (True, Act.RELU), (1, Act.RELU), (6, Act.RELU6)])
def test_act_of_accepts(value, want):
    got = Act.of(value)
    assert got is want and int(got) == {Act.NONE: 0, Act.RELU: 1, Act.RELU6: 6}[want]


@pytest.mark.parametrize("value", [2, -1, 6.0, 1.0, 0.0, "relu", "6", _OtherInt(6), _OtherInt(1), (), nn.ReLU()])
def test_act_of_rejects(value):
    with pytest.raises(ValueError) as e:
        Act.of(value)
    assert repr(value) in str(e.value)


def _kinds(stages):
    return [(s.kind, s.act) for s in stages]


def test_stages_of_the_heads():
    head = _deeplab.DeepLabHeadV3Plus(2048, 256, 2)
    st = head.classifier._stages()
    assert _kinds(st) == [("cba", Act.RELU), ("cba", Act.RELU), ("conv", Act.NONE)]
    assert [s.conv for s in st] == [head.classifier[0], head.classifier[3], head.classifier[6]]
    assert [s.bn for s in st] == [head.classifier[1], head.classifier[4], None]
    branch = head.aspp.convs[1]
    assert _kinds(branch._stages()) == [("cba", Act.RELU)]
    assert branch._stages()[0].bn_conv is branch[0]
    with pytest.raises(Exception):                          # immutable
        st[0].act = Act.NONE


def test_stages_of_an_inverted_residual():
    block = mobilenetv2.InvertedResidual(32, 32, 1, 1, 6)
    st = block._stages()
    assert [s.act for s in st] == [Act.RELU6, Act.RELU6, Act.NONE] and all(s.kind == "cba" for s in st)
    assert isinstance(st[1].conv, _hip.DepthwiseConv2d) and st[2].bn is block.conv[-1]
    assert [s.act for s in mobilenetv2.InvertedResidual(32, 16, 1, 1, 1)._stages()] == [Act.RELU6, Act.NONE]


def test_sequential_without_a_hip_implementation_raises():
    seq = _hip.HipSequential(_hip.Conv2d(8, 8, 1, bias=False), _hip.BatchNorm2d(8), _hip.ReLU(), nn.Sigmoid())
    with pytest.raises(NotImplementedError):
        seq._stages()
    with pytest.raises(ValueError):
        _hip.Stage("cba", seq[0], seq[1], True)             # a Stage holds an Act, not what Act.of coerces
    with pytest.raises(ValueError):
        _hip.Stage("bn", seq[0])


def test_stage_ctx_has_no_other_fields():
    conv, bn = _hip.Conv2d(8, 8, 1, bias=False), _hip.BatchNorm2d(8)
    ctx = _hip.StageCtx(_hip.Stage("cba", conv, bn, Act.RELU), x=None, y=None, coef=None, g=None, training=True)
    assert ctx.bn_stats is None and ctx.cls is None and ctx.sep is None and ctx.dw is False and ctx.res is False
    ctx.bn_stats = ops.BnStats(None, None, True)
    assert ctx.bn_stats.act is Act.RELU
    with pytest.raises(AttributeError):
        ctx.bn_stat = None
    with pytest.raises(AttributeError):
        ctx.relu
    dw = _hip.DepthwiseConv2d(8, 8, 3, 1, 1, groups=8, bias=False)
    assert _hip.StageCtx(_hip.Stage("cba", dw, bn, Act.RELU6), None, None, None, None, True).dw is True
    sep = _deeplab.AtrousSeparableConvolution(8, 8, 3, padding=1)
    c = _hip.StageCtx(_hip.Stage("cba", sep, bn, Act.RELU), None, None, None, None, True)
    assert c.sep is sep and c.dw is False and c.stage.bn_conv is sep.body[1]


def test_aspp_branch_convs_cover_relu_branches_only():
    aspp = _deeplab.ASPP(64, [6, 12, 18])
    br = aspp._branch_convs()
    assert len(br) == 4 and [s.conv for s in br] == [m[0] for m in list(aspp.convs)[:4]]
    assert all(s.kind == "cba" and s.act is Act.RELU for s in br)
    aspp.convs[2][2] = _hip.ReLU6()
    assert aspp._branch_convs() is None
    aspp.convs[2][2] = _hip.ReLU()
    assert len(aspp._branch_convs()) == 4
    aspp.convs[1] = _hip.HipSequential(aspp.convs[1][0], aspp.convs[1][1])      # activation removed
    assert aspp._branch_convs() is None
