"""Model construction API -- counterpart of the reference's network/modeling.py
(_segm_resnet :12-56, _load_model :58-73, deeplabv3plus_resnet50 :75-83), same names
and signatures, so ``network.modeling.deeplabv3plus_resnet50(num_classes=...,
output_stride=...)`` in train.py:414-417 / predict.py:71-75 keeps working.

Differences, all deliberate:
  * ``pretrained_backbone`` defaults to False: the reference default triggers an HTTP
    download (network/backbone/resnet.py:220-223) that cannot work offline;
  * ``deeplabv3plus_resnet101`` / ``deeplabv3_resnet50/101`` are exposed (the reference
    reaches ResNet-101 only through the private ``_segm_resnet``);
  * ``deeplabv3plus_mobilenet`` / ``deeplabv3_mobilenet``: the reference has no MobileNet; the backbone
    and its state_dict keys follow the public MobileNetV2 / DeepLabV3Plus-Pytorch definition;
  * ``deeplabv3plus_xception`` / ``deeplabv3_xception``: the reference ships the Xception backbone
    (network/backbone/xception.py) but no constructor selects it; ``_segm_xception`` follows the public
    DeepLabV3Plus-Pytorch definition the reference was forked from (return_layers conv4 / block1).
"""
import torch
from torch import nn

from . import _hip
from ._deeplab import DeepLabHead, DeepLabHeadV3Plus, DeepLabV3
from .backbone import mobilenetv2, resnet, xception
from .utils import IntermediateLayerGetter


def _segm_resnet(name, backbone_name, num_classes, output_stride, pretrained_backbone, in_channels=3):
    if output_stride == 8:
        replace_stride_with_dilation = [False, True, True]
        aspp_dilate = [12, 24, 36]
    else:
        replace_stride_with_dilation = [False, False, True]
        aspp_dilate = [6, 12, 18]

    backbone = resnet.__dict__[backbone_name](
        pretrained=pretrained_backbone,
        replace_stride_with_dilation=replace_stride_with_dilation)

    if in_channels != 3:
        # stem surgery for multi-channel satellite tiles (reference :25-43)
        original_conv = backbone.conv1
        backbone.conv1 = _hip.Conv2d(
            in_channels,
            original_conv.out_channels,
            kernel_size=original_conv.kernel_size,
            stride=original_conv.stride,
            padding=original_conv.padding,
            bias=original_conv.bias is not None
        )
        if pretrained_backbone:
            with torch.no_grad():
                backbone.conv1.weight[:, :3, :, :].data.copy_(original_conv.weight.data)
                original_weight_mean = original_conv.weight.mean(dim=1, keepdim=True)
                for i in range(3, in_channels):
                    backbone.conv1.weight[:, i:i + 1, :, :].data.copy_(original_weight_mean)
    inplanes = 2048
    low_level_planes = 256

    if name == 'deeplabv3plus':
        return_layers = {'layer4': 'out', 'layer1': 'low_level'}
        classifier = DeepLabHeadV3Plus(inplanes, low_level_planes, num_classes, aspp_dilate)
    elif name == 'deeplabv3':
        return_layers = {'layer4': 'out'}
        classifier = DeepLabHead(inplanes, num_classes, aspp_dilate)
    else:
        raise NotImplementedError(name)
    backbone = IntermediateLayerGetter(backbone, return_layers=return_layers)
    model = DeepLabV3(backbone, classifier)
    return model


def _segm_mobilenet(name, backbone_name, num_classes, output_stride, pretrained_backbone):
    aspp_dilate = [12, 24, 36] if output_stride == 8 else [6, 12, 18]
    backbone = mobilenetv2.mobilenet_v2(pretrained=pretrained_backbone, output_stride=output_stride)
    # slices of an nn.Sequential keep the original indices: backbone.low_level_features.{0..3}, high_level_features.{4..17}
    backbone.low_level_features = backbone.features[0:4]
    backbone.high_level_features = backbone.features[4:]
    backbone.features = None
    inplanes = 320
    low_level_planes = 24

    if name == 'deeplabv3plus':
        return_layers = {'high_level_features': 'out', 'low_level_features': 'low_level'}
        classifier = DeepLabHeadV3Plus(inplanes, low_level_planes, num_classes, aspp_dilate)
    elif name == 'deeplabv3':
        return_layers = {'high_level_features': 'out'}
        classifier = DeepLabHead(inplanes, num_classes, aspp_dilate)
    else:
        raise NotImplementedError(name)
    backbone = IntermediateLayerGetter(backbone, return_layers=return_layers)
    return DeepLabV3(backbone, classifier)


def _segm_xception(name, backbone_name, num_classes, output_stride, pretrained_backbone):
    if output_stride == 8:
        replace_stride_with_dilation = [False, False, True, True]
        aspp_dilate = [12, 24, 36]
    else:
        replace_stride_with_dilation = [False, False, False, True]
        aspp_dilate = [6, 12, 18]
    backbone = xception.xception(pretrained=pretrained_backbone, replace_stride_with_dilation=replace_stride_with_dilation)
    inplanes = 2048
    low_level_planes = 128

    # conv4 is the last child taken, so bn4 is never applied and is not part of the model
    if name == 'deeplabv3plus':
        return_layers = {'conv4': 'out', 'block1': 'low_level'}
        classifier = DeepLabHeadV3Plus(inplanes, low_level_planes, num_classes, aspp_dilate)
    elif name == 'deeplabv3':
        return_layers = {'conv4': 'out'}
        classifier = DeepLabHead(inplanes, num_classes, aspp_dilate)
    else:
        raise NotImplementedError(name)
    backbone = IntermediateLayerGetter(backbone, return_layers=return_layers)
    return DeepLabV3(backbone, classifier)


def _load_model(arch_type, backbone, num_classes, output_stride, pretrained_backbone, temporal=False,
                model_type='parallel', opts=None, in_channels=3):
    if backbone.startswith('resnet'):
        model = _segm_resnet(arch_type, backbone, num_classes, output_stride=output_stride,
                             pretrained_backbone=pretrained_backbone, in_channels=in_channels)
    elif backbone == 'mobilenetv2':
        model = _segm_mobilenet(arch_type, backbone, num_classes, output_stride=output_stride,
                                pretrained_backbone=pretrained_backbone)
    else:
        raise NotImplementedError
    return model


def deeplabv3plus_resnet50(num_classes=21, output_stride=8, pretrained_backbone=False):
    """Constructs a DeepLabV3+ model with a ResNet-50 backbone (reference :75-83)."""
    return _load_model('deeplabv3plus', 'resnet50', num_classes, output_stride=output_stride,
                       pretrained_backbone=pretrained_backbone)


def deeplabv3plus_resnet101(num_classes=21, output_stride=8, pretrained_backbone=False):
    """DeepLabV3+ with a ResNet-101 backbone (BASELINE.json's headline model)."""
    return _load_model('deeplabv3plus', 'resnet101', num_classes, output_stride=output_stride,
                       pretrained_backbone=pretrained_backbone)


def deeplabv3_resnet50(num_classes=21, output_stride=8, pretrained_backbone=False):
    return _load_model('deeplabv3', 'resnet50', num_classes, output_stride=output_stride,
                       pretrained_backbone=pretrained_backbone)


def deeplabv3_resnet101(num_classes=21, output_stride=8, pretrained_backbone=False):
    return _load_model('deeplabv3', 'resnet101', num_classes, output_stride=output_stride,
                       pretrained_backbone=pretrained_backbone)


def deeplabv3plus_mobilenet(num_classes=21, output_stride=8, pretrained_backbone=False):
    """DeepLabV3+ with a MobileNetV2 backbone (BASELINE.json configs[0])."""
    return _load_model('deeplabv3plus', 'mobilenetv2', num_classes, output_stride=output_stride,
                       pretrained_backbone=pretrained_backbone)


def deeplabv3_mobilenet(num_classes=21, output_stride=8, pretrained_backbone=False):
    return _load_model('deeplabv3', 'mobilenetv2', num_classes, output_stride=output_stride,
                       pretrained_backbone=pretrained_backbone)


def deeplabv3plus_xception(num_classes=21, output_stride=8, pretrained_backbone=False):
    """DeepLabV3+ with the dilated Xception backbone.  _load_model refuses 'xception' as the reference's does, so the two
    Xception constructors build through _segm_xception directly."""
    return _segm_xception('deeplabv3plus', 'xception', num_classes, output_stride=output_stride,
                          pretrained_backbone=pretrained_backbone)


def deeplabv3_xception(num_classes=21, output_stride=8, pretrained_backbone=False):
    return _segm_xception('deeplabv3', 'xception', num_classes, output_stride=output_stride,
                          pretrained_backbone=pretrained_backbone)
