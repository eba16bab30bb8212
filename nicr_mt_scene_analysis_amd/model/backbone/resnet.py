"""The ResNet (v1) backbones of the reference (model/backbone/resnet.py): a 7x7 stride-2 stem convolution,
the 3x3 stride-2 max pool and four layers of residual blocks (`model.block`), cut into five stages.

  stage 0   conv1 -> norm1 -> act (-> se_conv1)        downsampling 2
  stage 1   maxpool -> layer1 (-> se_layer1)           4
  stage 2-4 layer2 .. layer4 (-> se_layer2 .. 4)       8, 16, 32 (a stride replaced by a dilation keeps the value)

Constructor signatures, sub-module names (`conv1`, `norm1`, `act`, `maxpool`, `layer1..4`, `se_conv1`,
`se_layer1..4`, `downsample` = Sequential(conv1x1, norm)) and the `stages*` properties are the reference's, so
its checkpoints load with `strict=True`.

On the device.  `maxpool` is `model.pooling.MaxPool2d`: one HIP launch forward and one backward with a one-byte
code in place of ATen's int64 index.  Stage 0 hands `norm1` -> `act` to `block.batch_norm_tail`, the fused
batch-norm tail of the blocks, with the blocks' fallbacks (CPU tensors, other normalizations or activations,
maps below `block.FUSED_MIN_ELEMENTS`, ...).  `stages[0]` is a small module, `ResNetStem`, that refers to
`conv1`, `norm1`, `act` (and `se_conv1`) of the backbone; like the reference's stage list it is not registered
as a sub-module, so it adds no state-dict keys.  The convolutions, the `downsample` branch and the
SqueezeAndExcitation modules of the `*se` backbones are torch.

The library never downloads: `convert_torchvision_resnet_state_dict` is the reference's rewriting of a
torchvision checkpoint as a pure function, for a state dict the caller has."""
import warnings
from collections import OrderedDict
from typing import Any, Dict, List, Optional, Type, Union

import torch
from torch import Tensor, nn

from ..activation import get_activation_class
from ..block import BlockType, Bottleneck, batch_norm_tail
from ..normalization import get_normalization_class
from ..pooling import MaxPool2d
from ..utils import SqueezeAndExcitation, conv1x1
from .base import Backbone


class ResNetStem(nn.Module):
    """stage 0: conv -> norm -> act through the fused batch-norm tail, then the optional SE weighting"""

    def __init__(self, conv: nn.Module, norm: nn.Module, act: nn.Module, se: Optional[nn.Module] = None) -> None:
        super().__init__()
        self.conv, self.norm, self.act, self.se = conv, norm, act, se

    def forward(self, x: Tensor) -> Tensor:
        out = batch_norm_tail(self.norm, self.act, self.conv(x))
        return out if self.se is None else self.se(out)


class ResNetBackbone(Backbone):
    def __init__(self, block: Type[BlockType], layers: List[int], zero_init_residual: bool = False, groups: int = 1,
                 width_per_group: int = 64, replace_stride_with_dilation: Optional[List[bool]] = None,
                 normalization: Type[nn.Module] = get_normalization_class(),
                 activation: Type[nn.Module] = get_activation_class(), n_input_channels: int = 3) -> None:
        super().__init__()
        self._block, self._normalization, self._activation = block, normalization, activation
        self.inplanes = 64
        self.dilation = 1
        if replace_stride_with_dilation is None:
            replace_stride_with_dilation = [False, False, False]
        if len(replace_stride_with_dilation) != 3:
            raise ValueError('replace_stride_with_dilation should be None or a 3-element tuple, got '
                             f'{replace_stride_with_dilation}')
        self.groups = groups
        self.base_width = width_per_group
        self.conv1 = nn.Conv2d(n_input_channels, self.inplanes, kernel_size=7, stride=2, padding=3, bias=False)
        self.norm1 = normalization(self.inplanes)
        self.act = activation()
        self.maxpool = MaxPool2d(kernel_size=3, stride=2, padding=1)
        dilate = replace_stride_with_dilation
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2, dilate=dilate[0])
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2, dilate=dilate[1])
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2, dilate=dilate[2])

        e = block.expansion
        self._stages = [ResNetStem(self.conv1, self.norm1, self.act), nn.Sequential(self.maxpool, self.layer1),
                        self.layer2, self.layer3, self.layer4]
        self._stages_n_channels = [64, 64 * e, 128 * e, 256 * e, 512 * e]
        # a stride that became a dilation does not downsample
        self._stages_downsampling = [2, 4] + [4 * 2 ** (k - sum(dilate[:k])) for k in (1, 2, 3)]
        self._stages_memory_layout = ['nchw'] * 5

    @property
    def stages(self) -> List[Union[nn.Sequential, nn.Module]]:
        return self._stages

    @property
    def stages_n_channels(self) -> List[int]:
        return self._stages_n_channels

    @property
    def stages_downsampling(self) -> List[int]:
        return self._stages_downsampling

    @property
    def stages_memory_layout(self) -> List[str]:
        return self._stages_memory_layout

    def _make_layer(self, block: Type[BlockType], planes: int, blocks: int, stride: int = 1,
                    dilate: bool = False) -> nn.Sequential:
        first_dilation = self.dilation
        if dilate:
            self.dilation *= stride
            stride = 1
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(conv1x1(self.inplanes, planes * block.expansion, stride),
                                       self._normalization(planes * block.expansion))
        common = dict(planes=planes, groups=self.groups, base_width=self.base_width,
                      normalization=self._normalization, activation=self._activation)
        made = [block(inplanes=self.inplanes, stride=stride, downsample=downsample, dilation=first_dilation, **common)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            made.append(block(inplanes=self.inplanes, stride=1, downsample=None, dilation=self.dilation, **common))
        return nn.Sequential(*made)


class ResNetSEBackbone(ResNetBackbone):
    def __init__(self, block: Type[BlockType], layers: List[int], zero_init_residual: bool = False, groups: int = 1,
                 width_per_group: int = 64, replace_stride_with_dilation: Optional[List[bool]] = None,
                 normalization: Type[nn.Module] = get_normalization_class(),
                 activation: Type[nn.Module] = get_activation_class(), n_input_channels: int = 3) -> None:
        super().__init__(block=block, layers=layers, zero_init_residual=zero_init_residual, groups=groups,
                         width_per_group=width_per_group, replace_stride_with_dilation=replace_stride_with_dilation,
                         normalization=normalization, activation=activation, n_input_channels=n_input_channels)
        n = self.stages_n_channels
        self.se_conv1 = SqueezeAndExcitation(n_channels=n[0], activation=activation)
        self.se_layer1 = SqueezeAndExcitation(n_channels=n[1], activation=activation)
        self.se_layer2 = SqueezeAndExcitation(n_channels=n[2], activation=activation)
        self.se_layer3 = SqueezeAndExcitation(n_channels=n[3], activation=activation)
        self.se_layer4 = SqueezeAndExcitation(n_channels=n[4], activation=activation)
        self._stages = [ResNetStem(self.conv1, self.norm1, self.act, self.se_conv1),
                        nn.Sequential(self.maxpool, self.layer1, self.se_layer1),
                        nn.Sequential(self.layer2, self.se_layer2),
                        nn.Sequential(self.layer3, self.se_layer3),
                        nn.Sequential(self.layer4, self.se_layer4)]


def adapt_conv1_weight(weight: Tensor, n_input_channels: int) -> Tensor:
    """the 3-channel stem weight for another input: 1 channel (depth) the sum over the three, as if the depth
    image were fed three times; 4 channels (rgbd) the three with their sum appended, halved to keep the
    magnitude; anything else unchanged"""
    if n_input_channels == 1:
        return torch.sum(weight, dim=1, keepdim=True)
    if n_input_channels == 4:
        return torch.cat([weight, torch.sum(weight, dim=1, keepdim=True)], dim=1) / 2
    return weight


def convert_torchvision_resnet_state_dict(state_dict: Dict[str, Tensor],
                                          n_input_channels: int = 3) -> 'OrderedDict[str, Tensor]':
    """A torchvision ResNet state dict with this package's keys: `bn1/2/3` -> `norm1/2/3`, the classifier
    (`fc.*`) dropped, `conv1.weight` adapted for a 1-channel input (the reference sums it after its download;
    4 channels follow the checkpoint rule).  Pure: the input dict is not modified."""
    out = OrderedDict()
    for key, value in state_dict.items():
        if key.startswith('fc.'):
            continue
        for k in ('1', '2', '3'):
            key = key.replace('bn' + k, 'norm' + k)
        out[key] = value
    if 'conv1.weight' in out:
        out['conv1.weight'] = adapt_conv1_weight(out['conv1.weight'], n_input_channels)
    return out


def get_resnet_backbone(name: str, block: Type[BlockType], pretrained_torchvision: bool = False,
                        normalization: Type[nn.Module] = get_normalization_class(),
                        activation: Type[nn.Module] = get_activation_class(),
                        **kwargs: Any) -> Union[ResNetBackbone, ResNetSEBackbone]:
    name = name.lower()
    if 'resnet18' in name:
        layers = [2, 2, 2, 2]
    elif 'resnet34' in name or 'resnet50' in name:
        layers = [3, 4, 6, 3]
        if name == 'resnet50' and not issubclass(block, Bottleneck):
            warnings.warn(f"ResNet50 requires 'Bottleneck' block, but '{block}' was passed")   # a ResNet34 then
    elif 'resnet101' in name:
        if not issubclass(block, Bottleneck):
            warnings.warn(f"ResNet101 requires 'Bottleneck' block, but '{block}' was passed")
        layers = [3, 4, 23, 3]
    else:
        raise ValueError(f'Unknown ResNet backbone: {name}')
    if pretrained_torchvision:
        raise ValueError('This library never downloads: torchvision weights are not fetched.  Convert a state '
                         'dict you have with `convert_torchvision_resnet_state_dict` and load it, or pass '
                         '`pretrained_filepath` to `get_backbone`.')
    cls = ResNetSEBackbone if name.endswith('se') else ResNetBackbone
    return cls(block=block, layers=layers, normalization=normalization, activation=activation, **kwargs)
