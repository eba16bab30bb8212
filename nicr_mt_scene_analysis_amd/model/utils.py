"""Building blocks of the model (reference model/utils.py), plain torch:
`ConvNormAct`, a convolution (1x1 by default) followed by a normalization and an activation, with the
reference's sub-module names `conv`, `norm`, `act` (the encoder-decoder fusion's channel adapter);
`SqueezeAndExcitation`, the channel weighting of the encoder RGB-D fusion, with the reference's
sub-module layout `layers.{0..3}`.  `model.encoder_fusion` reads its parameters for the fused HIP path
and calls it as it is everywhere else;
`conv3x3` and `conv1x1`, the bias-free convolutions of the residual blocks (`model.block`)."""
from typing import Optional, Type

import torch.nn.functional as F
from torch import Tensor, nn

from .activation import get_activation_class
from .normalization import get_normalization_class


def conv3x3(in_planes: int, out_planes: int, stride: int = 1, groups: int = 1, dilation: int = 1) -> nn.Conv2d:
    return nn.Conv2d(in_planes, out_planes, kernel_size=3, stride=stride, padding=dilation, groups=groups,
                     bias=False, dilation=dilation)


def conv1x1(in_planes: int, out_planes: int, stride: int = 1) -> nn.Conv2d:
    return nn.Conv2d(in_planes, out_planes, kernel_size=1, stride=stride, bias=False)


class ConvNormAct(nn.Sequential):
    def __init__(self, n_channels_in: int, n_channels_out: int, kernel_size: int = 1, dilation: int = 1,
                 stride: int = 1, normalization: Optional[Type[nn.Module]] = get_normalization_class(),
                 activation: Optional[Type[nn.Module]] = get_activation_class()) -> None:
        super().__init__()
        # the convolution carries a bias only when no normalization follows it
        self.add_module('conv', nn.Conv2d(n_channels_in, n_channels_out, kernel_size=kernel_size,
                                          padding=kernel_size // 2 + dilation - 1, dilation=dilation,
                                          stride=stride, bias=normalization is None))
        if normalization is not None:
            self.add_module('norm', normalization(n_channels_out))
        if activation is not None:
            self.add_module('act', activation())


class SqueezeAndExcitation(nn.Module):
    def __init__(self, n_channels: int, reduction: int = 16,
                 activation: Type[nn.Module] = get_activation_class()) -> None:
        super().__init__()
        n_channels_red = n_channels // reduction
        assert n_channels_red > 0
        self.layers = nn.Sequential(
            nn.Conv2d(n_channels, n_channels_red, kernel_size=1),
            activation(),
            nn.Conv2d(n_channels_red, n_channels, kernel_size=1),
            nn.Sigmoid(),
        )

    def forward(self, x: Tensor) -> Tensor:
        return x * self.layers(F.adaptive_avg_pool2d(x, 1))
