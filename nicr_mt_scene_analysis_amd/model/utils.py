"""Building blocks of the model (reference model/utils.py), plain torch:
`ConvNormAct`, a convolution (1x1 by default) followed by a normalization and an activation, with the
reference's sub-module names `conv`, `norm`, `act` (the encoder-decoder fusion's channel adapter);
`SqueezeAndExcitation`, the channel weighting of the encoder RGB-D fusion, with the reference's
sub-module layout `layers.{0..3}`.  `model.encoder_fusion` reads its parameters for the fused HIP path
and calls it as it is everywhere else;
`conv3x3` and `conv1x1`, the bias-free convolutions of the residual blocks (`model.block`);
`fused_map` and `f32_master`, what every module with a fused HIP path asks of its input map and does to its
parameters before it hands them to the kernels."""
from typing import Optional, Tuple, Type

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from .activation import get_activation_class
from .normalization import get_normalization_class

FUSED_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def fused_map(x: Tensor) -> bool:
    """whether `x` is a map the fused HIP paths take: on the device, 4-D, float32 / bfloat16 / float16, not empty,
    dense NCHW.  Each module adds its own terms (channel limits, thresholds, a second tensor)."""
    return bool(x.is_cuda and x.ndim == 4 and x.dtype in FUSED_DTYPES and x.numel() > 0 and x.is_contiguous())


def f32_master(*tensors: Optional[Tensor]) -> Tuple[Optional[Tensor], ...]:
    """the parameters as the kernels take them, float32: each tensor itself when it is float32 already, a cast
    copy after `module.half()`, None for None"""
    return tuple([t if t is None or t.dtype == torch.float32 else t.float() for t in tensors])


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
