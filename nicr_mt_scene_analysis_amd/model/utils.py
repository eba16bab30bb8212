"""Building blocks of the model (reference model/utils.py); only what the encoder-decoder fusion
needs: `ConvNormAct`, a convolution (1x1 by default) followed by a normalization and an activation,
with the reference's sub-module names `conv`, `norm`, `act`.  Plain torch."""
from typing import Optional, Type

from torch import nn

from .activation import get_activation_class
from .normalization import get_normalization_class


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
