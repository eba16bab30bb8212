"""Adaptive pyramid pooling module (reference model/context_module/appm.py) on the HIP kernels of
csrc/context_module.hip: as `PyramidPoolingModule` (see context_module/ppm.py for the launches, the
autograd functions, the dtype rule and the stated deviations), but the pool sizes follow the input:
bin * int(h / h_inp + 0.5) rows and bin * int(w / w_inp + 0.5) columns for the `input_size`
(h_inp, w_inp) the module was built for.  Index 0 of each branch is `nn.Identity()`, as in the
reference, so PPM and APPM checkpoints are interchangeable."""
from typing import Tuple, Type

import torch.nn as nn

from ... import ops
from ...types import ContextModuleInputType
from ...types import ContextModuleOutputType
from ..activation import get_activation_class
from ..normalization import get_normalization_class
from ..utils import ConvNormAct
from .ppm import pyramid_forward


class AdaptivePyramidPoolingModule(nn.Module):
    def __init__(
        self,
        n_channels_in: int,
        n_channels_out: int,
        input_size: Tuple[int, int],
        bins: Tuple[int, ...] = (1, 2, 3, 6),
        normalization: Type[nn.Module] = get_normalization_class(),
        activation: Type[nn.Module] = get_activation_class(),
        upsampling: str = 'bilinear'
    ) -> None:
        super().__init__()
        ops._ppm_sizes(bins)                                # 1..4 bins, each at least 1
        n_channels_reduction = n_channels_in // len(bins)
        self._upsampling = upsampling
        self._input_size = input_size
        self._bins = tuple(bins)

        features = []
        for _ in bins:
            features.append(nn.Sequential(
                nn.Identity(),                              # to make ppm and appm interchangeable
                ConvNormAct(n_channels_in, n_channels_reduction, kernel_size=1,
                            normalization=normalization, activation=activation)
            ))
        self.features = nn.ModuleList(features)

        n_channels_in_last_conv = n_channels_in + n_channels_reduction * len(bins)
        self.final_conv = ConvNormAct(n_channels_in_last_conv, n_channels_out, kernel_size=1,
                                      normalization=normalization, activation=activation)
        self.n_channels_reduction = n_channels_reduction

    def pool_sizes(self, h: int, w: int) -> Tuple[Tuple[int, int], ...]:
        """the (rows, columns) of every pool for an input of h x w"""
        h_inp, w_inp = self._input_size
        bin_multiplier_h = int((h / h_inp) + 0.5)
        bin_multiplier_w = int((w / w_inp) + 0.5)
        return tuple((bin_ * bin_multiplier_h, bin_ * bin_multiplier_w) for bin_ in self._bins)

    def forward(self, x: ContextModuleInputType) -> ContextModuleOutputType:
        h, w = x.shape[2:]
        return pyramid_forward(self, x, self.pool_sizes(int(h), int(w)))
