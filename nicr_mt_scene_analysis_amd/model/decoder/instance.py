"""Instance decoders and their head (reference model/decoder/instance.py, `InstanceHead`, the convolutional
`InstanceDecoder` over `DenseDecoderBase`, `InstanceMLPDecoder`).
The head is plain torch; its 'learned-3x3' upsamplings run on HIP."""
from math import log2
from typing import Optional, Tuple, Type

import torch
from torch import Tensor, nn

from ...utils import OrientationOutputNormalization
from ..activation import get_activation_class
from ..block import BlockType
from ..encoder_decoder_fusion import EncoderDecoderFusionType
from ..normalization import get_normalization_class
from ..postprocessing import get_postprocessing_class
from ..upsampling import UpsamplingType
from ..upsampling import get_upsampling_class
from ..utils import ConvNormAct
from .dense_base import DenseDecoderBase
from .mlp_base import MLPDecoderBase


class InstanceHead(nn.Module):
    """shared 3x3 ConvNormAct, one convolution per task on its slice of the shared features (center 1,
    offset 2, orientation 2 channels), the x2 upsamplings on the concatenated task outputs, then
    sigmoid / tanh / unit length per task"""

    def __init__(
        self,
        n_channels_in: int,
        n_channels_per_task: int = 32,
        with_orientation: bool = False,
        sigmoid_for_center: bool = True,
        tanh_for_offset: bool = True,
        normalization: Type[nn.Module] = get_normalization_class(),
        activation: Type[nn.Module] = get_activation_class(),
        upsampling: Optional[Type[UpsamplingType]] = None,
        n_upsamplings: int = 0
    ) -> None:
        super().__init__()
        self._n_tasks = 3 if with_orientation else 2
        self._n_channels_per_task = n_channels_per_task
        self._sigmoid_for_center = sigmoid_for_center
        self._tanh_for_offset = tanh_for_offset
        self.shared_conv = ConvNormAct(n_channels_in, self._n_tasks * n_channels_per_task, kernel_size=3,
                                       normalization=normalization, activation=activation)
        kernel_size = 3 if n_upsamplings != 0 else 1        # main output / side output
        n_outs = (1, 2, 2)[:self._n_tasks]
        if with_orientation:
            self._act_orientation = OrientationOutputNormalization()
        self.task_convs = nn.ModuleList(
            nn.Conv2d(n_channels_per_task, n, kernel_size=kernel_size, padding=(kernel_size - 1) // 2)
            for n in n_outs)
        self.upsampling = nn.Sequential(*(upsampling(n_channels=sum(n_outs)) for _ in range(n_upsamplings)))

    def forward(self, x: Tensor) -> Tuple[Tensor, ...]:
        x = self.shared_conv(x)
        n = self._n_channels_per_task
        outs = [conv(x[:, i * n:(i + 1) * n]) for i, conv in enumerate(self.task_convs)]
        outs_cat = self.upsampling(torch.cat(outs, dim=1))
        outs = list(torch.split(outs_cat, [int(o.shape[1]) for o in outs], dim=1))
        if self._sigmoid_for_center:
            outs[0] = torch.sigmoid(outs[0])
        if self._tanh_for_offset:
            outs[1] = torch.tanh(outs[1])
        if self._n_tasks == 3:
            outs[2] = self._act_orientation(outs[2])
        return tuple(outs)


class InstanceDecoder(DenseDecoderBase):
    def __init__(
        self,
        n_channels_in: int,
        downsampling_in: int,
        n_channels: Tuple[int, ...],
        downsamplings: Tuple[int, ...],
        block: Type[BlockType],
        n_blocks: int,
        fusion: Type[EncoderDecoderFusionType],
        fusion_n_channels: Tuple[int, ...],
        fusion_downsamplings: Tuple[int, ...],
        n_channels_per_task: int = 32,
        with_orientation: bool = False,
        sigmoid_for_center: bool = True,
        tanh_for_offset: bool = True,
        postprocessing: Type = get_postprocessing_class('instance'),
        normalization: Type[nn.Module] = get_normalization_class(),
        activation: Type[nn.Module] = get_activation_class(),
        upsampling: Type[UpsamplingType] = get_upsampling_class(),
        prediction_upsampling: Type[UpsamplingType] = get_upsampling_class()
    ) -> None:
        super().__init__(n_channels_in=n_channels_in, downsampling_in=downsampling_in, n_channels=n_channels,
                         downsamplings=downsamplings, block=block, n_blocks=n_blocks, fusion=fusion,
                         fusion_n_channels=fusion_n_channels, fusion_downsamplings=fusion_downsamplings,
                         postprocessing=postprocessing, normalization=normalization, activation=activation,
                         upsampling=upsampling)

        def head(n_channels_in, upsampling, n_upsamplings):
            return InstanceHead(n_channels_in=n_channels_in, n_channels_per_task=n_channels_per_task,
                                with_orientation=with_orientation, sigmoid_for_center=sigmoid_for_center,
                                tanh_for_offset=tanh_for_offset, normalization=normalization, activation=activation,
                                upsampling=upsampling, n_upsamplings=n_upsamplings)

        # the main head upsamples to the input resolution; a side head stays at its own scale
        self._task_head = head(n_channels[-1], prediction_upsampling, int(log2(downsamplings[-1])))
        self._side_output_heads = nn.ModuleList(head(n, None, 0) for n in self.side_output_n_channels)

    @property
    def task_head(self) -> nn.Module:
        return self._task_head

    @property
    def side_output_heads(self) -> nn.ModuleList:
        return self._side_output_heads


class InstanceMLPDecoder(MLPDecoderBase):
    def __init__(
        self,
        n_channels_in: int,
        downsampling_in: int,
        n_channels: Tuple[int, ...],
        fusion: Type[EncoderDecoderFusionType],
        fusion_n_channels: Tuple[int, ...],
        fusion_downsamplings: Tuple[int, ...],
        n_channels_per_task: int = 32,
        with_orientation: bool = False,
        sigmoid_for_center: bool = True,
        tanh_for_offset: bool = True,
        downsampling_in_heads: int = 4,
        dropout_p: float = 0.1,
        postprocessing: Type = get_postprocessing_class('instance'),
        normalization: Type[nn.Module] = get_normalization_class(),
        activation: Type[nn.Module] = get_activation_class(),
        upsampling: Type[UpsamplingType] = get_upsampling_class(),
        prediction_upsampling: Type[UpsamplingType] = get_upsampling_class()
    ) -> None:
        super().__init__(n_channels_in=n_channels_in, downsampling_in=downsampling_in, n_channels=n_channels,
                         fusion=fusion, fusion_n_channels=fusion_n_channels,
                         fusion_downsamplings=fusion_downsamplings, downsampling_in_heads=downsampling_in_heads,
                         dropout_p=dropout_p, postprocessing=postprocessing, normalization=normalization,
                         activation=activation, upsampling=upsampling)
        self._downsampling_in_heads = downsampling_in_heads
        self._task_head = InstanceHead(n_channels_in=sum(n_channels) // len(n_channels),
                                       n_channels_per_task=n_channels_per_task, with_orientation=with_orientation,
                                       sigmoid_for_center=sigmoid_for_center, tanh_for_offset=tanh_for_offset,
                                       normalization=normalization, activation=activation,
                                       upsampling=prediction_upsampling,
                                       n_upsamplings=self._downsampling_in_heads // 2)

    @property
    def task_head(self) -> nn.Module:
        return self._task_head
