"""Surface-normal decoders (reference model/decoder/normal.py): the convolutional `NormalDecoder` over
`DenseDecoderBase` and the `NormalMLPDecoder`.

The reference's default postprocessing is `get_postprocessing_class('normal')`; this package's factory
does not register that name (an existing test pins it), so the default here is the
`NormalPostprocessing` class itself."""
from math import log2
from typing import Tuple, Type

from torch import nn

from ...utils import NormalOutputNormalization
from ..activation import get_activation_class
from ..block import BlockType
from ..encoder_decoder_fusion import EncoderDecoderFusionType
from ..normalization import get_normalization_class
from ..postprocessing import NormalPostprocessing
from ..upsampling import UpsamplingType
from ..upsampling import get_upsampling_class
from .dense_base import DenseDecoderBase
from .dense_utils import create_task_head
from .mlp_base import MLPDecoderBase


class NormalDecoder(DenseDecoderBase):
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
        n_channels_out: int = 3,
        postprocessing: Type = NormalPostprocessing,
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
        self._n_channels_out = n_channels_out
        # every head ends in the unit-length normalization
        self._task_head = create_task_head(n_channels_in=n_channels[-1], n_channels_out=self._n_channels_out,
                                           upsampling=prediction_upsampling,
                                           n_upsamplings=int(log2(downsamplings[-1])),
                                           post_modules=[NormalOutputNormalization()])
        self._side_output_heads = nn.ModuleList(
            create_task_head(n_channels_in=n, n_channels_out=self._n_channels_out,
                             post_modules=[NormalOutputNormalization()])
            for n in self.side_output_n_channels)

    @property
    def task_head(self) -> nn.Module:
        return self._task_head

    @property
    def side_output_heads(self) -> nn.ModuleList:
        return self._side_output_heads


class NormalMLPDecoder(MLPDecoderBase):
    def __init__(
        self,
        n_channels_in: int,
        downsampling_in: int,
        n_channels: Tuple[int, ...],
        fusion: Type[EncoderDecoderFusionType],
        fusion_n_channels: Tuple[int, ...],
        fusion_downsamplings: Tuple[int, ...],
        n_channels_out: int = 3,
        downsampling_in_heads: int = 4,
        dropout_p: float = 0.1,
        postprocessing: Type = NormalPostprocessing,
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
        self._n_channels_out = n_channels_out
        self._downsampling_in_heads = downsampling_in_heads
        self._task_head = create_task_head(n_channels_in=sum(n_channels) // len(n_channels),
                                           n_channels_out=self._n_channels_out, upsampling=prediction_upsampling,
                                           n_upsamplings=self._downsampling_in_heads // 2,
                                           post_modules=[NormalOutputNormalization()])

    @property
    def task_head(self) -> nn.Module:
        return self._task_head
