"""Semantic decoders (reference model/decoder/semantic.py): the convolutional `SemanticDecoder` over
`DenseDecoderBase` and the `SemanticMLPDecoder`."""
from math import log2
from typing import Optional, Tuple, Type

from torch import nn

from ..activation import get_activation_class
from ..block import BlockType
from ..encoder_decoder_fusion import EncoderDecoderFusionType
from ..normalization import get_normalization_class
from ..postprocessing import get_postprocessing_class
from ..upsampling import UpsamplingType
from ..upsampling import get_upsampling_class
from .dense_base import DenseDecoderBase
from .dense_utils import create_task_head
from .mlp_base import MLPDecoderBase


class SemanticDecoder(DenseDecoderBase):
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
        n_classes: int,
        postprocessing: Type = get_postprocessing_class('semantic'),
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
        self._n_classes = n_classes
        # the main head upsamples to the input resolution; a side head is a 1x1 convolution at its own scale
        self._task_head = create_task_head(n_channels_in=n_channels[-1], n_channels_out=self._n_classes,
                                           upsampling=prediction_upsampling,
                                           n_upsamplings=int(log2(downsamplings[-1])))
        self._side_output_heads = nn.ModuleList(
            create_task_head(n_channels_in=n, n_channels_out=self._n_classes) for n in self.side_output_n_channels)

    @property
    def task_head(self) -> nn.Module:
        return self._task_head

    @property
    def side_output_heads(self) -> nn.ModuleList:
        return self._side_output_heads


class SemanticMLPDecoder(MLPDecoderBase):
    def __init__(
        self,
        n_channels_in: int,
        downsampling_in: int,
        n_channels: Tuple[int, ...],
        fusion: Type[EncoderDecoderFusionType],
        fusion_n_channels: Tuple[int, ...],
        fusion_downsamplings: Tuple[int, ...],
        n_classes: int,
        downsampling_in_heads: int = 4,
        dropout_p: float = 0.1,
        n_channels_out: Optional[int] = None,
        n_upsamplings: Optional[int] = None,
        postprocessing: Type = get_postprocessing_class('semantic'),
        normalization: Type[nn.Module] = get_normalization_class(),
        activation: Type[nn.Module] = get_activation_class(),
        upsampling: Type[UpsamplingType] = get_upsampling_class(),
        prediction_upsampling: Type[UpsamplingType] = get_upsampling_class()
    ) -> None:
        # as in the reference, n_channels_out sizes the head only: `fuse` keeps its own default
        super().__init__(n_channels_in=n_channels_in, downsampling_in=downsampling_in, n_channels=n_channels,
                         fusion=fusion, fusion_n_channels=fusion_n_channels,
                         fusion_downsamplings=fusion_downsamplings, downsampling_in_heads=downsampling_in_heads,
                         dropout_p=dropout_p, postprocessing=postprocessing, normalization=normalization,
                         activation=activation, upsampling=upsampling)
        self._n_classes = n_classes
        self._downsampling_in_heads = downsampling_in_heads
        if n_channels_out is None:
            n_channels_out = sum(n_channels) // len(n_channels)
        if n_upsamplings is None:
            n_upsamplings = self._downsampling_in_heads // 2    # each doubles the resolution
        self._task_head = create_task_head(n_channels_in=n_channels_out, n_channels_out=self._n_classes,
                                           upsampling=prediction_upsampling, n_upsamplings=n_upsamplings)

    @property
    def task_head(self) -> nn.Module:
        return self._task_head
