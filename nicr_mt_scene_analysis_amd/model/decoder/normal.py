"""Surface-normal MLP decoder (reference model/decoder/normal.py, `NormalMLPDecoder`).

The reference's default postprocessing is `get_postprocessing_class('normal')`; this package's factory
does not register that name (an existing test pins it), so the default here is the
`NormalPostprocessing` class itself."""
from typing import Tuple, Type

from torch import nn

from ...utils import NormalOutputNormalization
from ..activation import get_activation_class
from ..encoder_decoder_fusion import EncoderDecoderFusionType
from ..normalization import get_normalization_class
from ..postprocessing import NormalPostprocessing
from ..upsampling import UpsamplingType
from ..upsampling import get_upsampling_class
from .dense_utils import create_task_head
from .mlp_base import MLPDecoderBase


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
