"""Panoptic helper (reference model/decoder/panoptic.py, `PanopticHelper`): runs the semantic and the instance
decoder without their own postprocessing, combines the two raw outputs and applies the panoptic
postprocessing.  Plain torch; works with the MLP decoders of this package."""
from typing import Tuple, Type

from torch import nn

from ...types import BatchType
from ...types import DecoderInputType
from ...types import EncoderSkipsType
from ..postprocessing import get_postprocessing_class


class PanopticHelper(nn.Module):
    def __init__(
        self,
        semantic_decoder: nn.Module,
        instance_decoder: nn.Module,
        postprocessing: Type = get_postprocessing_class('panoptic'),
    ) -> None:
        super().__init__()
        self.semantic_decoder = semantic_decoder
        self.instance_decoder = instance_decoder
        self._postprocessing = postprocessing()             # the combined postprocessing

    @property
    def side_output_downscales(self) -> Tuple[int, ...]:
        scales = set(self.semantic_decoder.side_output_downscales)
        scales |= set(self.instance_decoder.side_output_downscales)
        return tuple(scales)

    @property
    def postprocessing(self):
        return self._postprocessing

    def forward(self, x: DecoderInputType, skips: EncoderSkipsType, batch: BatchType,
                do_postprocessing: bool = True):
        # both decoders skip their postprocessing, it is done on the combined output
        s_output, s_side_outputs = self.semantic_decoder.forward(x=x, skips=skips, batch=batch,
                                                                 do_postprocessing=False)
        i_output, i_side_outputs = self.instance_decoder.forward(x=x, skips=skips, batch=batch,
                                                                 do_postprocessing=False)
        output = (s_output, i_output), (s_side_outputs, i_side_outputs)
        if do_postprocessing:
            output = self._postprocessing.postprocess(output, batch, is_training=self.training)
        return output
