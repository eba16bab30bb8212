"""`NormalPostprocessing` on the MI355X (reference model/postprocessing/normal.py:14-64).

Training is a pass-through.  At inference the reference crops the prediction to the valid
region and resizes it (nearest) to the dataset resolution at once; here that B x 3 x H x W map
is a lazy entry produced by `nmsa_resize_nearest` when somebody reads it — the task helper's
RMSE reads the network-resolution output instead (`.aux`, see
`RootMeanSquaredError.update_from_network_resolution`).
"""
import torch

from ... import ops
from ...data.preprocessing.resize import get_fullres_key
from ...data.preprocessing.resize import get_valid_region_slices_and_fullres_shape
from ...types import BatchType
from ...types import DecoderRawOutputType
from ...types import PostprocessingOutputType
from ._lazy import LazyDict
from .dense_base import DensePostprocessingBase

# .aux entry for in-package consumers: (network-resolution output, valid-region slices)
AUX_SOURCE_KEY = 'normal_output_fullres_source'


def _resize_nearest_any_float(output: torch.Tensor, shape, crop) -> torch.Tensor:
    """nearest resize moves elements unchanged: bf16 / f16 maps travel as their 16-bit patterns"""
    if output.dtype in (torch.bfloat16, torch.float16):
        return ops.resize_nearest(output.view(torch.int16), shape, crop).view(output.dtype)
    return ops.resize_nearest(output, shape, crop)


class NormalPostprocessing(DensePostprocessingBase):
    def __init__(self, **kwargs) -> None:
        super().__init__()

    def _postprocess_training(
        self, data: DecoderRawOutputType, batch: BatchType
    ) -> PostprocessingOutputType:
        output, side_outputs = data
        return {'normal_output': output, 'normal_side_outputs': side_outputs}

    def _postprocess_inference(
        self, data: DecoderRawOutputType, batch: BatchType
    ) -> PostprocessingOutputType:
        output, side_outputs = data
        r = LazyDict(normal_output=output, normal_side_outputs=side_outputs)
        crop, shape = get_valid_region_slices_and_fullres_shape(batch, 'normal')
        shape = tuple(int(n) for n in shape)
        cropped = output[..., crop[0], crop[1]]
        key = get_fullres_key('normal_output')
        if tuple(cropped.shape[-2:]) == shape:
            r[key] = cropped                    # nothing to resize (dense_base.py:28-31): a view
        else:
            r.set_lazy(key, lambda: _resize_nearest_any_float(output, shape, crop))
        r.aux[AUX_SOURCE_KEY] = (output, crop)
        return r
