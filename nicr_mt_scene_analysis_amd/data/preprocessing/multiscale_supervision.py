"""Side-output targets: `get_downscale` and the batch-level, on-device twin of
`MultiscaleSupervisionGenerator` (reference data/preprocessing/multiscale_supervision.py:16-67).

The reference clones the selected keys of a SAMPLE once per downscale d and resizes every spatial
entry of the clone to (int(h / d), int(w / d)) with `cv2.INTER_NEAREST` (resize.py:95-161).  Here
the whole collated BATCH is done on the device: every listed tensor [B,H,W] / [B,C,H,W] at every
downscale by ONE launch (`ops.multiscale_nearest` -> `nmsa_multiscale_nearest`), elements moved as
raw bits; the source indices are OpenCV's, evaluated on the host by `cv2_nearest_map`.  Listed
entries that are not spatial tensors (the `orientations` list of dicts, [B] tensors, per-image
lists) are deep-copied into every sub-batch, as the reference's `clone_entries` does.  The result
is `batch['_down_<d>']`; the generators that follow run on those sub-batches themselves
(`multiscale_processing`).
"""
from copy import deepcopy
from typing import Any, Dict, Optional, Tuple

import torch

from ... import ops
from ...ops import cv2_nearest_map      # noqa: F401  (the one host function that holds the index rule)
from .base import MULTI_DOWNSCALE_KEY_FMT


def get_downscale(sample: Dict[str, Any], downscale: int) -> Optional[Dict[str, Any]]:
    return sample.get(MULTI_DOWNSCALE_KEY_FMT.format(downscale), None)


class MultiscaleSupervisionGenerator:
    def __init__(self, downscales: Tuple[int], keys: Tuple[str]) -> None:
        self._downscales = downscales
        self._keys = keys
        self.last_dynamic_parameters: Dict[str, Any] = {}

    @property
    def downscales(self):
        return self._downscales

    def _input_shape(self, batch: Dict[str, Any]) -> Tuple[int, int]:
        """rgb, else depth (utils.py:48-54), else the first listed tensor: the last two dimensions"""
        for key in ('rgb', 'depth') + tuple(self._keys):
            value = batch.get(key)
            if isinstance(value, torch.Tensor) and value.ndim >= 2:
                return int(value.shape[-2]), int(value.shape[-1])
        raise ValueError(f"no tensor among 'rgb', 'depth' and {self._keys} to read the shape from")

    def __call__(self, batch: Dict[str, Any]) -> Dict[str, Any]:
        if not all(key in batch for key in self._keys):
            raise KeyError(f"At least one key of '{self._keys}' is missing in `sample`.")
        if 'rgb' in self._keys:
            raise NotImplementedError(
                "'rgb' is resized with cv2.INTER_LINEAR in the reference: not mirrored here")
        h, w = self._input_shape(batch)
        spatial = {key: batch[key] for key in self._keys
                   if isinstance(batch[key], torch.Tensor) and batch[key].ndim >= 3 and
                   tuple(batch[key].shape[-2:]) == (h, w)}
        resized = ops.multiscale_nearest(spatial, self._downscales, (h, w))
        shapes = {}
        for downscale in self._downscales:
            at_scale = resized[downscale]
            batch[MULTI_DOWNSCALE_KEY_FMT.format(downscale)] = {
                key: at_scale[key] if key in at_scale else deepcopy(batch[key]) for key in self._keys}
            shapes[downscale] = (int(h / downscale), int(w / downscale))
        self.last_dynamic_parameters = {'shapes': shapes}
        return batch
