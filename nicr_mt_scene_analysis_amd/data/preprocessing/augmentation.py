"""`BatchAugmentation`: the numpy steps of the reference's training chain between the dataset and
the target generators, for a whole collated raw batch on the device in ONE launch
(`ops.batch_augment` -> `nmsa_batch_augment`):

  RandomCrop (crop.py:16-79) -> RandomHorizontalFlip (flip.py:14-55) -> NormalizeRGB ->
  NormalizeDepth (normalize.py:34-124) -> ToTorchTensors (torch.py:16-73)

The chain's other two steps, `RandomResize` and `RandomHSVJitter`, and the upscale of an image
smaller than the crop inside `RandomCrop`, go through cv2 (`INTER_LINEAR`, `cvtColor`) and are NOT
mirrored: a caller that needs them applies them before collation.  `ScaleDepth` is not part of
this step either.

The random draws are the reference's, per sample in batch order: `randint(0, H - crop_h)` only if
`H - crop_h > 0`, the same for x, then `uniform() <= p` (the high end of `randint` is exclusive:
the last offset is never drawn, as in the reference).  After `np.random.seed(s)` the parameter
table equals what the reference produces when it processes the samples one after the other
through RandomCrop -> RandomHorizontalFlip.

Deviations that are the device batch's, not this step's: tensors keep their on-wire dtypes (the
reference's `ToTorchTensors` widens uint16 to int32 and uint32 to int64 because torch once lacked
them); entries named in `keys_to_ignore` are left exactly as they are (the reference still
transposes them to CHW).
"""
from typing import Any, Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch

from ... import ops

RGB_MEAN = np.array((0.485, 0.456, 0.406), dtype='float32') * 255       # normalize.py:44-47
RGB_STD = np.array((0.229, 0.224, 0.225), dtype='float32') * 255


def mirror_orientation(angle: float) -> float:
    """flip.py:52-53: an angle mirrored at the y axis, in float64"""
    return (2 * np.pi - angle) % (2 * np.pi)


class BatchAugmentation:
    """__call__(batch, params=None): `batch` is a collated raw batch on the device — `rgb` uint8
    [B,H,W,3], `depth` uint16 or float32 [B,H,W], every other spatial tensor [B,H,W] or
    [B,H,W,C] — and comes back as the reference chain would have collated it: `rgb` float32
    [B,3,h,w] normalised with the ImageNet constants, `depth` float32 [B,1,h,w] normalised with
    `depth_mean` / `depth_std` (without them: cropped and flipped only, [B,1,h,w]), the others
    [B,h,w] / [B,C,h,w] as raw bits.  Spatial are the tensors `_get_relevant_spatial_keys` selects
    per sample: at least two dimensions below the batch dimension, not in `keys_to_ignore`; one
    whose sides are not the image's raises.  `orientations` (one dict per sample) is mirrored for
    flipped samples, in place, in float64 on the host.

    Surface normals are flipped SPATIALLY ONLY: the reference does not negate the x component of
    a flipped normal, and neither does this class.

    `params` supplies the integer [B,3] table of (y0, x0, flip) instead of drawing it; drawn
    tables use `rng` (`randint` / `uniform` of a `np.random.RandomState`) if given, else the
    module-level `np.random`.  `last_dynamic_parameters` holds per sample `crop_slice_y`,
    `crop_slice_x` and `was_flipped`.  Under hipGraph capture `captured_staging` is the
    `ops.AugmentStaging` the graph re-reads: `captured_staging.write_params(table)` before a
    replay makes the replay augment with that table (the host-side parts, `orientations` and
    `last_dynamic_parameters`, belong to the call, not to the graph)."""

    def __init__(self, crop_height: int, crop_width: int, flip_p: float,
                 depth_mean: Optional[float] = None, depth_std: Optional[float] = None,
                 raw_depth: bool = False, invalid_depth_value: float = 0.0,
                 keys_to_ignore: Optional[Iterable[str]] = None, rng=None) -> None:
        if (depth_mean is None) != (depth_std is None):
            raise ValueError('depth_mean and depth_std are given together or not at all')
        if depth_std is not None and depth_std == 0.0:
            raise ValueError('depth_std must not be 0')
        self._crop_height, self._crop_width, self._p = int(crop_height), int(crop_width), flip_p
        self._depth = None if depth_mean is None else (depth_mean, depth_std, raw_depth, invalid_depth_value)
        self._keys_to_ignore = None if keys_to_ignore is None else tuple(keys_to_ignore)
        self._rng = rng
        self.last_dynamic_parameters: List[Dict[str, Any]] = []
        self.captured_staging = None

    def _input_shape(self, batch: Dict[str, Any]) -> Tuple[int, int, int]:
        """utils.py:49-55: rgb, else depth"""
        if 'rgb' in batch:
            B, H, W, _ = batch['rgb'].shape
        else:
            B, H, W = batch['depth'].shape
        return int(B), int(H), int(W)

    def _spatial_keys(self, batch: Dict[str, Any], H: int, W: int) -> List[str]:
        keys = []
        for key, value in batch.items():
            if self._keys_to_ignore is not None and key in self._keys_to_ignore:
                continue
            if not isinstance(value, torch.Tensor) or value.ndim < 3:
                continue
            if value.ndim > 4 or tuple(value.shape[1:3]) != (H, W):
                raise ValueError(f"'{key}' has {value.ndim - 1} dimensions per sample, so the reference would "
                                 f'crop it, but its shape {tuple(value.shape)} is not [B,{H},{W}] or '
                                 f"[B,{H},{W},C]: name it in `keys_to_ignore`")
            keys.append(key)
        return keys

    def draw_params(self, B: int, H: int, W: int) -> np.ndarray:
        """the reference's draws (crop.py:58-65, flip.py:40), per sample in batch order"""
        r = np.random if self._rng is None else self._rng
        table = np.zeros((B, 3), np.int32)
        for b in range(B):
            if H - self._crop_height > 0:
                table[b, 0] = r.randint(0, H - self._crop_height)
            if W - self._crop_width > 0:
                table[b, 1] = r.randint(0, W - self._crop_width)
            table[b, 2] = r.uniform() <= self._p
        return table

    @staticmethod
    def mirror_orientations(orientations: List[Dict[int, float]], flipped: List[bool]) -> None:
        """flip.py:49-53, in place: the angles of the flipped samples mirrored at the y axis"""
        for of_sample, was_flipped in zip(orientations, flipped):
            if was_flipped:
                for id_ in of_sample:
                    of_sample[id_] = mirror_orientation(of_sample[id_])

    def __call__(self, batch: Dict[str, Any], params=None) -> Dict[str, Any]:
        if 'orientations_present' in batch:
            raise RuntimeError('Do not apply `BatchAugmentation` (its horizontal flip) after '
                               '`OrientationTargetGenerator`.')
        B, H, W = self._input_shape(batch)
        h, w = self._crop_height, self._crop_width
        if H < h or W < w:
            raise NotImplementedError(
                f'a {H} x {W} image is smaller than the {h} x {w} crop: the reference upscales it through '
                'cv2.resize (crop.py:43-55), which is not mirrored here')
        keys = self._spatial_keys(batch, H, W)
        table = self.draw_params(B, H, W) if params is None else ops.check_augment_params(params, B, (H, W), (h, w))
        norm = {}
        if 'rgb' in keys:
            norm['rgb'] = ('rgb_norm', RGB_MEAN, RGB_STD)
        if 'depth' in keys and self._depth is not None:
            norm['depth'] = ('depth_norm',) + self._depth
        out, staging = ops.batch_augment({k: batch[k] for k in keys}, table, (h, w), norm, return_staging=True)
        if torch.cuda.is_current_stream_capturing():
            self.captured_staging = staging
        for key, value in out.items():
            batch[key] = value.view(B, 1, h, w) if key == 'depth' and value.ndim == 3 else value
        flipped = [bool(f) for f in table[:, 2]]
        if 'orientations' in batch:
            self.mirror_orientations(batch['orientations'], flipped)
        self.last_dynamic_parameters = [
            {'crop_slice_y': slice(int(y0), int(y0) + h), 'crop_slice_x': slice(int(x0), int(x0) + w),
             'was_flipped': f} for (y0, x0, _), f in zip(table.tolist(), flipped)]
        return batch
