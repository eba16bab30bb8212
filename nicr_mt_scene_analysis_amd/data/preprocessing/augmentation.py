"""`BatchAugmentation`: the numpy and resize steps of the reference's training chain between the
dataset and the target generators, for a whole collated raw batch on the device in ONE launch:

  RandomResize (resize.py:288-340) -> RandomCrop (crop.py:16-79) -> RandomHorizontalFlip
  (flip.py:14-55) -> NormalizeRGB -> NormalizeDepth (normalize.py:34-124) -> ToTorchTensors
  (torch.py:16-73)

A batch in which no sample is resized takes `ops.batch_augment` -> `nmsa_batch_augment`
(csrc/augment.hip), as it did before `RandomResize` was mirrored.  With `min_scale` / `max_scale`,
or with `upscale_too_small` and an image smaller than the crop (crop.py:43-55), it takes
`ops.batch_augment_resized` -> `nmsa_batch_augment_resized` (csrc/augment_resize.hip): the host
evaluates OpenCV's index and weight rules for the pixels of each sample's crop window
(`ops.cv2_nearest_map_vec`, `ops.cv2_linear_taps`) and the kernel resamples only those, `rgb` as
cv2.INTER_LINEAR on 8-bit pixels, everything else as cv2.INTER_NEAREST.  THE 8-BIT LINEAR RULE AND
THE NEAREST RULE ARE WRITTEN DOWN FROM OPENCV'S SOURCE AND HAVE NOT BEEN COMPARED WITH A REAL cv2
BUILD.

Still NOT mirrored: `RandomHSVJitter` (`cvtColor`), `ScaleDepth`, `Resize` with padding, and a
sample that the reference would resize TWICE — scales so small that the rescaled image is smaller
than the crop, which `RandomCrop` then upscales again from the rounded uint8 image; one resampling
cannot reproduce that, and the configuration is refused (from shapes alone, never from a draw).

The random draws are the reference's, per sample in batch order: `uniform(min_scale, max_scale)`
only if the two differ, `randint(0, rh - crop_h)` only if `rh - crop_h > 0` on the resized size,
the same for x, then `uniform() <= p` (the high end of `randint` is exclusive: the last offset is
never drawn, as in the reference).  After `np.random.seed(s)` the parameter table equals what the
reference produces when it processes the samples one after the other through RandomResize ->
RandomCrop -> RandomHorizontalFlip.

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

    `min_scale` / `max_scale` are RandomResize's; `upscale_too_small` lets an image smaller than
    the crop be upscaled as RandomCrop does (without it, that case raises NotImplementedError).
    With all three at their defaults nothing is resized.  `rgb` must be uint8 where a resize is
    configured.

    `params` supplies the parameter table instead of drawing it: integer [B,5], (y0, x0, flip, rh,
    rw) with the resized size rh x rw and the crop offset inside it, or, where no resize is
    configured, [B,3], (y0, x0, flip).  A [B,5] table is taken whatever the configuration, also
    by an object built without scales: it is how sizes of the caller's own (one per sample, as
    the reference's `resize()` would be given them) are applied, the rows whose (rh, rw) differ
    from the source's are resized, and `old_height` .. `new_width` are then recorded as for a
    rescale.  Drawn tables use `rng` (`randint` / `uniform` of a
    `np.random.RandomState`) if given, else the module-level `np.random`.
    `last_dynamic_parameters` holds per sample `crop_slice_y`, `crop_slice_x` and `was_flipped`,
    and the reference's `old_height`, `old_width`, `new_height`, `new_width` for a rescale or
    `was_resized`, `resize_height`, `resize_width` for an upscale.  Under hipGraph capture
    `captured_staging` is the `ops.AugmentStaging` / `ops.AugmentResizeStaging` the graph
    re-reads — of the launch the captured table selected —: `captured_staging.write_params(table)`
    before a replay makes the replay augment with that table (the host-side parts, `orientations`
    and `last_dynamic_parameters`, belong to the call, not to the graph)."""

    def __init__(self, crop_height: int, crop_width: int, flip_p: float,
                 depth_mean: Optional[float] = None, depth_std: Optional[float] = None,
                 raw_depth: bool = False, invalid_depth_value: float = 0.0,
                 keys_to_ignore: Optional[Iterable[str]] = None, rng=None,
                 min_scale: Optional[float] = None, max_scale: Optional[float] = None,
                 upscale_too_small: bool = False) -> None:
        if (depth_mean is None) != (depth_std is None):
            raise ValueError('depth_mean and depth_std are given together or not at all')
        if depth_std is not None and depth_std == 0.0:
            raise ValueError('depth_std must not be 0')
        if (min_scale is None) != (max_scale is None):
            raise ValueError('min_scale and max_scale are given together or not at all')
        if min_scale is not None and (min_scale < 0 or min_scale > max_scale):
            raise ValueError('Unexpected value for `min_scale`')                 # resize.py:295-296
        self._crop_height, self._crop_width, self._p = int(crop_height), int(crop_width), flip_p
        self._depth = None if depth_mean is None else (depth_mean, depth_std, raw_depth, invalid_depth_value)
        self._keys_to_ignore = None if keys_to_ignore is None else tuple(keys_to_ignore)
        self._rng = rng
        self._scales = None if min_scale is None else (min_scale, max_scale)
        self._upscale_too_small = bool(upscale_too_small)
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

    def resize_mode(self, H: int, W: int) -> Optional[str]:
        """'rescale' (RandomResize), 'upscale' (RandomCrop's, to `upscaled_size`) or None for an
        H x W batch; the refusals depend on the shapes and the configuration only"""
        h, w = self._crop_height, self._crop_width
        if self._scales is not None:
            lo = self._scales[0]
            if int(round(lo * H)) < h or int(round(lo * W)) < w:
                raise NotImplementedError(
                    f'a {H} x {W} image rescaled by {lo} can be smaller than the {h} x {w} crop: the reference '
                    'then resizes twice through cv2.resize (resize.py:330, crop.py:43-55), with a rounding to '
                    'uint8 in between that one resampling cannot reproduce')
            return 'rescale'
        if H < h or W < w:
            if not self._upscale_too_small:
                raise NotImplementedError(
                    f'a {H} x {W} image is smaller than the {h} x {w} crop: the reference upscales it through '
                    'cv2.resize (crop.py:43-55), which is mirrored only with `upscale_too_small=True`')
            return 'upscale'
        return None

    def upscaled_size(self, H: int, W: int) -> Tuple[int, int]:
        """crop.py:43-53"""
        scale = 1.0
        if H <= self._crop_height:
            scale = max(self._crop_height / H, scale)
        if W <= self._crop_width:
            scale = max(self._crop_width / W, scale)
        return int(H * scale + 0.5), int(W * scale + 0.5)

    def draw_params(self, B: int, H: int, W: int) -> np.ndarray:
        """the reference's draws (resize.py:320-327, crop.py:58-65, flip.py:40), per sample in batch
        order -> i32 [B,3] (y0, x0, flip), or [B,5] (y0, x0, flip, rh, rw) where `resize_mode`
        names a resize"""
        mode = self.resize_mode(H, W)
        r = np.random if self._rng is None else self._rng
        table = np.zeros((B, 3 if mode is None else 5), np.int32)
        rh, rw = self.upscaled_size(H, W) if mode == 'upscale' else (H, W)
        for b in range(B):
            if mode == 'rescale':
                lo, hi = self._scales
                scale = lo if lo == hi else r.uniform(lo, hi)
                rh, rw = int(round(scale * H)), int(round(scale * W))
            if rh - self._crop_height > 0:
                table[b, 0] = r.randint(0, rh - self._crop_height)
            if rw - self._crop_width > 0:
                table[b, 1] = r.randint(0, rw - self._crop_width)
            table[b, 2] = r.uniform() <= self._p
            if mode is not None:
                table[b, 3:] = (rh, rw)
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
        mode = self.resize_mode(H, W)
        keys = self._spatial_keys(batch, H, W)
        if mode is not None and 'rgb' in keys and batch['rgb'].dtype != torch.uint8:
            raise ValueError(f"`rgb` is {batch['rgb'].dtype}: behind a resize it must be uint8 (the reference's "
                             'cv2.INTER_LINEAR is mirrored for 8-bit images only)')
        if params is None:
            table = self.draw_params(B, H, W)
        elif np.asarray(params).ndim == 2 and np.asarray(params).shape[1] == 5:
            table = ops.check_augment_resize_params(params, B, (h, w))
        elif mode is None:
            table = ops.check_augment_params(params, B, (H, W), (h, w))
        else:
            raise ValueError(f'with a resize configured, params must be {B} integer rows (y0, x0, flip, rh, rw)')
        norm = {}
        if 'rgb' in keys:
            norm['rgb'] = ('rgb_norm', RGB_MEAN, RGB_STD)
        if 'depth' in keys and self._depth is not None:
            norm['depth'] = ('depth_norm',) + self._depth
        tensors = {k: batch[k] for k in keys}
        # a batch in which no sample is resized takes the launch it took before there was a resize
        if table.shape[1] == 5 and ((table[:, 3] != H) | (table[:, 4] != W)).any():
            out, staging = ops.batch_augment_resized(tensors, table, (h, w), norm, return_staging=True)
        else:
            out, staging = ops.batch_augment(tensors, table[:, :3], (h, w), norm, return_staging=True)
        if torch.cuda.is_current_stream_capturing():
            self.captured_staging = staging
        for key, value in out.items():
            batch[key] = value.view(B, 1, h, w) if key == 'depth' and value.ndim == 3 else value
        flipped = [bool(f) for f in table[:, 2]]
        if 'orientations' in batch:
            self.mirror_orientations(batch['orientations'], flipped)
        self.last_dynamic_parameters = [
            {'crop_slice_y': slice(int(y0), int(y0) + h), 'crop_slice_x': slice(int(x0), int(x0) + w),
             'was_flipped': f} for (y0, x0, *_), f in zip(table.tolist(), flipped)]
        if table.shape[1] == 5:
            for recorded, (_, _, _, rh, rw) in zip(self.last_dynamic_parameters, table.tolist()):
                if mode == 'upscale':
                    recorded.update(was_resized=True, resize_height=rh, resize_width=rw)
                else:
                    recorded.update(old_height=H, old_width=W, new_height=rh, new_width=rw)
        return batch
