"""Batch-level, on-device twin of the reference's orientation target preprocessing
(reference data/preprocessing/orientation.py:17-97).

The reference paints, per SAMPLE in numpy, the biternion (cos, sin) of every instance that has an
entry in `sample['orientations']` over the instance's mask, when the majority semantic class of
the mask is one whose orientation is estimated.  Here the whole BATCH is done on the device
(`nmsa_orientation_targets`): `semantic` uint8 [B,H,W], `instance` int32 [B,H,W] holding uint16
ids, `orientations` a list of B dicts {instance id: angle in rad}, as the reference's collate
leaves it.  Written keys, as a collated reference batch holds them: `orientation` f32 [B,2,H,W]
(channel 0 cos, channel 1 sin), `orientation_foreground` bool [B,H,W], `orientations_present` a
list of B dicts.  The biternions are computed on the host with the reference's numpy expression,
so the painted values are bit-identical; the per-image key tables travel in ONE pinned buffer and
one asynchronous copy, and one small device-to-host copy (flags of the painted keys + status) is
the only synchronisation.  With `multiscale_processing` (the reference's default: on) the
generator runs again on every `batch['_down_<k>']` sub-batch, one such copy per scale.
"""
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch

from ... import ops
from ...utils import np_rad2biternion
from .base import apply_to_downscales
from .instance import _device_lut

_KEY_PAD = 64               # K is padded to a multiple: the shapes stay stable from batch to batch
_MAX_KEYS = 4096


class OrientationTargetGenerator:
    def __init__(
        self,
        semantic_classes_estimate_orientation: Optional[Tuple[bool]] = None,     # with void
        max_instances: int = 1024,
        multiscale_processing: bool = True,
        **kwargs
    ) -> None:
        self._multiscale_processing = multiscale_processing
        if semantic_classes_estimate_orientation is not None:
            self._estimate = np.asarray(semantic_classes_estimate_orientation, dtype=bool)
            self._n_classes = len(self._estimate)
        else:
            self._estimate = None
            self._n_classes = None
        self._max_instances = max_instances
        self._luts: Dict = {}
        self._staging: Dict = {}

    def _pack(self, orientations, dev: torch.device):
        """per image the ids in [1, 65535] ascending; keys i32 [B,K] | biternion f32 [B,K,2] |
        n_keys i32 [B] in one pinned buffer, one asynchronous copy"""
        B = len(orientations)
        ids = [sorted(int(i) for i in d if 1 <= int(i) <= 65535) for d in orientations]
        longest = max((len(i) for i in ids), default=0)
        K = max(_KEY_PAD, -(-longest // _KEY_PAD) * _KEY_PAD)
        if K > _MAX_KEYS:
            raise ValueError(f'more than {_MAX_KEYS} orientations in one image')
        if (B, K, dev) not in self._staging:
            n = 3 * B * K + B
            self._staging[(B, K, dev)] = (torch.empty((n,), dtype=torch.int32).pin_memory(),
                                          torch.empty((n,), dtype=torch.int32, device=dev))
        host, device = self._staging[(B, K, dev)]
        packed = host.numpy()
        packed[:] = 0
        keys = packed[:B * K].reshape(B, K)
        bit = packed[B * K:3 * B * K].view(np.float32).reshape(B, K, 2)
        n_keys = packed[3 * B * K:]
        for b, (d, i) in enumerate(zip(orientations, ids)):
            # (a dict may be keyed by numpy integers: look the angle up under the caller's key)
            by_int = {int(k): k for k in d}
            keys[b, :len(i)] = i
            for k, iid in enumerate(i):
                bit[b, k] = np_rad2biternion(d[by_int[iid]])
            n_keys[b] = len(i)
        device.copy_(host, non_blocking=True)
        return (ids, device[:B * K].view(B, K), device[3 * B * K:],
                device[B * K:3 * B * K].view(torch.float32).view(B, K, 2))

    def __call__(self, batch: Dict[str, Any], n_classes: Optional[int] = None) -> Dict[str, Any]:
        batch = self._preprocess(batch, n_classes)
        if self._multiscale_processing:
            apply_to_downscales(batch, lambda sub, downscale: self._preprocess(sub, n_classes))
        return batch

    def _preprocess(self, batch: Dict[str, Any], n_classes: Optional[int] = None) -> Dict[str, Any]:
        if not all(k in batch for k in ('instance', 'orientations', 'semantic')):
            return batch                      # inference / no orientation labels (orientation.py:43-47)
        sem, ins, orientations = batch['semantic'], batch['instance'], batch['orientations']
        dev = sem.device
        B = sem.shape[0]
        if len(orientations) != B:
            raise ValueError(f'{len(orientations)} orientation dicts for a batch of {B}')
        est = None if self._estimate is None else _device_lut(self._estimate, dev, self._luts)
        nc = self._n_classes or n_classes or 256
        ids, keys, n_keys, bit = self._pack(orientations, dev)
        while True:
            r = ops.orientation_targets(sem, ins, nc, est, keys, n_keys, bit, self._max_instances)
            host = torch.cat([r['status'].view(torch.uint8), r['present'].reshape(-1)]).cpu().numpy()
            status = int(host[:4].view(np.int32)[0])
            if status & 1 and self._max_instances < 4096:
                self._max_instances = min(4096, self._max_instances * 4)
                continue
            break
        if status & 32:
            raise ValueError('instance ids outside [0, 65535]')
        if status & 64:
            raise ValueError(f'semantic labels outside [0, {nc})')
        if status & 1:
            raise NotImplementedError('more than 4096 distinct instance ids in one image')
        present = host[4:].reshape(B, -1)
        batch['orientation'] = r['orientation']
        batch['orientation_foreground'] = r['foreground']
        # ascending ids = the np.unique order the reference fills its dict in, the caller's angles
        out = []
        for b, (d, i) in enumerate(zip(orientations, ids)):
            by_int = {int(k): k for k in d}
            out.append({iid: d[by_int[iid]] for k, iid in enumerate(i) if present[b, k]})
        batch['orientations_present'] = out
        return batch
