"""Device-side stand-ins for "a list of B dicts" (extension; the reference keeps Python dicts).

`OrientationTable`: per image {integer key: angle in rad}, what
`InstancePostprocessing._get_instance_orientation` returns and `batch['orientations_present']`
holds.  `IdTable`: per image {panoptic id: instance id}, what the merge returns next to the
panoptic map and `batch['panoptic_ids_to_instance_dict']` holds.  The orientation metrics
(metric/mae.py) join such tables on the device (csrc/maae.hip); `to_dicts()` gives the reference's
Python objects back with ONE device->host copy.

`from_dicts` packs on the host the way `OrientationTargetGenerator._pack` does: one pinned staging
buffer per (B, K, device), K padded to a multiple of 64 so that the shapes stay stable from batch
to batch, one `non_blocking` copy, no synchronisation (a staging buffer is rewritten only once the
copy out of it has completed).
"""
from typing import Dict, List, Optional

import numpy as np
import torch

_KEY_PAD = 64
_MAX_KEYS = 4096
_MAX_KEY = 65535
_WIDE_RANGE_MESSAGE = ('instance ids outside [0, 65535] are not supported '
                       '(dataset instance maps are uint16)')
_WIDE_OVERFLOW_MESSAGE = 'more than 4096 distinct instance ids in one image'

_STAGING: Dict[tuple, dict] = {}


def _padded(longest: int) -> int:
    return max(_KEY_PAD, -(-longest // _KEY_PAD) * _KEY_PAD)


def _upload(kind: str, B: int, K: int, n_words: int, dtype: torch.dtype, device: torch.device, fill):
    """`fill(numpy view of the host buffer)`, then the buffer on `device` (a fresh tensor: tables
    outlive the call).  On a GPU the host side is a pinned buffer kept per (kind, B, K, device)."""
    if device.type != 'cuda':
        host = torch.zeros((n_words,), dtype=dtype)
        fill(host.numpy())
        return host.to(device)
    key = (kind, B, K, device)
    slot = _STAGING.get(key)
    if slot is None:
        slot = _STAGING[key] = {'host': torch.empty((n_words,), dtype=dtype).pin_memory(),
                                'done': torch.cuda.Event()}
    else:
        slot['done'].synchronize()              # the previous copy out of this buffer has landed
    packed = slot['host'].numpy()
    packed[:] = 0
    fill(packed)
    out = torch.empty((n_words,), dtype=dtype, device=device)
    out.copy_(slot['host'], non_blocking=True)
    slot['done'].record(torch.cuda.current_stream(device))
    return out


class OrientationTable:
    """per image {integer key: angle}: `keys` i32 [B,K] ascending within the first `n[b]` columns
    (None: dense, key = column index), `angle` f32 [B,K], `valid` u8 [B,K] (0: no entry), `n` i32
    [B] (None for a dense table: every column is looked at), `status`: None or the i32 [1] status
    word of the kernel that ranked the ids (bit 1: more than 4096 ids, bit 32: id out of range)."""

    def __init__(self, keys: Optional[torch.Tensor], angle: torch.Tensor, valid: torch.Tensor,
                 n: Optional[torch.Tensor], status: Optional[torch.Tensor] = None) -> None:
        assert angle.ndim == 2 and valid.shape == angle.shape
        assert angle.dtype == torch.float32 and valid.dtype == torch.uint8
        assert keys is None or (keys.shape == angle.shape and keys.dtype == torch.int32 and n is not None)
        assert n is None or (n.dtype == torch.int32 and n.shape == angle.shape[:1])
        self.keys, self.angle, self.valid, self.n, self.status = keys, angle, valid, n, status

    @property
    def batch_size(self) -> int:
        return self.angle.shape[0]

    @property
    def device(self) -> torch.device:
        return self.angle.device

    def __len__(self) -> int:
        return self.batch_size

    @classmethod
    def from_dicts(cls, dicts: List[Dict[int, float]], device) -> 'OrientationTable':
        device = torch.device(device)
        B = len(dicts)
        rows = []
        for d in dicts:
            by_int = {int(k): k for k in d}             # (a dict may be keyed by numpy integers)
            ids = sorted(by_int)
            if ids and (ids[0] < 0 or ids[-1] > _MAX_KEY):
                raise ValueError(f'orientation keys must lie in [0, {_MAX_KEY}]')
            if len(ids) > _MAX_KEYS:
                raise ValueError(f'more than {_MAX_KEYS} orientations in one image')
            # double -> float32 as `torch.tensor(python_float)` rounds it
            rows.append((ids, np.asarray([d[by_int[i]] for i in ids], dtype=np.float64).astype(np.float32)))
        K = _padded(max((len(i) for i, _ in rows), default=0))
        BK = B * K

        def fill(packed):                    # keys | angle bits | valid bytes | n
            keys = packed[:BK].reshape(B, K)
            angle = packed[BK:2 * BK].view(np.float32).reshape(B, K)
            valid = packed[2 * BK:2 * BK + BK // 4].view(np.uint8).reshape(B, K)
            n = packed[2 * BK + BK // 4:]
            for b, (ids, angles) in enumerate(rows):
                keys[b, :len(ids)] = ids
                angle[b, :len(ids)] = angles
                valid[b, :len(ids)] = 1
                n[b] = len(ids)
        buf = _upload('orientation', B, K, 2 * BK + BK // 4 + B, torch.int32, device, fill)
        return cls(buf[:BK].view(B, K), buf[BK:2 * BK].view(torch.float32).view(B, K),
                   buf[2 * BK:2 * BK + BK // 4].view(torch.uint8).view(B, K), buf[2 * BK + BK // 4:])

    def to_dicts(self) -> List[Dict[int, float]]:
        """the very list `_get_instance_orientation` returns: ascending keys, Python floats that
        hold the float32 angles; ONE device->host copy"""
        B, K = self.angle.shape
        parts = [self.angle.reshape(-1).view(torch.uint8), self.valid.reshape(-1)]
        if self.keys is not None:
            parts += [self.keys.reshape(-1).view(torch.uint8), self.n.view(torch.uint8)]
        if self.status is not None:
            parts.append(self.status.reshape(-1)[:1].view(torch.uint8))
        host = torch.cat(parts).cpu().numpy()
        BK = B * K
        angle = host[:4 * BK].view(np.float32).reshape(B, K).astype(np.float64)
        valid = host[4 * BK:5 * BK].reshape(B, K) != 0
        at = 5 * BK
        keys = n = None
        if self.keys is not None:
            keys = host[at:at + 4 * BK].view(np.int32).reshape(B, K)
            n = host[at + 4 * BK:at + 4 * BK + 4 * B].view(np.int32)
            at += 4 * BK + 4 * B
        if self.status is not None:
            status = int(host[at:at + 4].view(np.int32)[0])
            if status & 32:
                raise NotImplementedError(_WIDE_RANGE_MESSAGE)
            if status & 1:
                raise NotImplementedError(_WIDE_OVERFLOW_MESSAGE)
        out = []
        for b in range(B):
            if keys is None:
                cols = np.nonzero(valid[b])[0]
                out.append(dict(zip(cols.tolist(), angle[b, cols].tolist())))
            else:
                cols = np.nonzero(valid[b, :max(0, min(int(n[b]), K))])[0]
                out.append(dict(zip(keys[b, cols].tolist(), angle[b, cols].tolist())))
        return out


class IdTable:
    """per image {panoptic id: instance id}: `pan` i64 [B,K], `ins` i64 [B,K], `n` i32 [B].
    `ascending`: the first n[b] entries of every `pan` row ascend (lookups are binary searches);
    the tables of the merge kernels are in the id dict's insertion order (ascending INSTANCE id)
    and are walked instead."""

    def __init__(self, pan: torch.Tensor, ins: torch.Tensor, n: torch.Tensor,
                 ascending: bool = False) -> None:
        assert pan.ndim == 2 and ins.shape == pan.shape and n.shape == pan.shape[:1]
        assert pan.dtype == torch.int64 and ins.dtype == torch.int64 and n.dtype == torch.int32
        self.pan, self.ins, self.n, self.ascending = pan, ins, n, bool(ascending)

    @property
    def batch_size(self) -> int:
        return self.pan.shape[0]

    @property
    def device(self) -> torch.device:
        return self.pan.device

    def __len__(self) -> int:
        return self.batch_size

    @classmethod
    def from_dicts(cls, dicts: List[Dict[int, int]], device) -> 'IdTable':
        """rows sorted by panoptic id (`to_dicts()` then lists them in that order)"""
        device = torch.device(device)
        B = len(dicts)
        rows = [sorted((int(p), int(i)) for p, i in d.items()) for d in dicts]
        K = _padded(max((len(r) for r in rows), default=0))
        BK = B * K

        def fill(packed):                    # pan | ins | n (int32 pairs in the trailing words)
            pan = packed[:BK].reshape(B, K)
            ins = packed[BK:2 * BK].reshape(B, K)
            n = packed[2 * BK:].view(np.int32)
            for b, r in enumerate(rows):
                if r:
                    pan[b, :len(r)], ins[b, :len(r)] = np.asarray(r, dtype=np.int64).T
                n[b] = len(r)
        buf = _upload('ids', B, K, 2 * BK + (B + 1) // 2, torch.int64, device, fill)
        return cls(buf[:BK].view(B, K), buf[BK:2 * BK].view(B, K), buf[2 * BK:].view(torch.int32)[:B],
                   ascending=True)

    @classmethod
    def from_merge(cls, merged: Dict[str, torch.Tensor]) -> 'IdTable':
        """the id tables of a merge (`ids_pan` / `ids_ins` / `n_ids` of ops.panoptic_merge,
        ops.panoptic_merge_wide, ops.panoptic_pipeline), wrapped without a copy"""
        return cls(merged['ids_pan'], merged['ids_ins'], merged['n_ids'], ascending=False)

    def to_dicts(self) -> List[Dict[int, int]]:
        B, K = self.pan.shape
        host = torch.cat([self.pan.reshape(-1), self.ins.reshape(-1),
                          self.n.to(torch.int64)]).cpu().numpy()
        pan, ins, n = host[:B * K].reshape(B, K), host[B * K:2 * B * K].reshape(B, K), host[2 * B * K:]
        out = []
        for b in range(B):
            k = max(0, min(int(n[b]), K))
            out.append(dict(zip(pan[b, :k].tolist(), ins[b, :k].tolist())))
        return out
