"""Numpy restatement of what `nmsa_batch_augment_resized` computes FROM ITS TABLES: the window tables
of `ops.augment_window_tables` evaluated key by key on the host.  The CPU tests compare it with the
fixture of tools/gen_golden_augment_resize.py, whose stand-in resizes the whole image from the rules
written out a second time and then crops and flips as the reference does: tables and stand-in meet
only in the result."""
from typing import Dict, Optional, Tuple

import numpy as np


def gather_nearest(src: np.ndarray, cols: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """[B,H,W] -> [B,h,w], [B,H,W,C] -> [B,C,h,w] through the nearest tables (raw elements)"""
    out = np.stack([src[b][rows[0, b][:, None], cols[0, b][None, :]] for b in range(src.shape[0])])
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2)) if src.ndim == 4 else out


def linear_u8(src: np.ndarray, cols: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """u8 [B,H,W,C] -> i64 [B,C,h,w], values 0..255: the two fixed-point passes over the packed taps"""
    out = []
    for b in range(src.shape[0]):
        image = src[b].astype(np.int64)
        taps, wts = cols[1, b].view(np.uint32).astype(np.int64), cols[2, b].view(np.uint32).astype(np.int64)
        i0, i1, a0, a1 = taps & 0xffff, taps >> 16, (wts & 0xffff)[None, :, None], (wts >> 16)[None, :, None]
        taps, wts = rows[1, b].view(np.uint32).astype(np.int64), rows[2, b].view(np.uint32).astype(np.int64)
        j0, j1, b0, b1 = taps & 0xffff, taps >> 16, (wts & 0xffff)[:, None, None], (wts >> 16)[:, None, None]
        R0 = image[j0][:, i0] * a0 + image[j0][:, i1] * a1
        R1 = image[j1][:, i0] * a0 + image[j1][:, i1] * a1
        out.append((((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16) + 2) >> 2)
    return np.stack(out).transpose(0, 3, 1, 2)


def normalise_rgb(v: np.ndarray, mean, std) -> np.ndarray:
    """[B,3,h,w] values 0..255 -> f32: one float32 subtract, one float32 divide"""
    mean, std = (np.asarray(a, np.float32).reshape(1, 3, 1, 1) for a in (mean, std))
    return (v.astype(np.float32) - mean) / std


def normalise_depth(v: np.ndarray, mean: float, std: float, raw_depth: bool, invalid: float) -> np.ndarray:
    """[B,h,w] u16 / f32 -> f32 [B,1,h,w], invalid values kept with `raw_depth`"""
    f = v.astype(np.float32)
    with np.errstate(invalid='ignore'):
        out = (f - np.float32(mean)) / np.float32(std)
    if raw_depth:
        out = np.where(f == np.float32(invalid), np.float32(invalid), out)
    return out[:, None]


def evaluate(inputs: Dict[str, np.ndarray], tables: Tuple[np.ndarray, np.ndarray], rgb_norm: Tuple,
             depth_norm: Optional[Tuple]) -> Dict[str, np.ndarray]:
    """every array of `inputs` through `tables` = (cols, rows): `rgb` linear then normalised with
    rgb_norm = (mean[3], std[3]), `depth` nearest then normalised with depth_norm = (mean, std,
    raw_depth, invalid), everything else nearest as raw elements"""
    cols, rows = tables
    out = {}
    for key, value in inputs.items():
        if key == 'rgb':
            out[key] = normalise_rgb(linear_u8(value, cols, rows), *rgb_norm)
        elif key == 'depth' and depth_norm is not None:
            out[key] = normalise_depth(gather_nearest(value, cols, rows), *depth_norm)
        else:
            out[key] = gather_nearest(value, cols, rows)
    return out
