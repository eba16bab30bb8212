"""Biternion helpers used by the hot path (reference utils/_orientation.py:39-47)."""
import numpy as np
import torch


def biternion2rad(biternion: torch.Tensor) -> torch.Tensor:
    # channel 0 = cos, channel 1 = sin
    return torch.atan2(biternion[:, 1], biternion[:, 0])


def biternion2deg(biternion: torch.Tensor) -> torch.Tensor:
    return torch.rad2deg(biternion2rad(biternion)) % 360


def np_rad2biternion(rad) -> np.ndarray:
    # (cos, sin) evaluated in float64, then rounded to float32 (reference utils/_orientation.py:20-21)
    return np.array([np.cos(rad), np.sin(rad)], dtype='float32')
