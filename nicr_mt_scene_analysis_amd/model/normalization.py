"""Normalization classes by name (reference model/normalization.py): plain torch."""
from typing import Any, Optional, Type

from torch import nn

from ..utils import partial_class

KNOWN_NORMALIZATIONS = ('bn', 'batchnorm', 'ln', 'layernorm')


def get_normalization_class(name: Optional[str] = None, **kwargs: Any) -> Type[nn.Module]:
    name = (name or 'bn').lower()           # the reference's global default: batch normalization
    if name not in KNOWN_NORMALIZATIONS:
        raise ValueError(f"Unknown normalization: '{name}'")
    return partial_class(nn.BatchNorm2d if name in ('bn', 'batchnorm') else nn.LayerNorm, **kwargs)
