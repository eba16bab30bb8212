"""Activation classes by name (reference model/activation.py): plain torch."""
from typing import Any, Optional, Type

from torch import nn

from ..utils import partial_class

KNOWN_ACTIVATIONS = ('relu', 'silu', 'swish')


def get_activation_class(name: Optional[str] = None, **kwargs: Any) -> Type[nn.Module]:
    if name is None:
        name = 'relu'                       # the reference's global default: an in-place ReLU
        kwargs['inplace'] = True
    name = name.lower()
    if name not in KNOWN_ACTIVATIONS:
        raise ValueError(f"Unknown activation: '{name}'")
    return partial_class(nn.ReLU if name == 'relu' else nn.SiLU, **kwargs)
