"""The context module between the encoder and the decoders (reference model/context_module/):
`get_context_module(name, ...)` with the reference's nine names.
  'ppm', 'ppm-1-5', 'ppm-1-5-10', 'ppm-1-2-4-8'        `PyramidPoolingModule`: fixed pool sizes
  'appm', 'appm-1-5', 'appm-1-5-10', 'appm-1-2-4-8'    `AdaptivePyramidPoolingModule`: pool sizes that
                                                       grow with the input (fixed window sizes)
  'none'                                               `NoContextModule`, plain torch
Pooling and upsample + concatenation of the first two run on the HIP kernels of
csrc/context_module.hip (see context_module/ppm.py)."""
from typing import Tuple, Union

from ..activation import get_activation_class
from ..normalization import get_normalization_class

from .appm import AdaptivePyramidPoolingModule
from .ppm import PyramidPoolingModule
from .none import NoContextModule


KNOWN_CONTEXT_MODULES = (
    'ppm',              # same as ppm-1-5
    'ppm-1-5',          # 640x480 inputs
    'ppm-1-5-10',       # 1280x960 inputs
    'ppm-1-2-4-8',      # 1024x512 inputs
    'appm',             # same as appm-1-5
    'appm-1-5',
    'appm-1-5-10',
    'appm-1-2-4-8',
    'none',
)

_BINS = {'1-5': (1, 5), '1-5-10': (1, 5, 10), '1-2-4-8': (1, 2, 4, 8)}

ContextModuleType = Union[PyramidPoolingModule, AdaptivePyramidPoolingModule, NoContextModule]


def get_context_module(
    name: str,
    n_channels_in: int,
    n_channels_out: int,
    input_size: Tuple[int, int],
    normalization: str = 'batchnorm',
    activation: str = 'relu',
    upsampling: str = 'bilinear'
) -> ContextModuleType:
    name = name.lower()
    if name not in KNOWN_CONTEXT_MODULES:
        raise ValueError(f"Unknown context module: '{name}'")
    if name == 'none':
        bins, context_module_class = (), NoContextModule
    else:
        kind, _, suffix = name.partition('-')
        bins = _BINS.get(suffix, (1, 5))
        context_module_class = AdaptivePyramidPoolingModule if kind == 'appm' else PyramidPoolingModule
    return context_module_class(
        n_channels_in, n_channels_out,
        bins=bins,
        input_size=input_size,
        normalization=get_normalization_class(normalization),
        activation=get_activation_class(activation),
        upsampling=upsampling
    )
