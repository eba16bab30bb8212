"""Upsampling of the dense decoder heads (reference model/upsampling.py).

`Upsampling(mode, n_channels, scale_factor=2., use_bias=True)` with the reference's four modes:
  'nearest', 'bilinear'      the reference's plain `interpolate` call; the library is not touched
  'learned-3x3'              nearest x2, replication pad, depthwise 3x3 convolution
  'learned-3x3-zeropad'      nearest x2, depthwise 3x3 convolution with zero padding
The learned modes run as ONE HIP launch forward (`ops.upsample2x_dw3x3`) and one pass backward
(`ops.upsample2x_dw3x3_backward`) behind `LearnedUpsamplingFunction`; there is no eager fallback,
a CPU tensor raises `NmsaError`.  Their parameters live in an `nn.Conv2d` attribute `conv`
(groups = channels), so `state_dict()` has the reference's keys and shapes (`conv.weight`
[C, 1, 3, 3], `conv.bias` [C]) and a reference checkpoint loads; the initial values are the
reference's (the 1/16 - 2/16 - 4/16 bilinear stencil, zero bias).  The convolution module itself is
never called.

Autocast.  Inside `torch.autocast('cuda')` a float32 input is cast to the autocast dtype first, so
the output dtype is the reference's.  The weights stay float32 — a stated deviation: autocast
rounds them to half for the reference's convolution, the kernel multiplies with the float32
parameters (and accumulates in float32 either way).
"""
from typing import Any, Optional, Tuple, Type, Union

import torch
from torch import nn
from torch.nn.functional import interpolate

from .. import ops
from ..utils import partial_class
from .utils import f32_master

KNOWN_UPSAMPLING_METHODS = ('nearest', 'bilinear', 'learned-3x3', 'learned-3x3-zeropad')

# the stencil that makes nearest x2 + 3x3 equal bilinear x2 (exact in float32)
_BILINEAR_STENCIL = ((0.0625, 0.125, 0.0625), (0.125, 0.25, 0.125), (0.0625, 0.125, 0.0625))


class LearnedUpsamplingFunction(torch.autograd.Function):
    """y = upsample2x_dw3x3(x, weight, bias, zeropad); saves x and weight, and asks the backward
    kernel only for the gradients `needs_input_grad` names"""

    @staticmethod
    def forward(ctx, x, weight, bias, zeropad):
        ctx.zeropad = bool(zeropad)
        ctx.save_for_backward(x, weight)
        return ops.upsample2x_dw3x3(x, weight, bias, ctx.zeropad)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        need_gx, need_gw, need_gb = ctx.needs_input_grad[:3]
        if not (need_gx or need_gw or need_gb):
            return None, None, None, None
        if gy.dtype != x.dtype:
            gy = gy.to(x.dtype)
        gx, gw, gb = ops.upsample2x_dw3x3_backward(gy, x, weight, ctx.zeropad, need_gx, need_gw, need_gb)
        return gx, gw, gb, None


class Upsampling(nn.Module):
    def __init__(self, mode: str, n_channels: int,
                 scale_factor: Union[float, Tuple[float, float]] = 2., use_bias: bool = True) -> None:
        super().__init__()
        if mode not in KNOWN_UPSAMPLING_METHODS:
            raise ValueError(f"Unknown upsampling: '{mode}'")
        self._learned = mode.startswith('learned-3x3')
        self._zeropad = mode == 'learned-3x3-zeropad'
        self._align_corners = False if mode == 'bilinear' else None
        if self._learned:
            if scale_factor != 2. and tuple(scale_factor if isinstance(scale_factor, (tuple, list))
                                            else (scale_factor,)) != (2., 2.):
                raise ValueError(f"mode '{mode}' upsamples by 2, got scale_factor={scale_factor}")
            # parameter holder only (reference keys / shapes); forward never calls it
            self.conv = nn.Conv2d(n_channels, n_channels, groups=n_channels, kernel_size=3,
                                  padding=1 if self._zeropad else 0, bias=use_bias)
            with torch.no_grad():
                self.conv.weight.copy_(torch.tensor(_BILINEAR_STENCIL).expand(n_channels, 1, 3, 3))
                if use_bias:
                    self.conv.bias.zero_()
            self._mode = 'nearest'
        else:
            self.conv = nn.Identity()
            self._mode = mode
        self.pad = nn.Identity()            # the reference's attribute; no parameters in any mode
        self._scale_factor = scale_factor

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not self._learned:
            return interpolate(x, scale_factor=self._scale_factor, mode=self._mode,
                               align_corners=self._align_corners)
        if x.is_cuda and x.dtype == torch.float32 and torch.is_autocast_enabled('cuda'):
            x = x.to(torch.get_autocast_dtype('cuda'))
        weight, bias = f32_master(self.conv.weight, self.conv.bias)
        return LearnedUpsamplingFunction.apply(x, weight, bias, self._zeropad)


UpsamplingType = Upsampling


def get_upsampling_class(name: Optional[str] = None, **kwargs: Any) -> Type[UpsamplingType]:
    if name is None:
        name = 'bilinear'                   # the reference's global default
    name = name.lower()
    if name not in KNOWN_UPSAMPLING_METHODS:
        raise ValueError(f"Unknown upsampling: '{name}'")
    kwargs['mode'] = name
    return partial_class(Upsampling, **kwargs)
