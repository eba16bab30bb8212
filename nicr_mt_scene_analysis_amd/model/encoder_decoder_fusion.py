"""Fusion of encoder skip features into the decoders (reference model/encoder_decoder_fusion.py).

`get_encoder_decoder_fusion_class(name)` with the reference's 19 names and its default 'add-rgb':
  'add*', 'select*'             `EncoderDecoderFusion`: NCHW encoder features, added to / taken
                                instead of the decoder features; plain torch, the library is not touched
  'swin-add*', 'swin-select*'   `EncoderDecoderFusionSwin` without LayerNorm: NHWC -> NCHW as a
                                permuted view, then the same; plain torch
  'swin-ln-add*', 'swin-ln-select*'   LayerNorm over C, NHWC -> NCHW and (where it can be fused) the
                                addition in ONE HIP launch (`ops.ln_nhwc_to_nchw`), one pass plus a
                                small reduction backward (`ops.ln_nhwc_to_nchw_backward`) behind
                                `SwinFusionFunction`; no eager fallback, a CPU tensor raises `NmsaError`
  'none'                        returns the decoder features
`*-rgb` / `*-depth` pick that key of the encoder's skip dict; without a suffix the only key of the
first dict seen is taken.

Parameters.  `ln` is an `nn.LayerNorm(n_channels_encoder)` that only holds `weight`, `bias` and `eps`
(it is never called), `layer` is `nn.Identity()` or, for unequal channel counts, a `ConvNormAct`: the
state dict has the reference's keys and shapes and a reference checkpoint loads.

What the kernel covers.  Equal channel counts: 'select' is the kernel alone; 'add' has the addition
fused when `x_dec` has the output's shape and dtype (its gradient is then the upstream gradient
itself, the same tensor), otherwise `torch.add` follows (the reference's type promotion).  Unequal
channel counts: the kernel, then `layer`, then the fuse operation, both in torch.
Output dtype: the input's; inside `torch.autocast('cuda')` float32 (what autocast's `layer_norm`
returns), computed straight from the half input.  `module.half()`: the parameters are cast to
float32 for the kernel.
Stated deviation: the result is NCHW-contiguous where the reference returns a permuted view of the
NHWC result; the values are the same.
"""
from typing import Any, Callable, Dict, Optional, Type, Union

import torch
from torch import Tensor, nn

from .. import ops
from ..utils import partial_class
from .activation import get_activation_class
from .normalization import get_normalization_class
from .utils import ConvNormAct, f32_master

KNOWN_ENCODER_DECODER_FUSIONS = (
    'add', 'add-rgb', 'add-depth',
    'select', 'select-rgb', 'select-depth',
    'swin-ln-add', 'swin-ln-add-rgb', 'swin-ln-add-depth',
    'swin-ln-select', 'swin-ln-select-rgb', 'swin-ln-select-depth',
    'swin-add', 'swin-add-rgb', 'swin-add-depth',
    'swin-select', 'swin-select-rgb', 'swin-select-depth',
    'none',
)

EncoderSkipType = Dict[str, Tensor]


def _select(x_enc: Tensor, x_dec: Optional[Tensor]) -> Tensor:
    return x_enc


class SwinFusionFunction(torch.autograd.Function):
    """y = ln_nhwc_to_nchw(x, gamma, beta, eps, add) in `out_dtype`; saves x, gamma and the row
    statistics only when x, gamma or beta needs a gradient, asks the backward kernel only for those,
    and hands the upstream gradient itself on as the gradient of `add`"""

    @staticmethod
    def forward(ctx, x, gamma, beta, add, eps, out_dtype):
        if any(ctx.needs_input_grad[:3]):
            y, mean, rstd = ops.ln_nhwc_to_nchw(x, gamma, beta, eps, add=add, out_dtype=out_dtype, save_stats=True)
            ctx.save_for_backward(x, gamma, mean, rstd)
            return y
        return ops.ln_nhwc_to_nchw(x, gamma, beta, eps, add=add, out_dtype=out_dtype)

    @staticmethod
    def backward(ctx, gy):
        need_gx, need_gg, need_gb, need_add = ctx.needs_input_grad[:4]
        gx = gg = gb = None
        if need_gx or need_gg or need_gb:
            x, gamma, mean, rstd = ctx.saved_tensors
            gx, gg, gb = ops.ln_nhwc_to_nchw_backward(gy, x, gamma, mean, rstd, need_gx, need_gg, need_gb)
        return gx, gg, gb, (gy if need_add else None), None, None


class EncoderDecoderFusion(nn.Module):
    def __init__(self, n_channels_encoder: int, n_channels_decoder: int, fuse_features_from: Optional[str],
                 fuse_operation: Optional[Callable[[Tensor, Tensor], Tensor]] = torch.add,
                 normalization: Type[nn.Module] = get_normalization_class(),
                 activation: Type[nn.Module] = get_activation_class()) -> None:
        super().__init__()
        if fuse_operation is not None:
            # a 1x1 ConvNormAct adapts the channel count; equal counts add no parameters
            self.layer = (nn.Identity() if n_channels_encoder == n_channels_decoder else
                          ConvNormAct(n_channels_encoder, n_channels_decoder, normalization=normalization,
                                      activation=activation))
        self._fuse_features_from = fuse_features_from
        self._fuse_operation = fuse_operation

    def _encoder_features(self, x_enc: EncoderSkipType) -> Tensor:
        if self._fuse_features_from is None:
            # the key was not known at construction: a single-modality encoder has exactly one
            if len(x_enc) != 1:
                raise AssertionError(f'cannot pick the encoder features: keys {list(x_enc)}')
            self._fuse_features_from = next(iter(x_enc))
        return x_enc[self._fuse_features_from]

    def forward(self, x_enc: EncoderSkipType, x_dec: Optional[Tensor]) -> Tensor:
        if self._fuse_operation is None:
            return x_dec
        return self._fuse_operation(self.layer(self._encoder_features(x_enc)), x_dec)


class EncoderDecoderFusionSwin(EncoderDecoderFusion):
    def __init__(self, n_channels_encoder: int, n_channels_decoder: int, fuse_features_from: Optional[str],
                 fuse_operation: Callable[[Tensor, Tensor], Tensor] = torch.add, apply_layer_norm: bool = True,
                 normalization: Type[nn.Module] = get_normalization_class(),
                 activation: Type[nn.Module] = get_activation_class()) -> None:
        super().__init__(n_channels_encoder=n_channels_encoder, n_channels_decoder=n_channels_decoder,
                         fuse_features_from=fuse_features_from, fuse_operation=fuse_operation,
                         normalization=normalization, activation=activation)
        # parameter holder only (reference keys / shapes, eps); forward never calls it
        self.ln = get_normalization_class('ln')(n_channels_encoder) if apply_layer_norm else nn.Identity()
        self._apply_layer_norm = apply_layer_norm

    def forward(self, x_enc: EncoderSkipType, x_dec: Optional[Tensor]) -> Tensor:
        x = self._encoder_features(x_enc)           # NHWC
        if not self._apply_layer_norm:
            return self._fuse_operation(self.layer(torch.permute(x, (0, 3, 1, 2))), x_dec)
        gamma, beta = f32_master(self.ln.weight, self.ln.bias)
        out_dtype = torch.float32 if (x.is_cuda and torch.is_autocast_enabled('cuda')) else x.dtype
        identity = isinstance(self.layer, nn.Identity)
        add = None
        if (identity and self._fuse_operation is torch.add and x_dec is not None and x_dec.dtype == out_dtype
                and x.ndim == 4 and tuple(x_dec.shape) == (x.shape[0], x.shape[3], x.shape[1], x.shape[2])):
            add = x_dec
        y = SwinFusionFunction.apply(x, gamma, beta, add, self.ln.eps, out_dtype)
        if add is not None:
            return y
        return self._fuse_operation(self.layer(y), x_dec)


EncoderDecoderFusionType = Union[EncoderDecoderFusion, EncoderDecoderFusionSwin]


def get_encoder_decoder_fusion_class(name: Optional[str] = None, **kwargs: Any) -> Type[EncoderDecoderFusionType]:
    if name is None:
        name = 'add-rgb'                    # the reference's global default
    name = name.lower()
    if name not in KNOWN_ENCODER_DECODER_FUSIONS:
        raise ValueError(f"Unknown encoder decoder fusion: '{name}'")
    if name == 'none':
        return partial_class(EncoderDecoderFusion, fuse_features_from=None, fuse_operation=None, **kwargs)
    parts = name.split('-')
    cls = EncoderDecoderFusion
    if parts[0] == 'swin':
        cls = EncoderDecoderFusionSwin
        kwargs['apply_layer_norm'] = 'ln' in parts
    kwargs['fuse_operation'] = torch.add if 'add' in parts else _select
    kwargs['fuse_features_from'] = parts[-1] if parts[-1] in ('rgb', 'depth') else None
    return partial_class(cls, **kwargs)
