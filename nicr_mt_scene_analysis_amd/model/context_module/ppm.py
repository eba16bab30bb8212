"""Pyramid pooling module (reference model/context_module/ppm.py) on the HIP kernels of
csrc/context_module.hip.

forward(x) -> (out, tuple(features_context)), as in the reference:
    pooled_i = adaptive_avg_pool2d(x, bin_i)            all bins in ONE launch (`ops.ppm_pool`)
    y_i      = features[i][1](pooled_i)                 1x1 ConvNormAct, plain torch
    cat      = cat([x] + [interpolate(y_i, (h, w))], 1) ONE launch (`ops.ppm_upsample_concat`)
    out      = final_conv(cat)                          1x1 ConvNormAct, plain torch
Backward is one launch per step (`ops.ppm_upsample_concat_backward`, `ops.ppm_pool_backward`)
behind `UpsampleConcatFunction` and `PyramidPoolFunction`; both save shapes only, and the gradient
of x through the concatenation is a view of the upstream gradient.

State dict: the reference's keys and shapes (`features.<i>.1.conv.weight`, `features.<i>.1.norm.*`,
`final_conv.*`); index 0 of each branch stays the parameter-free `nn.AdaptiveAvgPool2d(bin)`, which
is never called.

Dtypes: the concatenation has torch's promoted dtype of x and the branch outputs.  Where they differ
(float32 x under autocast with half branch outputs, or the other way round) the smaller side is cast
with torch before the kernel: negligible for the branch maps (at most ph * pw pixels each), a FULL
PASS over x when x is the smaller side.

Stated deviations: there is no eager fallback (a CPU tensor raises `NmsaError`), and a channels-last x
is made contiguous (the concatenation is NCHW-contiguous).  More than four bins raise `ValueError`.
"""
from typing import Any, Sequence, Tuple, Type

import torch
import torch.nn as nn

from ... import ops
from ...types import ContextModuleInputType
from ...types import ContextModuleOutputType
from ..activation import get_activation_class
from ..normalization import get_normalization_class
from ..utils import ConvNormAct

KNOWN_CONTEXT_UPSAMPLINGS = ('nearest', 'bilinear')


class PyramidPoolFunction(torch.autograd.Function):
    """pooled_0, ... = ops.ppm_pool(x, sizes); saves x's shape only"""

    @staticmethod
    def forward(ctx, x, sizes):
        ctx.x_shape, ctx.sizes = tuple(x.shape), sizes
        return ops.ppm_pool(x, sizes)

    @staticmethod
    def backward(ctx, *gps):
        if not ctx.needs_input_grad[0] or all(g is None for g in gps):
            return None, None
        return ops.ppm_pool_backward(gps, ctx.x_shape, ctx.sizes), None


class UpsampleConcatFunction(torch.autograd.Function):
    """cat = ops.ppm_upsample_concat(x, ys, mode); saves shapes only.  The gradient of x is the view
    g[:, :C] of the upstream gradient; the branch gradients are asked from the kernel only where
    `needs_input_grad` names them."""

    @staticmethod
    def forward(ctx, mode, x, *ys):
        ctx.mode, ctx.n_channels_x = mode, int(x.shape[1])
        ctx.branch_shapes = tuple(tuple(y.shape) for y in ys)
        return ops.ppm_upsample_concat(x, ys, mode)

    @staticmethod
    def backward(ctx, g):
        need_x, need = ctx.needs_input_grad[1], ctx.needs_input_grad[2:]
        gys = (None,) * len(need)
        if any(need):
            gys = ops.ppm_upsample_concat_backward(g, ctx.n_channels_x, ctx.branch_shapes, ctx.mode, need)
        return (None, g[:, :ctx.n_channels_x] if need_x else None) + tuple(gys)


def pyramid_forward(module: nn.Module, x: torch.Tensor, sizes: Sequence[Tuple[int, int]]):
    """the forward pass PPM and APPM share: `sizes` are the pool sizes of this call"""
    if module._upsampling not in KNOWN_CONTEXT_UPSAMPLINGS:
        raise NotImplementedError()
    pooled = PyramidPoolFunction.apply(x, tuple(sizes))
    features_context = tuple(f[1](p) for f, p in zip(module.features, pooled))
    dtype = x.dtype
    for y in features_context:
        dtype = torch.promote_types(dtype, y.dtype)
    xc = x if x.dtype == dtype else x.to(dtype)             # a full pass over x (see the module docstring)
    ys = tuple(y if y.dtype == dtype else y.to(dtype) for y in features_context)
    out = UpsampleConcatFunction.apply(module._upsampling, xc, *ys)
    return module.final_conv(out), features_context


class PyramidPoolingModule(nn.Module):
    def __init__(
        self,
        n_channels_in: int,
        n_channels_out: int,
        bins: Tuple[int, ...] = (1, 2, 3, 6),
        normalization: Type[nn.Module] = get_normalization_class(),
        activation: Type[nn.Module] = get_activation_class(),
        upsampling: str = 'bilinear',
        **kwargs: Any
    ) -> None:
        super().__init__()
        ops._ppm_sizes(bins)                                # 1..4 bins, each at least 1
        n_channels_reduction = n_channels_in // len(bins)
        self._upsampling = upsampling
        self._bins = tuple(bins)

        features = []
        for bin in bins:
            features.append(nn.Sequential(
                nn.AdaptiveAvgPool2d(bin),                  # parameter-free, never called: the kernel pools
                ConvNormAct(n_channels_in, n_channels_reduction, kernel_size=1,
                            normalization=normalization, activation=activation)
            ))
        self.features = nn.ModuleList(features)

        n_channels_in_last_conv = n_channels_in + n_channels_reduction * len(bins)
        self.final_conv = ConvNormAct(n_channels_in_last_conv, n_channels_out, kernel_size=1,
                                      normalization=normalization, activation=activation)
        self.n_channels_reduction = n_channels_reduction

    def forward(self, x: ContextModuleInputType) -> ContextModuleOutputType:
        return pyramid_forward(self, x, ops._ppm_sizes(self._bins))
