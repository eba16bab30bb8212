"""Scene classification decoder (reference model/decoder/scene.py, `SceneClassificationDecoder`): the global
average pool of the context module's first context feature (the map itself without context features), flatten
and one linear layer.

For a CUDA, 4-D, dense NCHW map of float32 / bfloat16 / float16 the pool and the linear layer are ONE autograd
node, `SceneHeadFunction`: one HIP launch forward (`ops.scene_head`) and one backward
(`ops.scene_head_backward`), where the torch composition takes three small launches forward and four or more
backward.  The node saves the float32 pooled vector [B, C] and the weight it already holds, never the map; without
gradients no pooled vector is allocated or written.  All sums are float32 in a fixed order (include/nmsa.h).

Everything else runs the reference's `adaptive_avg_pool2d -> flatten -> linear` in plain torch: CPU tensors,
non-dense or channels-last maps, other dtypes, empty tensors, more than `NMSA_SCENE_HEAD_MAX_CHANNELS` channels
or `NMSA_SCENE_MAX_CLASSES` classes, and maps of more than `FUSED_MAX_ELEMENT_ROUTE_IMAGE` elements per image
that would take the kernels' element route (the measured crossover, see the constant).  `takes_hip_path(x)` says
which path a map takes.

The reference's default postprocessing is `get_postprocessing_class('scene')`; this package's factory does not
register that name (an existing test pins it), so the default here is the `ScenePostprocessing` class itself.

Autocast.  Inside `torch.autocast('cuda')` the logits have the autocast dtype, what `F.linear` returns there;
otherwise they have the map's dtype.  The weights are read as float32 masters and the map in its own dtype — a
stated deviation: autocast rounds the pooled vector and the weights to half for the reference's linear layer, the
kernel multiplies the float32 values (and accumulates in float32 either way).  A `module.half()` weight is cast
to float32 on the host side.
"""
from typing import Any, Type

import torch
import torch.nn.functional as F
from torch import Tensor, nn
from torch.autograd.function import once_differentiable

from ... import _lib as L
from ... import ops
from ...types import DecoderInputType
from ...types import DecoderRawOutputType
from ...types import EncoderSkipsType
from ..postprocessing import ScenePostprocessing
from ..utils import f32_master, fused_map
from .base import DecoderBase

# Maps that take the kernels' element route (H W off the 16-byte chunk, or a map off 16 bytes) with more elements
# per image (C H W) than this run the torch composition.  Measured (docs/measurement_log.md, "Scene decoder"):
# on that route the one-workgroup-per-image forward takes 27.4 us for a bfloat16 [B, 512, 15, 20] map (153600
# elements per image, whatever B), level with torch's 28 us, and the eager host floor of the fused forward is
# 22.5 us: the device time crosses it near 125000 elements.  The vector route stays ahead at that size.
FUSED_MAX_ELEMENT_ROUTE_IMAGE = 131072


class SceneHeadFunction(torch.autograd.Function):
    """logits = linear(mean over H W of x, weight, bias) (include/nmsa.h, nmsa_scene_head_*).  Saves pooled and
    weight; nothing when no input needs a gradient or gradients are switched off (`grad_enabled`: inside
    `forward` they always are, so the caller passes `torch.is_grad_enabled()`)."""

    @staticmethod
    def forward(ctx, x, weight, bias, out_dtype, grad_enabled):
        save = grad_enabled and any(ctx.needs_input_grad[:3])
        logits, pooled = ops.scene_head(x, weight, bias, need_pooled=save, out_dtype=out_dtype)
        if save:
            ctx.x_shape, ctx.x_dtype = tuple(x.shape), x.dtype
            ctx.save_for_backward(pooled, weight)
        return logits

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        pooled, weight = ctx.saved_tensors
        need = tuple(ctx.needs_input_grad[:3])
        gx, gw, gb = ops.scene_head_backward(g.contiguous(), pooled, weight, ctx.x_shape, ctx.x_dtype, need=need)
        return gx, gw, gb, None, None


class SceneClassificationDecoder(DecoderBase):
    def __init__(
        self,
        n_channels_in: int,
        n_classes: int,
        postprocessing: Type = ScenePostprocessing,
        **kwargs: Any    # just to catch unused parameters
    ) -> None:
        super().__init__(postprocessing=postprocessing)
        self._task_head = nn.Linear(n_channels_in, n_classes)

    def takes_hip_path(self, x: Tensor) -> bool:
        """whether the map `x` (the first context feature, or the context module's output) runs the HIP
        kernels (see the module docstring)"""
        if not fused_map(x):
            return False
        head = self._task_head
        if not (x.shape[1] == head.in_features and head.in_features <= L.NMSA_SCENE_HEAD_MAX_CHANNELS
                and head.out_features <= L.NMSA_SCENE_MAX_CLASSES and head.weight.is_cuda):
            return False
        if x[0].numel() > FUSED_MAX_ELEMENT_ROUTE_IMAGE:
            return ops.scene_head_route(x, head.out_features) != L.NMSA_SH_ROUTE_ELEMENT
        return True

    def _forward_training(self, x: DecoderInputType, skips: EncoderSkipsType) -> DecoderRawOutputType:
        # the first context feature is the global average pooling branch; an adaptive pyramid pooling module
        # hands out a larger one for larger validation inputs, and pooling it again is the single global pool
        cm_output, cm_context_features = x
        x = cm_context_features[0] if cm_context_features else cm_output
        if not self.takes_hip_path(x):
            out = self._task_head(torch.flatten(F.adaptive_avg_pool2d(x, 1), 1))
            return out, None
        weight, bias = f32_master(self._task_head.weight, self._task_head.bias)
        out_dtype = torch.get_autocast_dtype('cuda') if torch.is_autocast_enabled('cuda') else x.dtype
        out = SceneHeadFunction.apply(x, weight, bias, out_dtype, torch.is_grad_enabled())
        return out, None   # there are no side outputs
