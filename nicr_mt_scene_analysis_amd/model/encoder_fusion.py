"""Fusion of the RGB and the depth encoder after every encoder stage (reference model/encoder_fusion.py).

`get_encoder_fusion_class(name)` with the reference's seven names and its default 'add-uni-rgb':
  'add', 'add-uni-rgb', 'add-uni-depth'   `torch.add`; the library is not touched
  'se-add', 'se-add-uni-rgb', 'se-add-uni-depth'   each modality weighted by a `SqueezeAndExcitation`
                                (`weighting_rgb`, `weighting_depth`), then added
  'none'                        both inputs are handed through
`forward(x)` takes and returns {'rgb': ..., 'depth': ...}.  A key that is not a destination holds the
input tensor itself; with both destinations both keys hold the SAME fused tensor, as in the reference.

The SE-weighted add on the device.  x_rgb and x_depth CUDA, 4-D, dense NCHW, one shape, one dtype of
float32 / bfloat16 / float16, layout 'nchw', activation `nn.ReLU` or `nn.SiLU`: three HIP launches
forward (`ops.sefuse_squeeze`, `ops.sefuse_excite`, `ops.sefuse_scale_add`) and three backward
(`ops.sefuse_weight_grad`, `ops.sefuse_excite_backward`, `ops.sefuse_apply_backward`) behind ONE
autograd node, `SEWeightedAddFunction`; no intermediate map is written.  The parameter gradients are
small torch matmuls inside `backward`.  `module.half()`: the parameters are cast to float32 for the
kernels.  Inside `torch.autocast('cuda')` the fused path is taken when the torch composition would
return the inputs' dtype (float32 inputs, or half inputs of the autocast dtype); the squeeze-and-
excitation is then computed in float32 from the inputs, not in the autocast dtype.
Everything else runs the reference's own composition in torch through the `SqueezeAndExcitation`
modules: CPU tensors, 'nhwc' (the Swin encoders; permute, apply, permute back), mixed dtypes or shapes,
other activation modules, non-dense inputs, a half input whose autocast result would be float32.
No case is left on torch for speed: every ResNet34 stage shape measured faster than the torch
composition.
"""
from typing import Any, Callable, Optional, Tuple, Type

import torch
from torch import Tensor, nn

from .. import ops
from ..types import EncoderForwardType
from ..utils import partial_class
from .activation import get_activation_class
from .utils import SqueezeAndExcitation, f32_master, fused_map

KNOWN_ENCODER_FUSIONS = (
    'se-add', 'add',                        # both directions (the same tensor under both keys)
    'add-uni-rgb', 'add-uni-depth',         # one direction
    'se-add-uni-rgb', 'se-add-uni-depth',   # one direction, SE-weighted
    'none',                                 # no fusion
)


def _apply_NCHW_operation(x: Tensor, operation: Callable[[Tensor], Tensor], input_memory_layout: str) -> Tensor:
    if input_memory_layout == 'nchw':
        return operation(x)
    if input_memory_layout == 'nhwc':
        return operation(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    raise ValueError(f'Unknown input_memory_layout: {input_memory_layout}')


def _se_parameters(se: SqueezeAndExcitation) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(W1, b1, W2, b2) of a SqueezeAndExcitation as float32 (a cast copy after module.half())"""
    return f32_master(se.layers[0].weight, se.layers[0].bias, se.layers[2].weight, se.layers[2].bias)


class SEWeightedAddFunction(torch.autograd.Function):
    """y = x_rgb * w_rgb + x_depth * w_depth with w_m = sigmoid(W2_m act(W1_m mean(x_m) + b1_m) + b2_m):
    ONE node over the squeeze, the excitation and the weighted add, so that the gradient of a map,
    gy * w_m + gs_m / (H*W), is one pass and no map-sized intermediate exists.  Saves the two maps
    (each only when its modality needs a gradient), the per-(modality, image, channel) vectors s, z1, w
    and the two weight matrices per modality; nothing when no input needs a gradient or gradients are
    switched off (`grad_enabled`: inside `forward` they always are, so the caller passes
    `torch.is_grad_enabled()`, and `needs_input_grad` does not know about `torch.no_grad()`).  A modality whose
    map and parameters need no gradient is left out of all three backward kernels; the map pass is left
    out when only parameters need gradients."""

    @staticmethod
    def forward(ctx, x_rgb, x_depth, W1r, b1r, W2r, b2r, W1d, b1d, W2d, b2d, act, grad_enabled):
        need = ctx.needs_input_grad
        need_rgb = grad_enabled and (need[0] or any(need[2:6]))
        need_depth = grad_enabled and (need[1] or any(need[6:10]))
        s = ops.sefuse_squeeze(x_rgb, x_depth)
        ctx.act = act
        if need_rgb or need_depth:
            w, z1 = ops.sefuse_excite(s, (W1r, b1r, W2r, b2r), (W1d, b1d, W2d, b2d), act, save_z1=True)
            ctx.save_for_backward(x_rgb if need_rgb else None, x_depth if need_depth else None, s, z1, w,
                                  W1r if need_rgb else None, W2r if need_rgb else None,
                                  W1d if need_depth else None, W2d if need_depth else None)
        else:
            w = ops.sefuse_excite(s, (W1r, b1r, W2r, b2r), (W1d, b1d, W2d, b2d), act)
        return ops.sefuse_scale_add(x_rgb, x_depth, w)

    @staticmethod
    def backward(ctx, gy):
        need = ctx.needs_input_grad
        x_rgb, x_depth, s, z1, w, W1r, W2r, W1d, W2d = ctx.saved_tensors
        gw = ops.sefuse_weight_grad(gy, x_rgb, x_depth)
        gz2, gz1, gs, h = ops.sefuse_excite_backward(
            gw, w, z1, None if W1r is None else (W1r, W2r), None if W1d is None else (W1d, W2d), ctx.act)
        gx_rgb, gx_depth = ops.sefuse_apply_backward(gy, w, gs, need[0], need[1])
        grads = [gx_rgb, gx_depth]
        with torch.autocast('cuda', enabled=False):
            for m, W1 in enumerate((W1r, W1d)):
                nW1, nb1, nW2, nb2 = need[2 + 4 * m:6 + 4 * m]
                grads.append((gz1[m].t() @ s[m]).reshape(W1.shape) if nW1 else None)              # [R, C, 1, 1]
                grads.append(gz1[m].sum(0) if nb1 else None)
                grads.append((gz2[m].t() @ h[m]).reshape(W1.shape[1], W1.shape[0], 1, 1) if nW2 else None)
                grads.append(gz2[m].sum(0) if nb2 else None)
        return (*grads, None, None)


class EncoderRGBDFusionWeightedAdd(nn.Module):
    def __init__(self, n_channels_in: int, destinations: Tuple[str, ...], use_se_weighting: bool,
                 input_memory_layout: str, activation: Type[nn.Module] = get_activation_class(),
                 **kwargs: Any) -> None:
        super().__init__()
        if use_se_weighting:
            self.weighting_rgb = SqueezeAndExcitation(n_channels_in, activation=activation)
            self.weighting_depth = SqueezeAndExcitation(n_channels_in, activation=activation)
        self._n_channels_in = n_channels_in
        self._use_se_weighting = use_se_weighting
        self._destinations = destinations
        self._input_memory_layout = input_memory_layout

    def _fused_act(self, x_rgb: Tensor, x_depth: Tensor) -> Optional[str]:
        """the activation code of the fused HIP path, None when this call takes the torch composition"""
        if self._input_memory_layout != 'nchw':
            return None
        if not (fused_map(x_rgb) and x_depth.is_cuda and x_rgb.device == x_depth.device
                and x_rgb.shape == x_depth.shape and x_rgb.dtype == x_depth.dtype and x_depth.is_contiguous()):
            return None
        if torch.is_autocast_enabled('cuda') and \
                torch.promote_types(x_rgb.dtype, torch.get_autocast_dtype('cuda')) != x_rgb.dtype:
            return None
        acts = (self.weighting_rgb.layers[1], self.weighting_depth.layers[1])
        for cls, code in ((nn.ReLU, 'relu'), (nn.SiLU, 'silu')):
            if all(isinstance(a, cls) for a in acts):
                return code
        return None

    def forward(self, x: EncoderForwardType) -> EncoderForwardType:
        x_rgb, x_depth = x['rgb'], x['depth']
        if not self._destinations:
            return {'rgb': x_rgb, 'depth': x_depth}         # nothing is computed for 'none'
        if not self._use_se_weighting:
            fused = x_rgb + x_depth
        else:
            act = self._fused_act(x_rgb, x_depth)
            if act is not None:
                fused = SEWeightedAddFunction.apply(x_rgb, x_depth, *_se_parameters(self.weighting_rgb),
                                                    *_se_parameters(self.weighting_depth), act,
                                                    torch.is_grad_enabled())
            else:
                fused = (_apply_NCHW_operation(x_rgb, self.weighting_rgb, self._input_memory_layout)
                         + _apply_NCHW_operation(x_depth, self.weighting_depth, self._input_memory_layout))
        return {'rgb': fused if 'rgb' in self._destinations else x_rgb,
                'depth': fused if 'depth' in self._destinations else x_depth}


EncoderFusionType = EncoderRGBDFusionWeightedAdd


def get_encoder_fusion_class(name: Optional[str] = None, **kwargs: Any) -> Type[EncoderFusionType]:
    if name is None:
        name = 'add-uni-rgb'                # the reference's global default
    name = name.lower()
    if name not in KNOWN_ENCODER_FUSIONS:
        raise ValueError(f"Unknown encoder fusion: '{name}'")
    kwargs['use_se_weighting'] = 'se' in name
    if 'uni-rgb' in name:
        kwargs['destinations'] = ('rgb',)
    elif 'uni-depth' in name:
        kwargs['destinations'] = ('depth',)
    elif name == 'none':
        kwargs['destinations'] = ()
    else:
        kwargs['destinations'] = ('rgb', 'depth')
    return partial_class(EncoderRGBDFusionWeightedAdd, **kwargs)
