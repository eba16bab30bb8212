"""MLP decoder (reference model/decoder/mlp_base.py, after SegFormer, arXiv 2105.15203) with its hot
step on the HIP kernels of csrc/mlp_decoder.hip.

_forward_training((x, context_features), skips) -> (output, ()), as in the reference:
    e_0 = main_branch.embedding(x)                              1x1 convolution, plain torch
    e_i = skip_branches[i].embedding(skip_fusions[i](skip_i))   the fusion (LayerNorm + NHWC -> NCHW on
                                                                HIP for 'swin-ln-*'), 1x1 convolution
    cat = cat([upsample_i(e_i)], 1)                             ONE launch (`ops.mlpdec_upsample_concat`)
    out = task_head(dropout(fuse(cat)))                         plain torch; 'learned-3x3' head
                                                                upsamplings on HIP
Backward of the fused step is one launch (`ops.mlpdec_upsample_concat_backward`) behind
`MlpUpsampleConcatFunction`, which saves shapes only and asks the kernel only for the gradients
`needs_input_grad` names; the gradient of a branch that already has the output size is a view of the
upstream gradient.

The fused step is taken when every embedded map is on the GPU, every branch's `upsample` is a
non-learned `Upsampling` of one and the same mode, and the shapes pass `ops._mlpdec_shifts` (power-of-
two factors up to 16, at most four branches) with the largest map as the common output size.  The
dtype is the one the composition's concatenation has: torch.cat's promotion of what `interpolate`
returns for every map, which inside `torch.autocast('cuda')` may be float32 for half maps (torch is
asked, once per combination).  Maps of another dtype are cast with torch first: a full pass over the
factor-1 branch where that happens.
Anything else — CPU tensors, a learned mode, an odd factor, a fifth branch — takes the reference's
own composition, `branch.upsample(e)` per branch and `torch.cat`.  That composition is also the
baseline of tools/bench_mlp_decoder.py, and it lets the wiring be tested on a machine without a GPU.
The `upsample` modules stay in place for the state dict and for that composition; the fused step
does not call them.

State dict: the reference's keys and shapes (`main_branch.embedding.conv.*`, `skip_fusions.<i>.ln.*`,
`skip_branches.<i>.embedding.conv.*`, `fuse.conv.weight`, `fuse.norm.*`, and the task head's).

Stated deviation: a branch whose factor is 1 is copied; ATen's scale-1 bilinear turns -0 into +0 and
an inf next to a zero weight into NaN.
"""
import abc
from collections import OrderedDict
from typing import Optional, Sequence, Tuple, Type

import torch
from torch import nn
from torch.nn.functional import interpolate

from ... import ops
from ...types import DecoderInputType
from ...types import DecoderRawOutputType
from ...types import EncoderSkipsType
from ..activation import get_activation_class
from ..encoder_decoder_fusion import EncoderDecoderFusionType
from ..normalization import get_normalization_class
from ..upsampling import Upsampling
from ..upsampling import UpsamplingType
from ..upsampling import get_upsampling_class
from ..utils import ConvNormAct
from .base import DecoderBase


class MlpUpsampleConcatFunction(torch.autograd.Function):
    """cat = ops.mlpdec_upsample_concat(ys, mode); saves shapes only"""

    @staticmethod
    def forward(ctx, mode, *ys):
        ctx.mode = mode
        ctx.branch_shapes = tuple(tuple(y.shape) for y in ys)
        return ops.mlpdec_upsample_concat(ys, mode)

    @staticmethod
    def backward(ctx, g):
        need = ctx.needs_input_grad[1:]
        gys = (None,) * len(need)
        if any(need):
            gys = ops.mlpdec_upsample_concat_backward(g, ctx.branch_shapes, ctx.mode, need)
        return (None,) + tuple(gys)


def _fused_mode(upsamplings: Sequence[nn.Module], embedded: Sequence[torch.Tensor]) -> Optional[str]:
    """the one resize mode of the fused step, or None where the composition has to run"""
    if not all(e.is_cuda for e in embedded):
        return None
    if not all(isinstance(u, Upsampling) and not u._learned for u in upsamplings):
        return None
    modes = {u._mode for u in upsamplings}
    if len(modes) != 1:
        return None
    try:
        H, W, _ = ops._mlpdec_shifts([tuple(e.shape) for e in embedded])
    except ValueError:
        return None
    for u, e in zip(upsamplings, embedded):
        sf = u._scale_factor
        sh, sw = sf if isinstance(sf, (tuple, list)) else (sf, sf)
        if (e.shape[2] * sh, e.shape[3] * sw) != (H, W):    # the largest map is not the output size
            return None
    return modes.pop()


_AUTOCAST_RESIZED = {}


def _resized_dtype(e: torch.Tensor, mode: str) -> torch.dtype:
    """the dtype `interpolate` returns for this map in the current autocast state.  Which dtype autocast
    runs the resize in differs between torch builds, so it is asked of torch itself: once per
    combination, on a 1x1 map"""
    if not torch.is_autocast_enabled('cuda'):
        return e.dtype
    key = (e.dtype, mode, torch.get_autocast_dtype('cuda'))
    if key not in _AUTOCAST_RESIZED:
        probe = torch.zeros((1, 1, 1, 1), dtype=e.dtype, device=e.device)
        _AUTOCAST_RESIZED[key] = interpolate(probe, scale_factor=2, mode=mode,
                                             align_corners=False if mode == 'bilinear' else None).dtype
    return _AUTOCAST_RESIZED[key]


def upsample_concat(upsamplings: Sequence[nn.Module], embedded: Sequence[torch.Tensor]) -> torch.Tensor:
    """`torch.cat([u(e) for u, e in zip(upsamplings, embedded)], 1)`: one launch where the fused step
    applies (see the module docstring), the composition itself otherwise"""
    mode = _fused_mode(upsamplings, embedded)
    if mode is None:
        return torch.cat([u(e) for u, e in zip(upsamplings, embedded)], dim=1)
    dtype = _resized_dtype(embedded[0], mode)
    for e in embedded[1:]:
        dtype = torch.promote_types(dtype, _resized_dtype(e, mode))
    return MlpUpsampleConcatFunction.apply(mode, *(e if e.dtype == dtype else e.to(dtype) for e in embedded))


def _branch(n_channels_in: int, n_channels_out: int, upsampling: Type[UpsamplingType], scale_factor: int):
    return nn.Sequential(OrderedDict([
        ('embedding', ConvNormAct(n_channels_in, n_channels_out, kernel_size=1, normalization=None,
                                  activation=None)),
        ('upsample', upsampling(n_channels=n_channels_out, scale_factor=scale_factor)),
    ]))


class MLPDecoderBase(DecoderBase):
    def __init__(
        self,
        n_channels_in: int,
        downsampling_in: int,
        n_channels: Tuple[int, ...],
        fusion: Type[EncoderDecoderFusionType],
        fusion_n_channels: Tuple[int, ...],
        fusion_downsamplings: Tuple[int, ...],
        postprocessing: Type,
        downsampling_in_heads: int = 4,
        dropout_p: float = 0.1,
        n_channels_out: Optional[int] = None,
        normalization: Type[nn.Module] = get_normalization_class(),
        activation: Type[nn.Module] = get_activation_class(),
        upsampling: Type[UpsamplingType] = get_upsampling_class()
    ) -> None:
        super().__init__(postprocessing=postprocessing)
        assert len(n_channels) == 1 + len(fusion_n_channels)
        assert len(fusion_n_channels) == len(fusion_downsamplings)
        assert sorted(fusion_downsamplings, reverse=True) == list(fusion_downsamplings)
        self._fusion_downsamplings = fusion_downsamplings

        # the main branch from the encoder / context module, then one branch per encoder skip; the
        # fusion is a selection ('select*' / 'swin-ln-select*'): equal channel counts, no convolution
        self.main_branch = _branch(n_channels_in, n_channels[0], upsampling,
                                   downsampling_in // downsampling_in_heads)
        self.skip_fusions = nn.ModuleList(
            fusion(n_channels_encoder=n, n_channels_decoder=n, activation=None, normalization=None)
            for n in fusion_n_channels)
        self.skip_branches = nn.ModuleList(
            _branch(n_skip, n_dec, upsampling, down // downsampling_in_heads)
            for n_skip, n_dec, down in zip(fusion_n_channels, n_channels[1:], fusion_downsamplings))

        if n_channels_out is None:                          # SegFormer's default
            n_channels_out = sum(n_channels) // len(n_channels)
        self.fuse = ConvNormAct(sum(n_channels), n_channels_out, kernel_size=1,
                                normalization=normalization, activation=activation)
        self.dropout = nn.Dropout2d(dropout_p)

    def _forward_training(self, x: DecoderInputType, skips: EncoderSkipsType) -> DecoderRawOutputType:
        x, _ = x                                            # the context features are not used
        upsamplings = [self.main_branch.upsample]
        embedded = [self.main_branch.embedding(x)]
        for down, fusion, branch in zip(self._fusion_downsamplings, self.skip_fusions, self.skip_branches):
            upsamplings.append(branch.upsample)
            embedded.append(branch.embedding(fusion(x_enc=skips[str(down)], x_dec=None)))
        x = self.fuse(upsample_concat(upsamplings, embedded))
        x = self.dropout(x)
        return self.task_head(x), ()                        # MLP decoders have no side outputs

    @property
    @abc.abstractmethod
    def task_head(self) -> nn.Module:
        pass
