"""Convolutional dense decoder (reference model/decoder/dense_base.py, `DenseDecoderModule` and
`DenseDecoderBase`) with the end of its decoder modules on the HIP kernel of csrc/up_add.hip.

A decoder module is `conv` (3x3 ConvNormAct) -> `blocks` (`model.block`) -> `upsample` (x2 `Upsampling`, or
`nn.Identity()` for a module that keeps the resolution).  The decoder chains one module per entry of
`n_channels` / `downsamplings`, and where the resolution reached is one of `fusion_downsamplings` an encoder
skip is fused in by `fusions.<j>` (`model.encoder_decoder_fusion`).  In training mode the map in front of every
upsampling is kept as a side output (multiscale supervision); in eval mode the side outputs are None.

The fused step.  For the 'add*' fusions the reference runs `upsample(out)` and then `layer(skip) + u`: two
passes, 17 units of the low-resolution map read and written.  `ops.up2x_add` does both in ONE launch (9 units)
behind `UpsampleAddFunction`.  `_fused_mode` decides per step; it says yes when the module's `upsample` is an
`Upsampling` of factor 2, the fusion is a plain `EncoderDecoderFusion` that adds, `e = fusion.layer(skip)` and
the map in front of the upsampling are both fused maps (`utils.fused_map`: on the device, float32 / bfloat16 /
float16, dense NCHW) of one dtype with shapes [B, C, h, w] and [B, C, 2h, 2w], and autocast is off.  Everything
else — the 'swin-*' fusions (they have their own fused node), 'select*', 'none', a module without upsampling,
CPU tensors, channels-last, autocast — runs the reference's composition with the same torch calls.
Backward has nothing to fuse: the gradient of `e` is the upstream gradient itself (the same tensor, no copy),
the gradient of the map is the upsampling's backward (`ops.upsample2x_dw3x3_backward` for the learned modes,
`ops.mlpdec_upsample_concat_backward` with one branch of factor 2 for nearest / bilinear), both deterministic.
What stays in torch: the convolutions, the blocks (their batch-norm tails are `model.block`'s business), the
task heads and `fusion.layer` (the 1x1 channel adapter of a skip with another channel count).

`DenseDecoderModule.forward(x)` on its own is the reference's: `(upsampled, side)`.

State dict: the reference's keys and shapes (`decoder_modules.<i>.{conv,blocks,upsample}.*`,
`fusions.<j>.layer.*`, and the heads of the subclasses); the `upsample` modules stay in place for it and for the
composition, the fused step reads their parameters and does not call them.

Stated deviation: the fused step rounds a half result once, after the addition; the composition rounds the
upsampled map and the sum.  In float32 nearest is bit-identical, the other modes differ by the order and
fusing of float32 operations only.
"""
import abc
from typing import Optional, Tuple, Type

import torch
from torch import Tensor, nn

from ... import ops
from ...types import DecoderInputType
from ...types import DecoderRawOutputType
from ...types import EncoderSkipsType
from ..activation import get_activation_class
from ..block import BlockType
from ..encoder_decoder_fusion import EncoderDecoderFusion
from ..encoder_decoder_fusion import EncoderDecoderFusionSwin
from ..encoder_decoder_fusion import EncoderDecoderFusionType
from ..normalization import get_normalization_class
from ..upsampling import Upsampling
from ..upsampling import UpsamplingType
from ..upsampling import get_upsampling_class
from ..utils import ConvNormAct, f32_master, fused_map
from .base import DecoderBase


class UpsampleAddFunction(torch.autograd.Function):
    """y = ops.up2x_add(x, skip, mode, weight, bias); saves x and weight in the learned modes and nothing
    map-sized otherwise, asks the upsampling's backward only for the gradients `needs_input_grad` names and
    hands the upstream gradient itself on as the gradient of `skip`"""

    @staticmethod
    def forward(ctx, x, skip, weight, bias, mode):
        ctx.mode = mode
        ctx.learned = mode.startswith('learned-3x3')
        if ctx.learned:
            ctx.save_for_backward(x, weight)
        else:
            ctx.x_shape = tuple(x.shape)
        return ops.up2x_add(x, skip, mode, weight, bias)

    @staticmethod
    def backward(ctx, gy):
        need_gx, need_skip, need_gw, need_gb = ctx.needs_input_grad[:4]
        gx = gw = gb = None
        if ctx.learned:
            if need_gx or need_gw or need_gb:
                x, weight = ctx.saved_tensors
                gx, gw, gb = ops.upsample2x_dw3x3_backward(gy, x, weight, ctx.mode == 'learned-3x3-zeropad',
                                                           need_gx, need_gw, need_gb)
        elif need_gx:
            gx, = ops.mlpdec_upsample_concat_backward(gy, [ctx.x_shape], ctx.mode)
        return gx, (gy if need_skip else None), gw, gb, None


def _fusable(upsample: nn.Module, fusion: nn.Module) -> bool:
    """the part of `_fused_mode` that the modules decide: an x2 `Upsampling` followed by a plain adding fusion"""
    # the factories hand out subclasses (`partial_class`); the Swin fusion is one as well, with its own fused node
    if not isinstance(upsample, Upsampling) or not isinstance(fusion, EncoderDecoderFusion):
        return False
    if isinstance(fusion, EncoderDecoderFusionSwin):
        return False
    sf = upsample._scale_factor
    if tuple(sf if isinstance(sf, (tuple, list)) else (sf, sf)) != (2, 2):
        return False
    return fusion._fuse_operation is torch.add


def _fused_mode(upsample: nn.Module, fusion: nn.Module, x: Tensor, e: Tensor) -> Optional[str]:
    """the upsampling mode of the fused step for the map `x` in front of `upsample` and the adapted skip
    `e = fusion.layer(skip)`, or None where the composition has to run"""
    if not _fusable(upsample, fusion):
        return None
    if not (fused_map(x) and fused_map(e)) or x.dtype != e.dtype or x.device != e.device:
        return None
    if tuple(e.shape) != (x.shape[0], x.shape[1], 2 * x.shape[2], 2 * x.shape[3]):
        return None
    if torch.is_autocast_enabled('cuda'):
        return None
    if upsample._learned:
        return 'learned-3x3-zeropad' if upsample._zeropad else 'learned-3x3'
    return upsample._mode


def upsample_add(upsample: nn.Module, fusion: nn.Module, x: Tensor, e: Tensor) -> Tensor:
    """`fusion._fuse_operation(e, upsample(x))` for a pair `_fusable` accepts: one launch where `_fused_mode`
    names a mode, the composition itself otherwise"""
    mode = _fused_mode(upsample, fusion, x, e)
    if mode is None:
        return fusion._fuse_operation(e, upsample(x))
    weight = bias = None
    if upsample._learned:
        weight, bias = f32_master(upsample.conv.weight, upsample.conv.bias)
    return UpsampleAddFunction.apply(x, e, weight, bias, mode)


class DenseDecoderModule(nn.Module):
    def __init__(
        self,
        n_channels_in: int,
        n_channels: int,
        block: Type[BlockType],
        n_blocks: int,
        initial_conv: bool = True,
        activation: Type[nn.Module] = get_activation_class(),
        normalization: Type[nn.Module] = get_normalization_class(),
        upsampling: Optional[Type[UpsamplingType]] = get_upsampling_class()
    ) -> None:
        super().__init__()
        if initial_conv:
            self.conv = ConvNormAct(n_channels_in, n_channels, kernel_size=3, normalization=normalization,
                                    activation=activation)
            widths = [n_channels] * (n_blocks + 1)
        else:
            assert n_blocks > 0
            self.conv = nn.Identity()
            widths = [n_channels_in] + [n_channels] * n_blocks
        blocks = []
        for n_in, n_out in zip(widths[:-1], widths[1:]):
            # a block that changes the channel count carries a 1x1 adapter on its identity path
            downsample = None if n_in == n_out else ConvNormAct(n_in, n_out, kernel_size=1, activation=None)
            blocks.append(block(inplanes=n_in, planes=n_out, stride=1, downsample=downsample, groups=1,
                                base_width=64, dilation=1, normalization=normalization, activation=activation))
        self.blocks = nn.Sequential(*blocks)
        self.upsample = upsampling(n_channels=n_channels) if upsampling is not None else nn.Identity()

    def features(self, x: Tensor) -> Tensor:
        """the map in front of the upsampling: the side output of the module"""
        return self.blocks(self.conv(x))

    def forward(self, x: Tensor) -> Tuple[Tensor, Optional[Tensor]]:
        out = self.features(x)
        return self.upsample(out), (out if self.training else None)


class DenseDecoderBase(DecoderBase):
    def __init__(
        self,
        n_channels_in: int,
        downsampling_in: int,
        n_channels: Tuple[int, ...],
        downsamplings: Tuple[int, ...],
        block: Type[BlockType],
        n_blocks: int,
        fusion: Type[EncoderDecoderFusionType],
        fusion_n_channels: Tuple[int, ...],
        fusion_downsamplings: Tuple[int, ...],
        postprocessing: Type,
        normalization: Type[nn.Module] = get_normalization_class(),
        activation: Type[nn.Module] = get_activation_class(),
        upsampling: Type[UpsamplingType] = get_upsampling_class()
    ) -> None:
        super().__init__(postprocessing=postprocessing)
        assert len(n_channels) == len(downsamplings)
        assert sorted(downsamplings, reverse=True) == list(downsamplings)
        assert all(d <= downsampling_in for d in downsamplings)
        assert len(fusion_n_channels) == len(fusion_downsamplings)
        assert sorted(fusion_downsamplings, reverse=True) == list(fusion_downsamplings)

        # one module per entry; a module upsamples (and gets a side output in front of its upsampling) only
        # where its entry lowers the downsampling; a skip is fused in wherever the downsampling reached is listed
        modules, fusions = [], []
        side_downscales, side_n_channels, with_side, fused_at = [], [], [], []
        current = downsampling_in
        for n_in, n_out, down in zip((n_channels_in,) + tuple(n_channels[:-1]), n_channels, downsamplings):
            upsamples = down < current
            with_side.append(upsamples)
            if upsamples:
                side_downscales.append(current)
                side_n_channels.append(n_out)
                current = down
            modules.append(DenseDecoderModule(n_channels_in=n_in, n_channels=n_out, block=block, n_blocks=n_blocks,
                                              activation=activation, normalization=normalization,
                                              upsampling=upsampling if upsamples else None))
            if current in fusion_downsamplings:
                fused_at.append(current)
                fusions.append(fusion(n_channels_encoder=fusion_n_channels[len(fusions)], n_channels_decoder=n_out,
                                      activation=activation, normalization=normalization))
            else:
                fused_at.append(-1)
        self.decoder_modules = nn.ModuleList(modules)
        self.fusions = nn.ModuleList(fusions)
        self._side_output_downscales = tuple(side_downscales)
        self._side_output_n_channels = tuple(side_n_channels)
        self._decoder_modules_consider_side_output = tuple(with_side)
        self._decoder_modules_fusion_downsamplings = tuple(fused_at)

    @property
    @abc.abstractmethod
    def task_head(self) -> nn.Module:
        pass

    @property
    @abc.abstractmethod
    def side_output_heads(self) -> nn.ModuleList:
        pass

    @property
    def side_output_downscales(self) -> Tuple[int, ...]:
        return self._side_output_downscales

    @property
    def side_output_n_channels(self) -> Tuple[int, ...]:
        return self._side_output_n_channels

    def _forward_decoder_modules(self, x: Tensor, skips: EncoderSkipsType) -> DecoderRawOutputType:
        assert len(skips) == len(self.fusions)
        side_outputs = []
        fusions = iter(self.fusions)
        for module, with_side, down in zip(self.decoder_modules, self._decoder_modules_consider_side_output,
                                           self._decoder_modules_fusion_downsamplings):
            fusion = next(fusions) if down != -1 else None
            if fusion is not None and _fusable(module.upsample, fusion):
                out = module.features(x)
                side = out if module.training else None
                # the keys are strings, as the reference's (an ONNX export would turn integer keys into tensors)
                e = fusion.layer(fusion._encoder_features(skips[str(down)]))
                x = upsample_add(module.upsample, fusion, out, e)
            else:
                x, side = module(x)
                if fusion is not None:
                    x = fusion(x_enc=skips[str(down)], x_dec=x)
            if with_side:
                side_outputs.append(side)
        return x, tuple(side_outputs)

    def _forward_training(self, x: DecoderInputType, skips: EncoderSkipsType) -> DecoderRawOutputType:
        x, _ = x                                            # the context features are not used
        output, side_outputs = self._forward_decoder_modules(x, skips)
        output = self.task_head(output)
        side_outputs = tuple(None if side is None else head(side)
                             for head, side in zip(self.side_output_heads, side_outputs))
        return output, side_outputs
