"""The residual blocks of the ResNet backbones and the convolutional decoders (reference model/block.py).

`get_block_class(name)` with the reference's three names and its default 'nonbottleneck1d':
  'basicblock'        `BasicBlock`, two 3x3 convolutions (ResNet v1)
  'bottleneck'        `Bottleneck`, 1x1 - 3x3 - 1x1 with the stride at the 3x3 convolution (ResNet v1.5)
  'nonbottleneck1d'   `NonBottleneck1D`, the basic block with spatially factorised 3x1 / 1x3 convolutions (ERFNet)
Constructor signatures, defaults, `expansion`, the refusals and the sub-module names are the reference's, so
its checkpoints load with `strict=True`.  The convolutions, the activations behind a biased convolution
(`act1_1`, `act2_1`) and the `downsample` branch are torch.

The batch-norm tail on the device.  Every norm-to-activation segment of a block,
  BasicBlock        norm1 -> act1;   norm2 -> (+ identity) -> act2
  Bottleneck        norm1 -> act1;   norm2 -> act2;   norm3 -> (+ identity) -> act3
  NonBottleneck1D   norm1 -> act1_2; norm2 -> dropout -> (+ identity) -> act2_2
is ONE autograd node, `BatchNormTailFunction`: at most two HIP launches forward (`ops.bntail_stats`,
`ops.bntail_apply`; one in eval mode) and two backward (`ops.bntail_backward_reduce`,
`ops.bntail_backward_apply`).  It saves x, the output y (ReLU: the gate is 0 where y <= 0, so a NaN
y passes the gradient as ATen's threshold backward does) or the identity (SiLU: z is
recomputed), the Dropout2d scale [B, C] and per-channel vectors; the normalised map, the dropout product and
the sum are never written.  The `norm*` sub-modules stay the `nn.BatchNorm2d` modules `normalization(planes)`
returns: the fused path reads their parameters and buffers and writes their running statistics.  The
Dropout2d scale is drawn with the calls ATen's feature dropout makes, so one seed gives the planes
`F.dropout2d` zeroes.
Fused when: x (and the identity) CUDA, 4-D, dense NCHW, one dtype of float32 / bfloat16 / float16; the norm an
`nn.BatchNorm2d` with `affine`, `track_running_stats` and a float `momentum`; the activation `nn.ReLU` or
`nn.SiLU`.  After `module.half()` the parameters and buffers are cast to float32 for the kernels.
Everything else runs the reference's own composition in torch: CPU tensors, channels-last or non-dense
inputs, mixed dtypes (an f32 identity beside a half main path under autocast), another normalization or
activation, `momentum=None`, `affine=False`, `track_running_stats=False`, and, for speed, maps of fewer than
`FUSED_MIN_ELEMENTS` elements: below it a segment is bound by host time per call, of which the fused path
spends more than the torch composition it replaces (measured).
"""
from typing import Any, Optional, Type, Union

import torch
from torch import Tensor, nn

from .. import ops
from ..utils import partial_class
from .activation import get_activation_class
from .normalization import get_normalization_class
from .utils import conv1x1, conv3x3, f32_master, fused_map

KNOWN_BLOCKS = ('basicblock', 'bottleneck', 'nonbottleneck1d')

# elements of a map (B*C*H*W) from which the fused path is taken: measured faster end to end at 8 x 64 x 120 x 160
# (9.8M) and slower at 8 x 128 x 60 x 80 (2.5M) and below; sizes between the two were not measured
# and stay on torch
FUSED_MIN_ELEMENTS = 8 * 2 ** 20


class BatchNormTailFunction(torch.autograd.Function):
    """y = act(bn(x) * scale[b, c] + identity) over a whole norm-to-activation segment (include/nmsa.h,
    nmsa_bntail_*).  `running_mean` / `running_var` (float32) are updated in place when `training`.
    Gradients: x, identity, gamma, beta; only the passes somebody needs are launched: no reduction without a
    gradient of x or of the parameters (and none in eval mode with frozen parameters), no map pass
    without a gradient of x or of the identity.  Nothing is saved when nothing needs a gradient or gradients
    are switched off (`grad_enabled`: inside `forward` they always are, so the caller passes
    `torch.is_grad_enabled()`)."""

    @staticmethod
    def forward(ctx, x, identity, scale, gamma, beta, running_mean, running_var, training, eps, momentum, act,
                grad_enabled):
        need = ctx.needs_input_grad
        save = grad_enabled and (need[0] or need[1] or need[3] or need[4])
        part = ops.bntail_stats(x) if training else None
        out = ops.bntail_apply(x, gamma, beta, running_mean, running_var, eps, momentum if training else 0.0, act,
                               part=part, identity=identity, scale=scale, save=save)
        ctx.act, ctx.training = act, training
        if not save:
            return out
        y, mean, invstd = out
        ctx.has_identity = identity is not None
        aux = y if act == 'relu' else identity
        ctx.save_for_backward(x, aux, scale, gamma, beta if act == 'silu' else None, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, gy):
        need_x, need_id, _, need_g, need_b = ctx.needs_input_grad[:5]
        need_id = need_id and ctx.has_identity
        need_p = need_g or need_b
        x, aux, scale, gamma, beta, mean, invstd = ctx.saved_tensors
        gy = gy.contiguous()
        args = (gy, x, aux, gamma, beta, mean, invstd, ctx.act)
        gx = gid = dgamma = dbeta = None
        if ctx.training and need_x:
            part = ops.bntail_backward_reduce(*args, scale=scale)
            gx, gid, dgamma, dbeta = ops.bntail_backward_apply(*args, scale=scale, part=part, need_x=True,
                                                               need_identity=need_id, need_params=need_p)
        else:
            if need_p:
                dgamma, dbeta = ops.bntail_backward_reduce(*args, scale=scale, finish=True)
            if need_x or need_id:
                gx, gid, _, _ = ops.bntail_backward_apply(*args, scale=scale, need_x=need_x, need_identity=need_id)
        return (gx, gid, None, dgamma if need_g else None, dbeta if need_b else None,
                None, None, None, None, None, None, None)


def _fused_act(norm: nn.Module, act: nn.Module, x: Tensor, identity: Optional[Tensor]) -> Optional[str]:
    """the activation code of the fused HIP path, None when this segment takes the torch composition"""
    if not fused_map(x) or x.numel() < FUSED_MIN_ELEMENTS:
        return None
    if identity is not None and not (identity.device == x.device and identity.shape == x.shape
                                     and identity.dtype == x.dtype and identity.is_contiguous()):
        return None
    if not (isinstance(norm, nn.BatchNorm2d) and norm.affine and norm.track_running_stats
            and isinstance(norm.momentum, float) and norm.running_mean is not None):
        return None
    for cls, code in ((nn.ReLU, 'relu'), (nn.SiLU, 'silu')):
        if isinstance(act, cls):
            return code
    return None


def dropout2d_scale(x: Tensor, p: float) -> Tensor:
    """the [B, C, 1, 1] scale of `F.dropout2d(x, p, training=True)`, 0 or 1 / (1 - p), drawn with the calls
    ATen's feature dropout makes: under one seed the same planes are zeroed"""
    return x.new_empty((x.shape[0], x.shape[1], 1, 1)).bernoulli_(1 - p).div_(1 - p)


def batch_norm_tail(norm: nn.Module, act: nn.Module, x: Tensor, identity: Optional[Tensor] = None,
                    dropout: Optional[nn.Dropout2d] = None) -> Tensor:
    """act(dropout(norm(x)) + identity): the fused HIP path where it applies (see the module docstring), the
    reference's composition in torch everywhere else"""
    drawing = dropout is not None and dropout.training and dropout.p > 0
    code = None if drawing and dropout.p >= 1 else _fused_act(norm, act, x, identity)
    if code is None:
        out = norm(x)
        if dropout is not None:
            out = dropout(out)
        if identity is not None:
            out = out + identity
        return act(out)
    training = norm.training
    if training and x.numel() // x.shape[1] < 2:
        raise ValueError(f'Expected more than 1 value per channel when training, got input size {x.size()}')
    scale = dropout2d_scale(x, dropout.p) if drawing else None
    gamma, beta, rm, rv = f32_master(norm.weight, norm.bias, norm.running_mean, norm.running_var)
    y = BatchNormTailFunction.apply(x, identity, scale, gamma, beta, rm, rv, training, norm.eps, norm.momentum, code,
                                    torch.is_grad_enabled())
    if training:
        with torch.no_grad():
            if rm is not norm.running_mean:                 # module.half(): the kernels wrote float32 copies
                norm.running_mean.copy_(rm)
                norm.running_var.copy_(rv)
            norm.num_batches_tracked.add_(1)
    return y


class BasicBlock(nn.Module):
    expansion: int = 1

    def __init__(self, inplanes: int, planes: int, stride: int = 1, downsample: Optional[nn.Module] = None,
                 groups: int = 1, base_width: int = 64, dilation: int = 1,
                 normalization: Type[nn.Module] = get_normalization_class(),
                 activation: Type[nn.Module] = get_activation_class(), **kwargs: Any) -> None:
        super().__init__()
        if groups != 1 or base_width != 64:
            raise ValueError('BasicBlock only supports groups=1 and base_width=64')
        if dilation > 1:
            raise NotImplementedError('Dilation > 1 not supported in BasicBlock')
        # conv1 and the downsample branch both carry the stride
        self.conv1 = conv3x3(inplanes, planes, stride)
        self.norm1 = normalization(planes)
        self.act1 = activation()
        self.conv2 = conv3x3(planes, planes)
        self.norm2 = normalization(planes)
        self.act2 = activation()
        self.downsample = downsample
        self.stride = stride

    def forward(self, x: Tensor) -> Tensor:
        out = batch_norm_tail(self.norm1, self.act1, self.conv1(x))
        out = self.conv2(out)
        identity = x if self.downsample is None else self.downsample(x)
        return batch_norm_tail(self.norm2, self.act2, out, identity)


class Bottleneck(nn.Module):
    expansion: int = 4

    def __init__(self, inplanes: int, planes: int, stride: int = 1, downsample: Optional[nn.Module] = None,
                 groups: int = 1, base_width: int = 64, dilation: int = 1,
                 normalization: Type[nn.Module] = get_normalization_class(),
                 activation: Type[nn.Module] = get_activation_class(), **kwargs: Any) -> None:
        super().__init__()
        width = int(planes * (base_width / 64.0)) * groups
        # conv2 and the downsample branch both carry the stride (ResNet v1.5)
        self.conv1 = conv1x1(inplanes, width)
        self.norm1 = normalization(width)
        self.act1 = activation()
        self.conv2 = conv3x3(width, width, stride, groups, dilation)
        self.norm2 = normalization(width)
        self.act2 = activation()
        self.conv3 = conv1x1(width, planes * self.expansion)
        self.norm3 = normalization(planes * self.expansion)
        self.act3 = activation()
        self.downsample = downsample
        self.stride = stride

    def forward(self, x: Tensor) -> Tensor:
        out = batch_norm_tail(self.norm1, self.act1, self.conv1(x))
        out = batch_norm_tail(self.norm2, self.act2, self.conv2(out))
        out = self.conv3(out)
        identity = x if self.downsample is None else self.downsample(x)
        return batch_norm_tail(self.norm3, self.act3, out, identity)


class NonBottleneck1D(nn.Module):
    expansion = 1

    def __init__(self, inplanes: int, planes: int, stride: int = 1, downsample: Optional[nn.Module] = None,
                 groups: int = 1, base_width: int = 64, dilation: int = 1,
                 normalization: Type[nn.Module] = get_normalization_class(),
                 activation: Type[nn.Module] = get_activation_class(), dropout_p: float = 0.2,
                 **kwargs: Any) -> None:
        super().__init__()
        if groups != 1 or base_width != 64:
            raise ValueError('NonBottleneck1D only supports groups=1 and base_width=64')
        self.conv1_1 = nn.Conv2d(inplanes, planes, (3, 1), stride=(stride, 1), padding=(1, 0), bias=True)
        self.act1_1 = activation()
        self.conv1_2 = nn.Conv2d(planes, planes, (1, 3), stride=(1, stride), padding=(0, 1), bias=False)
        self.norm1 = normalization(planes)
        self.act1_2 = activation()
        self.conv2_1 = nn.Conv2d(planes, planes, (3, 1), padding=(dilation, 0), bias=True, dilation=(dilation, 1))
        self.act2_1 = activation()
        self.conv2_2 = nn.Conv2d(planes, planes, (1, 3), padding=(0, dilation), bias=False, dilation=(1, dilation))
        self.norm2 = normalization(planes)
        self.act2_2 = activation()
        self.dropout = nn.Dropout2d(p=dropout_p)            # whole channels, not positions
        self.downsample = downsample
        self.stride = stride
        self.dropout_p = dropout_p

    def forward(self, input: Tensor) -> Tensor:
        out = self.conv1_2(self.act1_1(self.conv1_1(input)))
        out = batch_norm_tail(self.norm1, self.act1_2, out)
        out = self.conv2_2(self.act2_1(self.conv2_1(out)))
        identity = input if self.downsample is None else self.downsample(input)
        return batch_norm_tail(self.norm2, self.act2_2, out, identity,
                               self.dropout if self.dropout_p > 0 else None)


BlockType = Union[BasicBlock, Bottleneck, NonBottleneck1D]


def get_block_class(name: Optional[str] = None, **kwargs: Any) -> Type[BlockType]:
    if name is None:
        name = 'nonbottleneck1d'            # the reference's global default
    name = name.lower()
    if name not in KNOWN_BLOCKS:
        raise ValueError(f"Unknown block: '{name}'")
    block = {'basicblock': BasicBlock, 'bottleneck': Bottleneck, 'nonbottleneck1d': NonBottleneck1D}[name]
    return partial_class(block, **kwargs)
