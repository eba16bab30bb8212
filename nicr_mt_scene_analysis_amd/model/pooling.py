"""The stem max pool of the ResNet backbones on the device.

`MaxPool2d` is `nn.MaxPool2d` with one more path: for the ResNet stem's configuration, kernel 3, stride 2,
padding 1, dilation 1, `ceil_mode=False`, `return_indices=False`, and a CUDA, 4-D, dense NCHW input of float32 /
bfloat16 / float16 it is ONE autograd node, `MaxPool3x3S2Function`: one HIP launch forward
(`ops.maxpool3x3s2`) and one backward (`ops.maxpool3x3s2_backward`).  The training forward writes a one-byte
window-position code per output pixel where ATen's `max_pool2d_with_indices` writes an int64 index, and the
backward reads it back: 11 bytes moved per output pixel of a half map in each direction against 18.  The node
saves only the code.  Without gradients no code is allocated or written.  The selection is ATen's (the first
maximum of a window, the last NaN), y carries the selected element's bits; the backward is a gather with
float32 sums in a fixed order rounded once, where ATen's half kernels round after every add.
Everything else calls `nn.MaxPool2d.forward` unchanged: other kernel sizes, strides, paddings or dilations,
`ceil_mode`, `return_indices`, CPU tensors, 3-D inputs, channels-last or non-dense inputs, other dtypes, empty
tensors.  Autocast: max pooling keeps its input's dtype under autocast in torch, and so does this path.
"""
import torch
from torch import Tensor, nn
from torch.autograd.function import once_differentiable

from .. import ops
from .utils import fused_map


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


class MaxPool3x3S2Function(torch.autograd.Function):
    """y = max_pool2d(x, 3, 2, 1) (include/nmsa.h, nmsa_maxpool3x3s2_*).  Saves the uint8 code alone; nothing
    when x needs no gradient or gradients are switched off (`grad_enabled`: inside `forward` they always are,
    so the caller passes `torch.is_grad_enabled()`)."""

    @staticmethod
    def forward(ctx, x, grad_enabled):
        save = grad_enabled and ctx.needs_input_grad[0]
        y, code = ops.maxpool3x3s2(x, need_code=save)
        if save:
            ctx.input_hw = (int(x.shape[2]), int(x.shape[3]))
            ctx.save_for_backward(code)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        code, = ctx.saved_tensors
        return ops.maxpool3x3s2_backward(gy.contiguous(), code, ctx.input_hw), None


class MaxPool2d(nn.MaxPool2d):
    def takes_hip_path(self, x: Tensor) -> bool:
        """whether `forward(x)` runs the HIP kernels (see the module docstring)"""
        stride = self.kernel_size if self.stride is None else self.stride
        if not (_pair(self.kernel_size) == (3, 3) and _pair(stride) == (2, 2) and _pair(self.padding) == (1, 1)
                and _pair(self.dilation) == (1, 1) and not self.ceil_mode and not self.return_indices):
            return False
        return fused_map(x)

    def forward(self, input: Tensor):
        if not self.takes_hip_path(input):
            return super().forward(input)
        return MaxPool3x3S2Function.apply(input, torch.is_grad_enabled())
