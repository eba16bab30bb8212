"""`CrossEntropyLossScene`: the scene head's loss (reference task_helper/scene.py:37-42, a plain
`torch.nn.CrossEntropyLoss(weight, label_smoothing, ignore_index=-1, reduction='mean')`) on the
one-launch kernel k_scene_step (csrc/scene.hip).

The forward call is that launch; it also writes d loss / d logits when the input requires a
gradient, and backward multiplies it with the upstream gradient.  The tensor is B x C elements:
there is nothing to speculate about, unlike the dense losses."""
from typing import Optional

import torch

from .. import ops


class _SceneCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input_, labels, weights, label_smoothing):
        needs_grad = ctx.needs_input_grad[0]
        out = ops.scene_step(input_, labels, weights, label_smoothing,
                             want=('loss', 'grad') if needs_grad else ('loss',))
        if needs_grad:
            ctx.save_for_backward(out['grad'])
        return out['loss'][2]

    @staticmethod
    def backward(ctx, grad_output):
        grad, = ctx.saved_tensors
        return (grad_output * grad).to(grad.dtype), None, None, None


class CrossEntropyLossScene(torch.nn.Module):
    def __init__(self, weights: Optional[torch.Tensor] = None, label_smoothing: float = 0.0) -> None:
        super().__init__()
        self._weights = weights
        self._label_smoothing = float(label_smoothing)

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """input [B, C] logits; target [B] int64 class indices, -1 = ignore -> the mean loss (0-dim)"""
        # the kernel takes the label form of batch['scene']: 0 = void, class c is c + 1
        return self.from_labels(input, target + 1)

    def from_labels(self, input: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        """the same with labels in the form of batch['scene'] (uint8 / int32 / int64, 0 = void, class
        c is c + 1): no op besides the launch"""
        return _SceneCE.apply(input, labels, self._weights, self._label_smoothing)
