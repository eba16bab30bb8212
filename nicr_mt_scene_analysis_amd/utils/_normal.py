"""Unit-length output of the decoder heads (reference utils/_normal.py, utils/_torch.py:60-63).
Plain torch."""
import torch


def unit_length(x: torch.Tensor, epsilon: float = 1e-7) -> torch.Tensor:
    norm = torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True))
    return x / (norm + epsilon)


class NormalOutputNormalization(torch.nn.Module):
    def __init__(self, epsilon=1e-7) -> None:
        super().__init__()
        self._epsilon = epsilon

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return unit_length(x, self._epsilon)


class OrientationOutputNormalization(NormalOutputNormalization):
    """(cos, sin) on the unit circle: the same operation on two channels"""
