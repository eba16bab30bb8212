"""No context module (reference model/context_module/none.py): a 1x1 ConvNormAct where the channel
counts differ, the identity otherwise, and no context features.  Plain torch."""
from typing import Any, Type

from torch import nn

from ...types import ContextModuleInputType
from ...types import ContextModuleOutputType
from ..activation import get_activation_class
from ..normalization import get_normalization_class
from ..utils import ConvNormAct


class NoContextModule(nn.Module):
    def __init__(
        self,
        n_channels_in: int,
        n_channels_out: int,
        normalization: Type[nn.Module] = get_normalization_class(),
        activation: Type[nn.Module] = get_activation_class(),
        **kwargs: Any
    ) -> None:
        super().__init__()
        if n_channels_out != n_channels_in:
            self.layer = ConvNormAct(n_channels_in, n_channels_out, kernel_size=1,
                                     normalization=normalization, activation=activation)
        else:
            self.layer = nn.Identity()
        # no reduction here: n_channels_out stands in for it, which is what a scene decoder reads
        self.n_channels_reduction = n_channels_out

    def forward(self, x: ContextModuleInputType) -> ContextModuleOutputType:
        return self.layer(x), ()
