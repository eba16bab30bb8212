"""The interface every backbone offers the encoders (reference model/backbone/base.py): a list of stages with,
per stage, the channel count, the downsampling against the input and the memory layout of its output.  The
encoders run a backbone stage by stage (`forward_stage`), because the RGB-D fusion and the decoder skips read
every stage's output."""
import abc
from typing import List, Union

from torch import Tensor, nn


class Backbone(abc.ABC, nn.Module):
    def __init__(self) -> None:
        super().__init__()

    @property
    @abc.abstractmethod
    def stages(self) -> List[Union[nn.Sequential, nn.Module]]:
        """the stages in forward order"""

    @property
    @abc.abstractmethod
    def stages_n_channels(self) -> List[int]:
        """output channels of every stage"""

    @property
    @abc.abstractmethod
    def stages_downsampling(self) -> List[int]:
        """downsampling of every stage's output against the input"""

    @property
    @abc.abstractmethod
    def stages_memory_layout(self) -> List[str]:
        """'nchw' or 'nhwc' per stage"""

    def forward_stage(self, stage_idx: int, x: Tensor) -> Tensor:
        return self.stages[stage_idx](x)

    def forward(self, x: Tensor) -> Tensor:
        for idx in range(len(self.stages)):
            x = self.forward_stage(idx, x)
        return x
