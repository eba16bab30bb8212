"""`ConfusionMatrix`: an int64 [C, C] state on the device, row = target, column = prediction
(what the reference's scene task takes from torchmetrics, task_helper/scene.py:44-52, there kept
on the CPU).  The scene step's kernel (csrc/scene.hip) adds into the state tensor directly
(`SceneTaskHelper.validation_step`); `update` exists for API parity and goes through k_confmat
(csrc/metrics.hip); an index out of range there sets a device word that `check_status()` reads."""
from typing import Optional

import torch

from .. import _lib as L
from .base import Metric
from .miou import confmat_update


class ConfusionMatrix(Metric):
    def __init__(self, num_classes: int, device: Optional[torch.device] = None, **kwargs) -> None:
        super().__init__(device=device, **kwargs)
        self.add_state('confmat', torch.zeros((num_classes, num_classes), dtype=torch.int64),
                       dist_reduce_fx='sum')
        self._n_classes = num_classes
        self._status = torch.zeros((1,), dtype=torch.int32, device=self.device)

    def to(self, device, *args, **kwargs):
        super().to(device)
        self._status = self._status.to(self.device)
        return self

    def state_for_kernel(self) -> torch.Tensor:
        """the packed state tensor a kernel adds into (its address is stable from here on: graph
        captures hold it); refuses while the states are summed over the ranks"""
        self._require_unsynced()
        if self.device.type != 'cuda':
            raise L.NmsaError('ConfusionMatrix needs the MI355X (the state lives on the GPU; '
                              'no CPU fallback)')
        self._pack()
        return self.confmat

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        """preds / target: class indices [N] in [0, num_classes), no void entries"""
        confmat_update(self.state_for_kernel(), self._status, preds, target, self._n_classes)

    def check_status(self) -> None:
        """raises when `update` saw an index outside [0, num_classes) since the last call (the
        reference raises in bincount); a host sync"""
        if int(self._status.item()):
            self._status.zero_()
            raise ValueError('ConfusionMatrix: index outside [0, num_classes)')

    def compute(self) -> torch.Tensor:
        # a copy: under a process group the state holds the ranks' sum only inside this call
        return self.confmat.clone()
