"""`SceneTaskHelper` (reference task_helper/scene.py:18-132): cross entropy over the scene
classes with void ignored, accuracy and balanced accuracy from a confusion matrix.

The reference's validation step waits for the device three times per batch — a Python
`sum(mask) > 0` and two `.cpu()` copies — and updates a torchmetrics matrix on the host.  Here a
step is ONE launch of k_scene_step (csrc/scene.hip) and nothing is awaited:
  training_step     loss + d loss / d logits (`CrossEntropyLossScene`)
  validation_step   loss + the confusion-matrix update, added into the metric's device state
The kernel takes `batch['scene']` as it is (0 = void, class c is c + 1): void rows add nothing to
either, an all-void batch needs no branch on the host (its loss is 0 / 0 = NaN, as torch's), and
the step can be captured in a graph.

The matrix's column is derived from `scene_output` by the kernel itself — the same code that
produced `scene_class_idx` in `ScenePostprocessing`, so the two agree by construction;
`predictions_post['scene_class_idx']` is not read.  A label above the number of classes (the
reference raises in the loss) sets a status bit on the device and counts as void;
`check_status()` reads it."""
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch

from .. import ops
from ..loss import CrossEntropyLossScene
from ..metric import ConfusionMatrix
from .base import TaskHelperBase
from .base import append_detached_losses_to_logs
from .base import append_profile_to_logs


class SceneTaskHelper(TaskHelperBase):
    def __init__(self, n_classes: int, class_weights: Optional[np.ndarray] = None,
                 label_smoothing: float = 0.0) -> None:
        super().__init__()
        self._class_weights = class_weights
        self._label_smoothing = label_smoothing
        self._n_classes = n_classes

    def initialize(self, device: torch.device):
        if self._class_weights is not None:
            self._class_weights = torch.as_tensor(self._class_weights, device=device).float()
        self._loss = CrossEntropyLossScene(weights=self._class_weights,
                                           label_smoothing=self._label_smoothing)
        self._metric_cm = ConfusionMatrix(num_classes=self._n_classes, device=device)
        self._status = torch.zeros((1,), dtype=torch.int32, device=device)

    @staticmethod
    def _labels(batch) -> torch.Tensor:
        labels = batch['scene']
        if labels.dtype not in (torch.uint8, torch.int32, torch.int64):
            labels = labels.long()
        return labels

    @append_profile_to_logs('scene_step_time')
    @append_detached_losses_to_logs()
    def training_step(self, batch, batch_idx, predictions_post
                      ) -> Tuple[Dict[str, torch.Tensor], Dict[str, Any]]:
        # (the labels as they are: the reference's `target - 1` with ignore_index=-1 is the kernel's
        # 0 = void rule)
        total = self._loss.from_labels(predictions_post['scene_output'], self._labels(batch))
        return {self.mark_as_total('scene'): total}, {}

    @append_profile_to_logs('scene_step_time')
    @append_detached_losses_to_logs()
    def validation_step(self, batch, batch_idx, predictions_post
                        ) -> Tuple[Dict[str, torch.Tensor], Dict[str, Any]]:
        r = ops.scene_step(predictions_post['scene_output'], self._labels(batch), self._class_weights,
                           self._label_smoothing, want=('loss',),
                           confmat=self._metric_cm.state_for_kernel(), status=self._status)
        return {self.mark_as_total('scene'): r['loss'][2]}, {}

    def check_status(self) -> None:
        """raises when a label above n_classes was seen since the last call (a host sync)"""
        if int(self._status.item()):
            self._status.zero_()
            raise ValueError('SceneTaskHelper: scene label outside [0, n_classes]')

    @append_profile_to_logs('scene_epoch_end_time')
    def validation_epoch_end(self):
        # the reference's expressions (scene.py:115-122) on the device matrix; the boolean indexing
        # and the host mean wait for the device, once per epoch
        cm = self._metric_cm.confmat
        tp = torch.diag(cm)
        gt = torch.sum(cm, dim=1)
        tp = tp[gt != 0]                        # ignore empty classes
        gt = gt[gt != 0]
        acc = tp.sum().float() / gt.sum().float()
        # the mean alone on the host, where the reference takes it: the per-class ratios are one
        # IEEE division each, but a float32 mean reduced on the device may add in another order
        bacc = torch.mean((tp.float() / gt.float()).cpu()).to(cm.device)
        artifacts = {'scene_cm': cm.clone()}
        logs = {'scene_acc': acc, 'scene_bacc': bacc}
        self._metric_cm.reset()                 # (it is not done automatically)
        return artifacts, {}, logs
