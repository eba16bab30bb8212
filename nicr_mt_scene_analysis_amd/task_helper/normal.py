"""`NormalTaskHelper` (reference task_helper/normal.py:27-167): MSE | L1 loss on the valid
ground-truth normals of every supervision scale, RMSE at the dataset resolution at validation.

The reference builds the valid mask with three compares, two ANDs and a NOT, counts it with a
`sum().item()` host sync per scale and multiplies the prediction with it.  Here the mask is one
pass of `nmsa_normal_valid_mask`, the masking is folded into the HIP loss kernels and the
counts stay on the device.  The validation RMSE reads the network-resolution prediction and
derives the mask from the target inside the kernel (`nmsa_rmse_update`).

A scale without any valid pixel: its `normal_loss_<scale>` is 0 / 0 = NaN, as in the reference;
it adds nothing to the total, which divides the summed losses by the summed counts (the summed
losses themselves when no scale has a valid pixel).  Visualisation examples are out of scope
(`_examples` stays empty)."""
from typing import Any, Dict

import torch

from ..data.preprocessing.resize import get_fullres
from ..data.preprocessing.resize import get_fullres_key
from ..loss import _functional as F_
from ..loss import L1Loss
from ..loss import MSELoss
from ..metric import RootMeanSquaredError
from ..model.postprocessing.normal import AUX_SOURCE_KEY
from .. import ops
from .base import TaskHelperBase
from .base import append_detached_losses_to_logs
from .base import append_profile_to_logs

KNOWN_NORMAL_LOSS_FUNCTIONS = ('mse', 'l1')


class NormalTaskHelper(TaskHelperBase):
    def __init__(self, loss_name: str, disable_multiscale_supervision: bool = False) -> None:
        super().__init__()
        assert loss_name in KNOWN_NORMAL_LOSS_FUNCTIONS
        self._loss_name = loss_name
        self._loss_class = {'mse': MSELoss, 'l1': L1Loss}[loss_name]
        self._disable_multiscale_supervision = disable_multiscale_supervision
        self._examples: Dict[str, Any] = {}

    def initialize(self, device: torch.device):
        self._loss = self._loss_class(reduction='sum')
        self._metric_rmse = RootMeanSquaredError(device=device)

    def _compute_losses(self, batch, batch_idx, predictions_post) -> Dict[str, torch.Tensor]:
        no_multiscale = self._disable_multiscale_supervision
        preds, targets, keys = self.collect_predictions_and_targets_for_loss(
            batch=batch, batch_key='normal', predictions_post=predictions_post,
            predictions_post_key='normal_output',
            side_outputs_key=None if no_multiscale else 'normal_side_outputs')
        # pixels with a ground-truth normal, per scale: pred*mask vs target, n = sum(mask)
        # (normal.py:69-92); targets of invalid pixels are zero, so they add f(0 - 0) = 0
        items = [{'kind': self._loss_name, 'pred': p.contiguous(), 'target': t,
                  'mask': ops.normal_valid_mask(t), 'total': 0} for p, t in zip(preds, targets)]
        names = [f'normal_loss_{k}' for k in keys]
        from ..loss import _multi
        if F_.speculation_enabled() and F_.wants_gradient(preds[0]) and _multi.supported(items):
            # every scale in ONE forward call that also writes the gradients
            return self.multi_losses(items, names, ('normal',))
        out = [self._loss.masked_sum(it['pred'], it['target'], it['mask']) for it in items]
        loss_dict = {name: l / n for name, (l, n) in zip(names, out)}
        loss_dict[self.mark_as_total('normal')] = self.accumulate_losses(
            [l for l, _ in out], [n for _, n in out])
        return loss_dict

    @append_profile_to_logs('normal_step_time')
    @append_detached_losses_to_logs()
    def training_step(self, batch, batch_idx, predictions_post):
        return self._compute_losses(batch, batch_idx, predictions_post), {}

    @append_profile_to_logs('normal_step_time')
    @append_detached_losses_to_logs()
    def validation_step(self, batch, batch_idx, predictions_post):
        loss_dict = self._compute_losses(batch, batch_idx, predictions_post)
        target = get_fullres(batch, 'normal')
        source = getattr(predictions_post, 'aux', {}).get(AUX_SOURCE_KEY)
        if source is not None:
            # crop + nearest resize + mask + RMSE in one pass over the target
            output, crop = source
            self._metric_rmse.update_from_network_resolution(output, crop, target, mask='target')
        else:
            self._metric_rmse.update(preds=predictions_post[get_fullres_key('normal_output')],
                                     target=target, mask=ops.normal_valid_mask(target))
        return loss_dict, {}

    @append_profile_to_logs('normal_epoch_end_time')
    def validation_epoch_end(self):
        logs = {'normal_rmse': self._metric_rmse.compute()}
        self._metric_rmse.reset()
        return {}, self._examples, logs
