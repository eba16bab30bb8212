"""`RootMeanSquaredError` with device-resident states (reference metric/rmse.py:12-62):
the per-pixel root of the channel-mean squared error, averaged over the valid pixels.
`update` is the HIP kernel k_rmse (csrc/normal.hip): it adds into the two states on the
device, without a host sync, and can be captured in a graph."""
from typing import Optional, Tuple, Union

import torch

from .. import _lib as L
from .. import ops
from .base import Metric


class RootMeanSquaredError(Metric):
    def __init__(self, device: Optional[torch.device] = None, **kwargs) -> None:
        super().__init__(device=device, **kwargs)
        self.add_state('sum_root_mean_squared_error', torch.tensor(0, dtype=torch.float64),
                       dist_reduce_fx='sum')
        self.add_state('n_observations', torch.tensor(0, dtype=torch.int64), dist_reduce_fx='sum')

    def _require_gpu(self) -> None:
        if self.device.type != 'cuda':
            raise L.NmsaError('RootMeanSquaredError.update needs the MI355X '
                              '(states live on the GPU; no CPU fallback)')
        self._pack()

    def update(self, preds: torch.Tensor, target: torch.Tensor,
               mask: Optional[torch.Tensor] = None) -> None:
        """preds / target [B,C,H,W]; mask: bool [B,H,W] of the pixels to consider, or None"""
        self._require_gpu()
        ops.rmse_update(self.sum_root_mean_squared_error, self.n_observations, preds, target, mask)

    def update_from_network_resolution(
        self, preds: torch.Tensor, valid_region_slices: Optional[Tuple[slice, slice]],
        target: torch.Tensor, mask: Union[None, str, torch.Tensor] = 'target'
    ) -> None:
        """`update(resize_nearest(preds[..., valid_region_slices], target.shape[-2:]), target, mask)`
        (what NormalPostprocessing + NormalTaskHelper.validation_step do in the reference) from
        the network-resolution prediction: every target pixel reads its nearest source, the
        full-resolution prediction is not materialised.  mask='target': the valid-normal rule
        (some channel of the target != 0), evaluated on the fly."""
        self._require_gpu()
        crop = valid_region_slices if valid_region_slices is not None else (slice(None), slice(None))
        ops.rmse_update(self.sum_root_mean_squared_error, self.n_observations, preds, target, mask,
                        crop=crop)

    def compute(self) -> torch.Tensor:
        rmse = self.sum_root_mean_squared_error / self.n_observations      # 0 / 0: NaN, as the reference
        return rmse.to(torch.float32)
