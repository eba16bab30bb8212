"""Task heads of the dense decoders (reference model/decoder/dense_utils.py): a convolution `conv`
(3x3 for a main output, 1x1 for a side output), `n_upsamplings` x2 upsamplings `upsample_<k>` and
optional `post_<k>` modules, under the reference's names.  Plain torch; the 'learned-3x3' upsamplings
run on HIP (`model.upsampling`)."""
from collections import OrderedDict
from typing import List, Optional, Type

from torch import nn


def create_task_head(n_channels_in: int, n_channels_out: int, upsampling: Optional[Type] = None,
                     n_upsamplings: int = 0, post_modules: Optional[List[nn.Module]] = None) -> nn.Module:
    is_main_output = n_upsamplings != 0
    modules = [('conv', nn.Conv2d(n_channels_in, n_channels_out, kernel_size=3 if is_main_output else 1,
                                  padding=1 if is_main_output else 0))]
    for i in range(n_upsamplings):
        modules.append((f'upsample_{i}', upsampling(n_channels=n_channels_out)))
    for i, module in enumerate(post_modules or ()):
        modules.append((f'post_{i}', module))
    return nn.Sequential(OrderedDict(modules))
