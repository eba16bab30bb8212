"""`get_backbone(name, resnet_block, ...)`: the reference's factory (model/backbone/__init__.py) for its twelve
ResNet names.  The Swin backbones need torchvision and are not provided.

Weights.  The library never downloads.  `pretrained=True` (the reference's default) needs `pretrained_filepath`:
the checkpoint's `state_dict` (or `model`) container is rewritten as the reference rewrites it, the prefixes
`model.`, `backbone.` and `_orig_mod.` removed, the classifier keys (`fc.*`, `fc_embedding.*`) dropped,
`conv1.weight` summed for a 1-channel input and, for 4 channels, concatenated with its sum and halved, and
loaded with `strict=True`.  Without a path it raises; pass `pretrained=False` for random weights."""
from collections import OrderedDict
from typing import Any, Optional, Type, Union

import torch

from ..activation import get_activation_class
from ..block import BlockType, get_block_class
from ..normalization import get_normalization_class
from .base import Backbone
from .resnet import ResNetBackbone
from .resnet import ResNetSEBackbone
from .resnet import ResNetStem
from .resnet import adapt_conv1_weight
from .resnet import convert_torchvision_resnet_state_dict
from .resnet import get_resnet_backbone

KNOWN_BACKBONES = [
    'resnet18', 'resnet34', 'resnet50', 'resnet101',
    # dilation in the last stage: downsampling 16
    'resnet18-d16', 'resnet34-d16', 'resnet50-d16', 'resnet101-d16',
    # SqueezeAndExcitation at the end of every stage
    'resnet18se', 'resnet34se', 'resnet50se', 'resnet101se',
]

_CHECKPOINT_PREFIXES = ('model.', 'backbone.', '_orig_mod.')
_CHECKPOINT_DROPPED = ('fc.weight', 'fc.bias', 'fc_embedding.weight', 'fc_embedding.bias')


def rewrite_checkpoint_state_dict(checkpoint: dict, n_input_channels: int = 3) -> 'OrderedDict[str, torch.Tensor]':
    """the backbone state dict of a loaded checkpoint (see the module docstring)"""
    weights = checkpoint['state_dict'] if 'state_dict' in checkpoint else checkpoint['model']
    state = OrderedDict()
    for key, value in weights.items():
        for prefix in _CHECKPOINT_PREFIXES:
            key = key.replace(prefix, '')
        state[key] = value
    for key in _CHECKPOINT_DROPPED:
        state.pop(key, None)
    if 'conv1.weight' in state:
        state['conv1.weight'] = adapt_conv1_weight(state['conv1.weight'], n_input_channels)
    return state


def get_backbone(name: str, resnet_block: Union[str, Type[BlockType]], n_input_channels: int = 3,
                 normalization: Union[str, Type[torch.nn.Module]] = 'batchnorm',
                 activation: Union[str, Type[torch.nn.Module]] = 'relu', pretrained: bool = True,
                 pretrained_filepath: Optional[str] = None, **kwargs: Any) -> Backbone:
    name = name.lower()
    if isinstance(normalization, str):
        normalization = get_normalization_class(normalization)
    if isinstance(activation, str):
        activation = get_activation_class(activation)
    if 'swin' in name:
        raise ValueError(f"Backbone '{name}': the Swin backbones need torchvision and are not provided by this "
                         f'package.  Known backbones: {KNOWN_BACKBONES}')
    if name not in KNOWN_BACKBONES:
        raise ValueError(f'Unknown backbone: {name}')
    if pretrained and pretrained_filepath is None:
        raise ValueError('pretrained=True needs `pretrained_filepath`: this library never downloads weights.  '
                         'Pass the path of a checkpoint, or pretrained=False for random weights.')
    if isinstance(resnet_block, str):
        resnet_block = get_block_class(resnet_block)
    dilate = [False, False, True] if 'd16' in name else None
    backbone = get_resnet_backbone(name, resnet_block, pretrained_torchvision=False, normalization=normalization,
                                   activation=activation, n_input_channels=n_input_channels,
                                   replace_stride_with_dilation=dilate, **kwargs)
    if pretrained:
        checkpoint = torch.load(pretrained_filepath, map_location='cpu', weights_only=False)   # old checkpoints pickle
        backbone.load_state_dict(rewrite_checkpoint_state_dict(checkpoint, n_input_channels), strict=True)
    return backbone
