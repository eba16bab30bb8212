"""The encoders of the reference (model/encoder.py): one backbone (`Encoder`) or an RGB and a depth backbone
fused after every stage (`FusedRGBDEncoder`), run stage by stage so that the decoder skips can be taken.

Input: a dict modality -> tensor ({'rgb': ..} / {'depth': ..} / {'rgbd': ..} for `Encoder`, both 'rgb' and
'depth' for `FusedRGBDEncoder`); it is not modified.  Output: (features, skips).  `features` has the input's
keys.  `skips` maps `str(downsampling)` to a dict modality -> tensor of the stage chosen for that downsampling
(a string, so that an ONNX export does not turn the key into a tensor).

Skip selection: for every requested downsampling the LAST stage with it; when that is the final stage (a
`-d16` backbone repeats 16 in its last two stages) the FIRST stage with it instead: the final stage is the
encoder's output, not a skip.

On the device the stages run `model.pooling.MaxPool2d` and the fused batch-norm tails of `model.block`, and the
fusions of `FusedRGBDEncoder` the SE-weighted add of `model.encoder_fusion`."""
import abc
from itertools import compress
from typing import Dict, List, Optional, Sequence, Tuple, Type, Union

from torch import Tensor, nn

from .activation import get_activation_class
from .backbone.base import Backbone
from .encoder_fusion import EncoderFusionType, get_encoder_fusion_class
from .normalization import get_normalization_class

EncoderInputType = Dict[str, Tensor]
EncoderSkipsType = Dict[str, Dict[str, Tensor]]
EncoderOutputType = Tuple[Dict[str, Tensor], EncoderSkipsType]


def select_skip_stages(stages_downsampling: Sequence[int], skip_downsamplings: Sequence[int]) -> List[bool]:
    """per stage: whether its output is a decoder skip (see the module docstring)"""
    stages = list(stages_downsampling)
    last = len(stages) - 1
    chosen = [False] * len(stages)
    for ds in skip_downsamplings:
        idx = last - stages[::-1].index(ds)              # ValueError for a downsampling no stage has
        if idx == last:
            idx = stages.index(ds)
        chosen[idx] = True
    return chosen


class EncoderBase(abc.ABC, nn.Module):
    def __init__(self) -> None:
        super().__init__()

    def _init_stages(self, backbone: Backbone, skip_downsamplings: Sequence[int]) -> None:
        self._n_stages = len(backbone.stages)
        self._stages_downsampling = backbone.stages_downsampling
        self._stages_n_channels = backbone.stages_n_channels
        self._skips_downsamplings = skip_downsamplings
        self._stages_skip_connections = select_skip_stages(self._stages_downsampling, skip_downsamplings)

    @property
    def skips_n_channels(self) -> Tuple[int, ...]:
        """channels of every skip connection"""
        return tuple(compress(self._stages_n_channels, self._stages_skip_connections))

    @property
    def skips_downsamplings(self) -> Sequence[int]:
        """downsampling of every skip connection"""
        return self._skips_downsamplings

    @property
    def n_channels_out(self) -> int:
        return self._stages_n_channels[-1]

    @property
    def downsampling(self) -> int:
        """the downsampling at the end of the encoder"""
        return self._stages_downsampling[-1]

    @abc.abstractmethod
    def forward(self, x: EncoderInputType) -> EncoderOutputType:
        pass


class Encoder(EncoderBase):
    """one backbone, one modality"""

    def __init__(self, backbone: Backbone, skip_downsamplings: Sequence[int] = (4, 8, 16)) -> None:
        super().__init__()
        self.backbone = backbone
        self._init_stages(backbone, skip_downsamplings)

    def forward(self, x: EncoderInputType) -> EncoderOutputType:
        assert len(x) == 1
        (key, out), = x.items()
        skips: EncoderSkipsType = {}
        taken = 0
        for idx in range(self._n_stages):
            out = self.backbone.forward_stage(idx, out)
            if self._stages_skip_connections[idx]:
                skips.setdefault(str(self.skips_downsamplings[taken]), {})[key] = out
                taken += 1
        return {key: out}, skips


class FusedRGBDEncoder(EncoderBase):
    """an RGB and a depth backbone with a fusion module behind every stage"""

    def __init__(self, backbone_rgb: Optional[Backbone], backbone_depth: Optional[Backbone],
                 fusion: Type[EncoderFusionType], normalization: Type[nn.Module] = get_normalization_class(),
                 activation: Type[nn.Module] = get_activation_class(),
                 skip_downsamplings: Sequence[int] = (4, 8, 16)) -> None:
        super().__init__()
        self.backbone_rgb = backbone_rgb
        self.backbone_depth = backbone_depth
        if backbone_rgb is not None and backbone_depth is not None:
            assert len(backbone_rgb.stages) == len(backbone_depth.stages)
            assert backbone_rgb.stages_n_channels == backbone_depth.stages_n_channels
            assert backbone_rgb.stages_downsampling == backbone_depth.stages_downsampling
            assert backbone_rgb.stages_memory_layout == backbone_depth.stages_memory_layout
            self.fusions = nn.ModuleList(
                fusion(n_channels_in=n, normalization=normalization, activation=activation,
                       input_memory_layout=layout)
                for n, layout in zip(backbone_rgb.stages_n_channels, backbone_rgb.stages_memory_layout))
        self._init_stages(backbone_rgb if backbone_rgb is not None else backbone_depth, skip_downsamplings)

    def forward(self, x: EncoderInputType) -> EncoderOutputType:
        assert len(x) == 2
        out = {'rgb': x['rgb'], 'depth': x['depth']}        # the input dict stays as it is
        skips: EncoderSkipsType = {}
        taken = 0
        for idx in range(self._n_stages):
            if self.backbone_rgb is not None:
                out['rgb'] = self.backbone_rgb.forward_stage(idx, out['rgb'])
            if self.backbone_depth is not None:
                out['depth'] = self.backbone_depth.forward_stage(idx, out['depth'])
            out = self.fusions[idx](out)
            if self._stages_skip_connections[idx]:
                skip = skips.setdefault(str(self.skips_downsamplings[taken]), {})
                skip['rgb'], skip['depth'] = out['rgb'], out['depth']
                taken += 1
        return out, skips


EncoderType = Union[Encoder, FusedRGBDEncoder]


def get_encoder(backbone_rgb: Optional[Backbone] = None, backbone_depth: Optional[Backbone] = None,
                backbone_rgbd: Optional[Backbone] = None, fusion: Optional[str] = None,
                normalization: str = 'batchnorm', activation: str = 'relu',
                skip_downsamplings: Sequence[int] = (4, 8, 16)) -> EncoderType:
    """both `backbone_rgb` and `backbone_depth`: the fused RGB-D encoder; `backbone_rgbd`, or exactly one of the
    two: a single-backbone encoder"""
    if backbone_rgb is not None and backbone_depth is not None:
        return FusedRGBDEncoder(backbone_rgb=backbone_rgb, backbone_depth=backbone_depth,
                                fusion=get_encoder_fusion_class(fusion),
                                normalization=get_normalization_class(normalization),
                                activation=get_activation_class(activation), skip_downsamplings=skip_downsamplings)
    if backbone_rgbd is not None:
        backbone = backbone_rgbd
    elif (backbone_rgb is not None) ^ (backbone_depth is not None):
        backbone = backbone_rgb if backbone_rgb is not None else backbone_depth
    else:
        raise ValueError('Either `backbone_rgb` and/or `backbone_depth` or `backbone_rgbd` must be given.')
    return Encoder(backbone=backbone, skip_downsamplings=skip_downsamplings)
