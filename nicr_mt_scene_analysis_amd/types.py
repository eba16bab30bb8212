"""Type aliases used in the signatures of the hot-path API
(names as in the reference's types.py:33-47)."""
from typing import Any, Dict, Tuple, Union

from torch import Tensor

BatchType = Dict[str, Any]
DecoderRawOutputType = Tuple[Any, Any]          # (outputs, side_outputs)
DecoderPostprocessedOutputType = Dict[str, Any]
PostprocessingOutputType = DecoderPostprocessedOutputType
TensorOrTuple = Union[Tensor, Tuple[Tensor, ...]]

# context module (reference types.py:23-26)
ContextModuleInputType = Tensor
ContextModuleContextFeaturesType = Union[Tuple[Tensor, ...], Tuple[()]]
ContextModuleOutputType = Tuple[Tensor, ContextModuleContextFeaturesType]

# encoder and decoder (reference types.py:17-21, 29, 49)
EncoderForwardType = Dict[str, Tensor]              # modality: features
EncoderSkipType = EncoderForwardType
EncoderSkipsType = Dict[str, EncoderSkipType]       # downsampling: skip features
DecoderInputType = ContextModuleOutputType
DecoderOutputType = Union[DecoderRawOutputType, DecoderPostprocessedOutputType]
