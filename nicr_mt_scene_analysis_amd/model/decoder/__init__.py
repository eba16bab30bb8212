"""The MLP (SegFormer-style) decoders of the reference's model/decoder package; their resize +
concatenation step runs on HIP (see mlp_base.py), the scene classification decoder, whose global pool and
linear head are one HIP launch (see scene.py), and the panoptic helper (plain torch).  The
convolutional dense decoders are not part of this package."""
from .base import DecoderBase
from .dense_utils import create_task_head
from .mlp_base import MLPDecoderBase
from .mlp_base import MlpUpsampleConcatFunction
from .embedding import EmbeddingMLPDecoder
from .semantic import SemanticMLPDecoder
from .instance import InstanceHead
from .instance import InstanceMLPDecoder
from .normal import NormalMLPDecoder
from .scene import SceneClassificationDecoder
from .scene import SceneHeadFunction
from .panoptic import PanopticHelper
