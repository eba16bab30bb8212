"""The MLP (SegFormer-style) decoders of the reference's model/decoder package; their resize +
concatenation step runs on HIP (see mlp_base.py), the scene classification decoder, whose global pool and
linear head are one HIP launch (see scene.py), the convolutional dense decoders, whose x2 upsampling and
skip addition are one HIP launch per decoder module (see dense_base.py), and the panoptic helper (plain
torch)."""
from .base import DecoderBase
from .dense_utils import create_task_head
from .dense_base import DenseDecoderBase
from .dense_base import DenseDecoderModule
from .dense_base import UpsampleAddFunction
from .mlp_base import MLPDecoderBase
from .mlp_base import MlpUpsampleConcatFunction
from .embedding import EmbeddingMLPDecoder
from .semantic import SemanticDecoder
from .semantic import SemanticMLPDecoder
from .instance import InstanceHead
from .instance import InstanceDecoder
from .instance import InstanceMLPDecoder
from .normal import NormalDecoder
from .normal import NormalMLPDecoder
from .scene import SceneClassificationDecoder
from .scene import SceneHeadFunction
from .panoptic import PanopticHelper
