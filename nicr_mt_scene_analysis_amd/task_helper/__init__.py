"""Task helpers on the hot path (reference task_helper/__init__.py): every task of the
reference, the scene classification (`SceneTaskHelper`, one launch per step) included."""
from .base import TaskHelperBase
from .base import get_total_loss_key
from .dense_visual_embedding import DenseVisualEmbeddingTaskHelper
from .instance import InstanceTaskHelper
from .normal import NormalTaskHelper
from .panoptic import PanopticTaskHelper
from .scene import SceneTaskHelper
from .semantic import SemanticTaskHelper
