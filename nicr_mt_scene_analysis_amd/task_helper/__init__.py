"""Task helpers on the hot path (reference task_helper/__init__.py).
`SceneTaskHelper` belongs to another task and is out of scope."""
from .base import TaskHelperBase
from .base import get_total_loss_key
from .dense_visual_embedding import DenseVisualEmbeddingTaskHelper
from .instance import InstanceTaskHelper
from .normal import NormalTaskHelper
from .panoptic import PanopticTaskHelper
from .semantic import SemanticTaskHelper
