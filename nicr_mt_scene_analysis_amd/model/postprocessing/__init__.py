"""Postprocessing factory (reference model/postprocessing/__init__.py:24-44).

On the hot path: 'semantic', 'instance', 'panoptic' and 'dense-visual-embedding' (in-place
normalisation + projection onto the class embeddings on HIP, class maps through the semantic
path).  `NormalPostprocessing` exists as a class (lazy nearest resize to the dataset resolution)
but is not registered here yet: the factory still raises NotImplementedError for 'normal', which
an existing test pins; registering it is a follow-up that flips that assertion.  The same holds
for 'scene': `ScenePostprocessing` (softmax score and index of the [B, C] logits in one launch)
exists as a class and is used directly; the factory keeps raising for the name."""
from typing import Any

from ...utils import partial_class
from .base import PostprocessingBase
from .dense_base import DensePostprocessingBase
from .dense_visual_embedding import DenseVisualEmbeddingPostprocessing
from .instance import InstancePostprocessing
from .normal import NormalPostprocessing
from .panoptic import PanopticPostprocessing
from .scene import ScenePostprocessing
from .semantic import SemanticPostprocessing

_OUT_OF_SCOPE = ('normal', 'scene')


def get_postprocessing_class(name: str, **kwargs: Any):
    if name == 'semantic':
        cls = SemanticPostprocessing
    elif name == 'instance':
        cls = InstancePostprocessing
    elif name == 'panoptic':
        cls = PanopticPostprocessing
    elif name == 'dense-visual-embedding':
        cls = DenseVisualEmbeddingPostprocessing
    elif name in _OUT_OF_SCOPE:
        raise NotImplementedError(
            f"postprocessing '{name}' is not part of the MI355X hot path; use the "
            "reference implementation for it")
    else:
        raise ValueError(f"Unknown postprocessing: '{name}'")
    return partial_class(cls, **kwargs)
