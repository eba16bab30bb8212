"""`ScenePostprocessing` on the MI355X (reference model/postprocessing/scene.py:15-53).

Training is a pass-through.  At inference the reference's softmax + max over the [B, C] logits
is one launch of k_scene_step (csrc/scene.hip) that writes the score and the index only.  The
index is the first index of the largest logit — what `torch.max(F.softmax(x, 1), 1)` returns on
the CPU wherever the two largest probabilities differ or the two largest logits are equal.
"""
from ... import ops
from ...types import BatchType
from ...types import DecoderRawOutputType
from ...types import PostprocessingOutputType
from .base import PostprocessingBase


class ScenePostprocessing(PostprocessingBase):
    def __init__(self, **kwargs) -> None:
        super().__init__()

    def _postprocess_training(
        self, data: DecoderRawOutputType, batch: BatchType
    ) -> PostprocessingOutputType:
        output, side_outputs = data
        return {'scene_output': output}

    def _postprocess_inference(
        self, data: DecoderRawOutputType, batch: BatchType
    ) -> PostprocessingOutputType:
        output, side_outputs = data             # (there are no side outputs)
        r = ops.scene_step(output, want=('score', 'idx'))
        # ('scene_output' is part of the inference dict too, as in the reference: scene.py:47-51)
        return {'scene_class_score': r['score'], 'scene_class_idx': r['idx'], 'scene_output': output}
