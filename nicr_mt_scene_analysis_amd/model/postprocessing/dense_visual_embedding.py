"""`DenseVisualEmbeddingPostprocessing` on the MI355X
(reference model/postprocessing/dense_visual_embedding.py:19-167).

The reference normalises the decoder output in place (`norm`, `div_`), runs one 1x1 `conv2d` per
set of class embeddings and then softmax + max, at the network and at the dataset resolution.
Here `nmsa_dve_project` normalises and projects for both sets in one pass over the embedding map;
everything after the logits is the semantic task's code path (`SemanticPostprocessing`'s argmax /
resize entries under this task's keys): class maps now, softmax tensors, scores and
full-resolution logits when somebody reads them.
"""
from typing import Optional

import torch

from ... import ops
from ...types import BatchType
from ...types import DecoderRawOutputType
from ...types import PostprocessingOutputType
from ._lazy import LazyDict
from .dense_base import DensePostprocessingBase
from .semantic import SemanticPostprocessing

_TEXT = 'dense_visual_embedding_text_based_'
_VISUAL_MEAN = 'dense_visual_embedding_visual_mean_based_'


class DenseVisualEmbeddingPostprocessing(DensePostprocessingBase):
    def __init__(
        self,
        with_text_embeddings_per_class: bool = False,
        text_embeddings_per_class: Optional[torch.Tensor] = None,
        with_mean_visual_embedding_per_class: bool = False,
        mean_visual_embedding_per_class: Optional[torch.Tensor] = None,
        **kwargs
    ):
        super().__init__()
        self.with_semantic_text_embeddings = with_text_embeddings_per_class
        self._semantic_text_embeddings = None
        if self.with_semantic_text_embeddings:
            assert text_embeddings_per_class is not None
            self._semantic_text_embeddings = text_embeddings_per_class

        self.with_mean_visual_embedding_per_class = with_mean_visual_embedding_per_class
        self._mean_visual_embedding_per_class = None
        if self.with_mean_visual_embedding_per_class:
            assert mean_visual_embedding_per_class is not None
            self._mean_visual_embedding_per_class = mean_visual_embedding_per_class
        # device -> (key, [C, D] float32 copies of the class embeddings next to the predictions)
        self._on_device = {}

    def _postprocess_training(
        self, data: DecoderRawOutputType, batch: BatchType
    ) -> PostprocessingOutputType:
        output, side_outputs = data
        return {'dense_visual_embedding_output': output,
                'dense_visual_embedding_side_outputs': side_outputs}

    def _weights(self, device: torch.device):
        """[C, D] float32 class embeddings on `device`.  The reference reads its tensors on every
        call; the copies here are keyed on the tensors' storage and in-place version counter, so
        embeddings updated in place (mean visual embeddings recomputed per epoch) are copied anew"""
        src = (self._semantic_text_embeddings, self._mean_visual_embedding_per_class)
        key = tuple(None if t is None else (t.data_ptr(), t._version) for t in src)
        cached = self._on_device.get(device)
        if cached is None or cached[0] != key:
            cached = (key, tuple(None if t is None else
                                 t.detach().to(device=device, dtype=torch.float32).contiguous()
                                 for t in src))
            self._on_device[device] = cached
        return cached[1]

    def _postprocess_inference(
        self, data: DecoderRawOutputType, batch: BatchType
    ) -> PostprocessingOutputType:
        output, side_outputs = data
        r = LazyDict(dense_visual_embedding_output=output,
                     dense_visual_embedding_side_outputs=side_outputs)
        # `output /= output.norm(dim=1, keepdim=True)` and both projections: one launch sequence
        text, visual_mean = self._weights(output.device)
        logits = ops.dve_project(output, text, visual_mean)
        for prefix, head_logits in zip((_TEXT, _VISUAL_MEAN), logits):
            if head_logits is None:
                continue
            r[prefix + 'semantic_output'] = head_logits
            SemanticPostprocessing._argmax_entries(r, head_logits, prefix=prefix, stem='semantic')
            SemanticPostprocessing._fullres_entries(r, head_logits, batch, prefix=prefix,
                                                    stem='semantic')
        return r
