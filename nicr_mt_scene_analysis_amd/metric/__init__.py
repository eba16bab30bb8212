"""Metric accumulators of the hot path (reference metric/__init__.py)."""
from .base import Metric
from .confmat import ConfusionMatrix
from .mae import MeanAbsoluteAngularError
from .mae import PanopticQualityWithOrientationMAE
from .miou import MeanIntersectionOverUnion
from .pq import PanopticQuality
from .rmse import RootMeanSquaredError
