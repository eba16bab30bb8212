"""Batch-meta keys written by the reference's preprocessing pipeline
(reference data/preprocessing/base.py:17-30); the hot path only READS them."""
import re
from typing import Any, Callable, Dict, List

MULTI_DOWNSCALE_KEY_FMT = '_down_{}'
APPLIED_PREPROCESSING_KEY = '_applied_preprocessing'


def get_applied_preprocessing_meta(sample: Dict[str, Any]) -> List[Any]:
    return sample.setdefault(APPLIED_PREPROCESSING_KEY, [])


_DOWNSCALE_KEY = re.compile(MULTI_DOWNSCALE_KEY_FMT.format('([0-9]+)'))


def apply_to_downscales(batch: Dict[str, Any],
                        preprocess: Callable[[Dict[str, Any], int], Dict[str, Any]]) -> None:
    """The `multiscale_processing` loop of the reference's `PreprocessingBase.__call__`
    (base.py:80-93): `batch[key] = preprocess(batch[key], downscale)` for every key that matches
    `_down_<k>`, in the batch's key order."""
    for key in batch:
        m = _DOWNSCALE_KEY.match(key)
        if m is not None:
            batch[key] = preprocess(batch[key], int(m.group(1)))
