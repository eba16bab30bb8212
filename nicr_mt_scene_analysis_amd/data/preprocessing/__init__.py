"""The batch helpers the hot-path callers use, plus the on-device target generators of
SURVEY.md §8 f4 and `BatchAugmentation`, the numpy steps of the reference's training chain (crop, flip, normalise,
HWC -> CHW) in one launch; the chain's cv2 steps (`RandomResize`, `RandomHSVJitter`, the upscale of
`RandomCrop`) stay out of scope."""
from .augmentation import BatchAugmentation
from .base import APPLIED_PREPROCESSING_KEY
from .base import get_applied_preprocessing_meta
from .multiscale_supervision import MultiscaleSupervisionGenerator
from .multiscale_supervision import cv2_nearest_map
from .multiscale_supervision import get_downscale
from .resize import FULLRES_SUFFIX
from .resize import get_fullres
from .resize import get_fullres_key
from .resize import get_fullres_shape
from .resize import get_valid_region_slices
from .resize import get_valid_region_slices_and_fullres_shape
from .dense_visual_embedding import DenseVisualEmbeddingTargetGenerator
from .instance import InstanceClearStuffIDs
from .instance import InstanceTargetGenerator
from .orientation import OrientationTargetGenerator
from .panoptic import PanopticTargetGenerator
