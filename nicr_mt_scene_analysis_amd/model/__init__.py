from .upsampling import KNOWN_UPSAMPLING_METHODS
from .upsampling import Upsampling
from .upsampling import UpsamplingType
from .upsampling import get_upsampling_class
