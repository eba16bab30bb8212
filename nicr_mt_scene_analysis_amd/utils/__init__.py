from ._misc import partial_class
from ._orientation import biternion2deg
from ._orientation import biternion2rad
from ._orientation import np_rad2biternion
from . import panoptic_merge
from ._tables import IdTable
from ._tables import OrientationTable
