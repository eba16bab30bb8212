"""Helpers the GPU tests share: import what a file needs (pytest picks an imported fixture up)."""
import os

import numpy as np
import pytest
import torch


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture
def assume_cus():
    """NMSA_ASSUME_CUS (read by the library at every call), restored afterwards.  set_cus(n) -> the
    compute units the library sizes its grids from now; None: the device's own count"""
    from nicr_mt_scene_analysis_amd import _lib as L
    saved = os.environ.get('NMSA_ASSUME_CUS')
    own = torch.cuda.get_device_properties(0).multi_processor_count

    def set_cus(n):
        if n is None:
            os.environ.pop('NMSA_ASSUME_CUS', None)
        else:
            os.environ['NMSA_ASSUME_CUS'] = str(n)
        cus = L.device_geometry()[0]
        assert cus == (own if n is None else n), 'the library does not follow NMSA_ASSUME_CUS'
        return cus
    yield set_cus
    if saved is None:
        os.environ.pop('NMSA_ASSUME_CUS', None)
    else:
        os.environ['NMSA_ASSUME_CUS'] = saved
