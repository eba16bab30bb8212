"""CPU tier: code-generation guard for csrc/upsampling.hip (the harness is tests/_codegen.py).  The
forward kernel keeps three input rows, the backward kernel a 4-row window of gy (up to 40 values on
the half vector route) plus ten accumulators per lane, all indexed by compile-time constants after
unrolling: scratch or spilled registers would mean a window went to memory."""
import pytest

import _codegen


@pytest.fixture(scope='module')
def usage():
    return _codegen.usage('upsampling.hip')


def test_every_upsampling_kernel_has_no_scratch_and_no_spills(usage):
    # 3 dtypes x (vector, one-pixel) of the forward and of the backward kernel, and the reducer
    _codegen.assert_clean(usage, {'k_up_fwd': 6, 'k_up_bwd': 6, 'k_up_reduce': 1}, whole_file=True)
