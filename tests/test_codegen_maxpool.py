"""CPU tier: code-generation guard for csrc/maxpool.hip (the harness is tests/_codegen.py).  The forward kernel
keeps three scanned rows of up to four (value, bits, position) choices per lane, the backward kernel two window
rows of five gradients and codes and eight sums: scratch or spilled registers would mean one of them went to
memory."""
import pytest

import _codegen


@pytest.fixture(scope='module')
def usage():
    return _codegen.usage('maxpool.hip')


def test_every_maxpool_kernel_has_no_scratch_and_no_spills(usage):
    # forward and backward: 3 dtypes x (VECTOR, PIXEL)
    _codegen.assert_clean(usage, {'k_mp_fwd': 6, 'k_mp_bwd': 6}, whole_file=True)
