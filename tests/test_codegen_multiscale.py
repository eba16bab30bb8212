"""CPU tier: code-generation guard for csrc/multiscale.hip (the harness is tests/_codegen.py).  The
gather kernel keeps its descriptor in scalar registers and a handful of values per lane: scratch or
spilled registers would mean the descriptor copy went to memory."""
import pytest

import _codegen


@pytest.fixture(scope='module')
def usage():
    return _codegen.usage('multiscale.hip')


def test_gather_kernel_has_no_scratch_and_no_spills(usage):
    _codegen.assert_clean(usage, {'k_multiscale_nearest': 1})   # one kernel for every element size
