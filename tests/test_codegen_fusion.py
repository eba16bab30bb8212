"""CPU tier: code-generation guard for csrc/ln_transpose.hip (the harness is tests/_codegen.py).  The
forward kernel holds a row of up to 32 values per lane (and their squared deviations) for the two
summation trees, the backward kernel 16 row-sum partials per lane, all indexed by compile-time
constants after unrolling: scratch or spilled registers would mean a row went to memory."""
import pytest

import _codegen


@pytest.fixture(scope='module')
def usage():
    return _codegen.usage('ln_transpose.hip')


def test_every_fusion_kernel_has_no_scratch_and_no_spills(usage):
    # 5 dtype pairs x (vector, element) of the forward and of the backward kernel, and the reducer
    _codegen.assert_clean(usage, {'k_lnt_fwd': 10, 'k_lnt_bwd': 10, 'k_lnt_reduce': 1}, whole_file=True)
