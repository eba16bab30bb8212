"""CPU tier: code-generation guard for csrc/normal.hip (the harness is tests/_codegen.py).  Both
kernels are streaming passes with a handful of live values per lane; scratch or spilled registers
would add memory traffic to a memory-bound pass."""
import pytest

import _codegen


@pytest.fixture(scope='module')
def usage():
    return _codegen.usage('normal.hip')


@pytest.mark.parametrize('kernel, variants', [('k_normal_valid_mask', 2), ('k_rmse', 36)])
def test_kernels_have_no_scratch_and_no_spills(usage, kernel, variants):
    # mask: vector / scalar; rmse: 3 dtypes x 3 masks x 2 sources x 2
    _codegen.assert_clean(usage, {kernel: variants})
