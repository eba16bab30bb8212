"""CPU tier: code-generation guard for the orientation paint kernel of csrc/targets.hip (the harness
is tests/_codegen.py).  The paint is a streaming pass (4 B/px read, 9 B/px written) with a handful
of live values per lane; scratch or spilled registers would add memory traffic to a memory-bound
pass."""
import pytest

import _codegen

VARIANTS = 4        # (on-wire 16-byte accesses | per-pixel) x (probe of the scan's id table | binary search in LDS)


@pytest.fixture(scope='module')
def usage():
    return _codegen.usage('targets.hip')


def test_paint_kernel_has_no_scratch_and_no_spills(usage):
    _codegen.assert_clean(usage, {'k_ot_paint': VARIANTS})
