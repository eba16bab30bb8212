"""CPU tier: code-generation guard for csrc/dve_project.hip (the harness is tests/_codegen.py).  The
MFMA kernel keeps 16*PT x 16*NT accumulators per wave in registers; a spill to scratch would put
them into the memory stream the kernel is bound by."""
import re

import pytest

import _codegen


@pytest.fixture(scope='module')
def usage():
    return _codegen.usage('dve_project.hip')


def test_tuned_kernel_has_no_scratch_and_no_spills(usage):
    tuned = _codegen.assert_clean(usage, {'k_dve_project': 3})     # <8,3>, <4,3>, <4,6>
    for k, v in tuned.items():
        assert v['occupancy'] >= 2, (k, v)         # two waves per SIMD keep the MFMA pipe fed
        # 16 pixels x 16 classes per tile, four accumulator registers each, nothing duplicated
        pt, nt = (int(n) for n in re.search(r'k_dve_projectILi(\d)ELi(\d)E', k).groups())
        assert v['agpr'] == 4 * pt * nt, (k, v)


def test_generic_kernel_has_no_scratch(usage):
    generic = [v for k, v in usage.items() if 'k_dve_generic' in k]
    assert len(generic) == 1 and generic[0]['scratch'] == 0, generic
