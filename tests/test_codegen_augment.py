"""CPU tier: code-generation guard for csrc/augment.hip (the harness is tests/_codegen.py).  The
augmentation kernel keeps its descriptor in scalar registers and at most the 12 source elements of
four pixels per lane: scratch or spilled registers would mean the pixel array, indexed by the flip,
went to memory."""
import pytest

import _codegen


@pytest.fixture(scope='module')
def usage():
    return _codegen.usage('augment.hip')


def test_augment_kernel_has_no_scratch_and_no_spills(usage):
    _codegen.assert_clean(usage, {'k_batch_augment': 1})    # one kernel for every mode and element size
