"""CPU tier: code-generation guard for csrc/augment_resize.hip (the harness is tests/_codegen.py).
The kernel keeps its descriptor in scalar registers and, per lane, the table entries and source
pixels of at most four output pixels — for rgb the four taps of each —: scratch or spilled registers
would mean those arrays went to memory."""
import pytest

import _codegen


@pytest.fixture(scope='module')
def usage():
    return _codegen.usage('augment_resize.hip')


def test_resize_kernel_has_no_scratch_and_no_spills(usage):
    found = _codegen.assert_clean(usage, {'k_batch_augment_resized': 1}, whole_file=True)
    (kernel,) = found.values()
    print('VGPRs', kernel['vgpr'], 'occupancy', kernel['occupancy'])
    # what DESIGN.md §4b records: 60 VGPRs, 8 waves per SIMD (64 VGPRs are the most that allow 8)
    assert kernel['agpr'] == 0 and kernel['vgpr'] <= 64 and kernel['occupancy'] >= 8
