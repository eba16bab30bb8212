"""CPU tier: code-generation guard for csrc/block_tail.hip (the harness is tests/_codegen.py).  The statistics
kernel keeps the 32 values of a lane's share of a unit in registers between its two passes, the backward kernels
hold up to three chunks of eight values and two sets of partial sums per lane, and the apply kernels carry their
per-channel pointers in a by-value argument struct: scratch or spilled registers would mean one of them
went to memory."""
import pytest

import _codegen


@pytest.fixture(scope='module')
def usage():
    return _codegen.usage('block_tail.hip')


def test_every_block_tail_kernel_has_no_scratch_and_no_spills(usage):
    # statistics: 3 dtypes x (VECTOR, ELEMENT); apply and the two backward kernels: 3 dtypes x
    # (VECTOR, ELEMENT) x (ReLU, SiLU)
    stems = {'k_bntail_stats': 6, 'k_bntail_applyI': 12, 'k_bntail_bwd_reduce': 12, 'k_bntail_bwd_apply': 12}
    _codegen.assert_clean(usage, stems, whole_file=True)
