"""CPU tier: code-generation guard for csrc/up_add.hip (the harness is tests/_codegen.py).  The kernel keeps a
rolling window of three input rows (up to 18 values on the half vector route), the sixteen pre-added weights of the
learned modes or the sixteen column weights of the bilinear mode and two output rows of up to eight pixels per lane,
all indexed by compile-time constants after unrolling: scratch or spilled registers would mean a window went to
memory."""
import pytest

import _codegen


@pytest.fixture(scope='module')
def usage():
    return _codegen.usage('up_add.hip')


def test_every_up_add_kernel_has_no_scratch_and_no_spills(usage):
    # 3 dtypes x (vector, one-pixel) x (nearest, bilinear, learned: both pad modes are one kernel)
    found = _codegen.assert_clean(usage, {'k_up_add': 18}, whole_file=True)
    # 256 lanes per workgroup, 8 workgroups per compute unit asked for: at most 128 registers keep 4 waves per SIMD
    assert max(v['vgpr'] for v in found.values()) <= 128, {k: v['vgpr'] for k, v in found.items()}
