"""CPU tier: code-generation guard for csrc/scene_head.hip (the harness is tests/_codegen.py).  The forward
kernel keeps a chunk of up to eight elements and a lane sum per lane, the backward kernel a packed plane value:
scratch or spilled registers would mean one of them went to memory."""
import pytest

import _codegen


@pytest.fixture(scope='module')
def usage():
    return _codegen.usage('scene_head.hip')


def test_every_scene_head_kernel_has_no_scratch_and_no_spills(usage):
    # forward and backward: 3 dtypes x (UNIT, VECTOR, ELEMENT)
    _codegen.assert_clean(usage, {'k_sh_fwd': 9, 'k_sh_bwd': 9}, whole_file=True)
