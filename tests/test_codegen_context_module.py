"""CPU tier: code-generation guard for csrc/context_module.hip (the harness is tests/_codegen.py).
The kernels carry the per-branch sizes and pointers in a by-value argument struct and walk it with
fully unrolled loops: scratch or spilled registers would mean the struct (or a lane's per-branch
column ranges) went to memory."""
import pytest

import _codegen


@pytest.fixture(scope='module')
def usage():
    return _codegen.usage('context_module.hip')


def test_every_context_module_kernel_has_no_scratch_and_no_spills(usage):
    # 3 dtypes x (LDS, GLOBAL) of the two plane-reducing kernels, 3 dtypes of the other two
    stems = {'k_ppm_pool_fwd': 6, 'k_ppm_pool_bwd': 3, 'k_ppm_upcat_fwd': 3, 'k_ppm_upcat_bwd': 6}
    _codegen.assert_clean(usage, stems, whole_file=True)
