"""CPU tier: code-generation guard for csrc/mlp_decoder.hip (the harness is tests/_codegen.py).  The
kernels carry the per-branch channel counts, shifts and pointers in a by-value argument struct and
pick a branch with fully unrolled selects inside a grid-stride loop: scratch or spilled registers
would mean the struct (or a lane's vector of results) went to memory."""
import pytest

import _codegen


@pytest.fixture(scope='module')
def usage():
    return _codegen.usage('mlp_decoder.hip')


def test_every_mlp_decoder_kernel_has_no_scratch_and_no_spills(usage):
    # 3 dtypes x (VECTOR, ELEMENT) of the forward kernel, 3 dtypes of the backward kernel
    _codegen.assert_clean(usage, {'k_mlpdec_upcat_fwd': 6, 'k_mlpdec_upcat_bwd': 3}, whole_file=True)
