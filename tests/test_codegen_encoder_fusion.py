"""CPU tier: code-generation guard for csrc/encoder_fusion.hip (the harness is tests/_codegen.py).
The reduction kernels keep up to sixteen partial sums and two chunks of eight values per lane, the
excite kernels carry eight parameter pointers in a by-value argument struct: scratch or spilled
registers would mean one of them went to memory."""
import pytest

import _codegen


@pytest.fixture(scope='module')
def usage():
    return _codegen.usage('encoder_fusion.hip')


def test_every_encoder_fusion_kernel_has_no_scratch_and_no_spills(usage):
    # squeeze, weight gradient: 3 dtypes x (VECTOR, ELEMENT) x (WAVE, BLOCK); scale-add, apply: 3 dtypes x
    # (VECTOR, ELEMENT); the excite kernels: ReLU, SiLU
    stems = {'k_sefuse_squeeze': 12, 'k_sefuse_wgrad': 12, 'k_sefuse_scale_add': 6, 'k_sefuse_apply': 6,
             'k_sefuse_exciteI': 2, 'k_sefuse_excite_bwd': 2}
    _codegen.assert_clean(usage, stems, whole_file=True)
