"""CPU tier: code-generation guard for csrc/maae.hip (the harness is tests/_codegen.py).  Both
kernels are one latency-bound workgroup; the matched one keeps its table descriptors in LDS so that
nothing spills."""
import pytest

import _codegen


@pytest.fixture(scope='module')
def usage():
    return _codegen.usage('maae.hip')


def test_the_file_holds_exactly_the_two_kernels(usage):
    assert len(usage) == 2, sorted(usage)


@pytest.mark.parametrize('kernel', ['k_maae_keyed', 'k_maae_matched'])
def test_kernels_have_no_scratch_and_no_spills(usage, kernel):
    _codegen.assert_clean(usage, {kernel: 1})               # one instantiation each
