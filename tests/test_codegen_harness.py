"""CPU tier: the harness of the code-generation guards (tests/_codegen.py) on canned input: the remark
parser and `assert_clean` on two kernels' worth of remarks, and the flags read from csrc/Makefile.
Nothing compiles here."""
import pytest

import _codegen

# The first two kernels of a maxpool.hip compile, source snippet included as the compiler prints it;
# the second edited to 24 bytes of scratch and 3 + 5 spilled registers.
REMARKS = """\
maxpool.hip:126:1: remark: Function Name: _ZN4nmsa12_GLOBAL__N_18k_mp_fwdILi0ELi2EEEvPKNS_4elemIXT_EE4typeEPS4_PhNS0_6MpGeomE [-Rpass-analysis=kernel-resource-usage]
  126 | {
      | ^
maxpool.hip:126:1: remark:     TotalSGPRs: 49 [-Rpass-analysis=kernel-resource-usage]
maxpool.hip:126:1: remark:     VGPRs: 33 [-Rpass-analysis=kernel-resource-usage]
maxpool.hip:126:1: remark:     AGPRs: 0 [-Rpass-analysis=kernel-resource-usage]
maxpool.hip:126:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]
maxpool.hip:126:1: remark:     Dynamic Stack: False [-Rpass-analysis=kernel-resource-usage]
maxpool.hip:126:1: remark:     Occupancy [waves/SIMD]: 8 [-Rpass-analysis=kernel-resource-usage]
maxpool.hip:126:1: remark:     SGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
maxpool.hip:126:1: remark:     VGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
maxpool.hip:126:1: remark:     LDS Size [bytes/block]: 0 [-Rpass-analysis=kernel-resource-usage]
maxpool.hip:126:1: remark: Function Name: _ZN4nmsa12_GLOBAL__N_18k_mp_fwdILi0ELi1EEEvPKNS_4elemIXT_EE4typeEPS4_PhNS0_6MpGeomE [-Rpass-analysis=kernel-resource-usage]
maxpool.hip:126:1: remark:     TotalSGPRs: 54 [-Rpass-analysis=kernel-resource-usage]
maxpool.hip:126:1: remark:     VGPRs: 27 [-Rpass-analysis=kernel-resource-usage]
maxpool.hip:126:1: remark:     AGPRs: 0 [-Rpass-analysis=kernel-resource-usage]
maxpool.hip:126:1: remark:     ScratchSize [bytes/lane]: 24 [-Rpass-analysis=kernel-resource-usage]
maxpool.hip:126:1: remark:     Dynamic Stack: False [-Rpass-analysis=kernel-resource-usage]
maxpool.hip:126:1: remark:     Occupancy [waves/SIMD]: 8 [-Rpass-analysis=kernel-resource-usage]
maxpool.hip:126:1: remark:     SGPRs Spill: 3 [-Rpass-analysis=kernel-resource-usage]
maxpool.hip:126:1: remark:     VGPRs Spill: 5 [-Rpass-analysis=kernel-resource-usage]
maxpool.hip:126:1: remark:     LDS Size [bytes/block]: 0 [-Rpass-analysis=kernel-resource-usage]
"""
CLEAN = '_ZN4nmsa12_GLOBAL__N_18k_mp_fwdILi0ELi2EEEvPKNS_4elemIXT_EE4typeEPS4_PhNS0_6MpGeomE'
SPILLED = '_ZN4nmsa12_GLOBAL__N_18k_mp_fwdILi0ELi1EEEvPKNS_4elemIXT_EE4typeEPS4_PhNS0_6MpGeomE'

MAKEFILE_FLAGS = ['-O3', '-std=c++17', '--offload-arch=gfx950', '-fPIC', '-ffp-contract=off', '-Wall',
                  '-Wno-unused-function']
SURVEY_FLAGS = ['--offload-device-only', '-Rpass-analysis=kernel-resource-usage', '-c', '-o', '/dev/null']


def test_the_parser_reads_every_field_of_every_kernel():
    assert _codegen.parse_usage(REMARKS) == {
        CLEAN: {'vgpr': 33, 'agpr': 0, 'scratch': 0, 'sgpr_spill': 0, 'vgpr_spill': 0, 'occupancy': 8},
        SPILLED: {'vgpr': 27, 'agpr': 0, 'scratch': 24, 'sgpr_spill': 3, 'vgpr_spill': 5, 'occupancy': 8}}


def test_assert_clean_passes_on_the_clean_kernel():
    kernels = _codegen.parse_usage(REMARKS)
    clean = {CLEAN: kernels[CLEAN]}
    assert _codegen.assert_clean(clean) == clean
    assert _codegen.assert_clean(clean, {'k_mp_fwd': 1}, whole_file=True) == clean
    assert _codegen.assert_clean(kernels, {'ILi0ELi2E': 1}) == clean        # the spilled one is not selected


@pytest.mark.parametrize('field', ['scratch', 'sgpr_spill', 'vgpr_spill'])
def test_assert_clean_raises_on_each_nonzero_field(field):
    record = dict(_codegen.parse_usage(REMARKS)[CLEAN], **{field: 1})
    with pytest.raises(AssertionError, match=CLEAN):
        _codegen.assert_clean({CLEAN: record})


def test_assert_clean_raises_on_the_spilled_kernel_and_names_it():
    kernels = _codegen.parse_usage(REMARKS)
    for args in ((), ({'k_mp_fwd': 2},), ({'ILi0ELi1E': 1},)):
        with pytest.raises(AssertionError, match=SPILLED):
            _codegen.assert_clean(kernels, *args)


def test_assert_clean_raises_on_a_wrong_count_and_lists_the_kernels():
    clean = {CLEAN: _codegen.parse_usage(REMARKS)[CLEAN]}
    for stems in ({'k_mp_fwd': 2}, {'k_mp_fwd': 1, 'k_mp_bwd': 1}, {'k_mp_fwd': 0}):
        with pytest.raises(AssertionError, match=CLEAN):
            _codegen.assert_clean(clean, stems)


def test_assert_clean_raises_on_a_whole_file_total_off_by_one():
    kernels = _codegen.parse_usage(REMARKS)
    kernels[SPILLED] = kernels[CLEAN]
    assert _codegen.assert_clean(kernels, {'ILi0ELi2E': 1}) == {CLEAN: kernels[CLEAN]}
    with pytest.raises(AssertionError, match=SPILLED):
        _codegen.assert_clean(kernels, {'ILi0ELi2E': 1}, whole_file=True)


def test_the_flags_are_the_makefiles_and_the_surveys():
    assert _codegen.flags_for('maxpool.hip') == MAKEFILE_FLAGS + SURVEY_FLAGS
    assert _codegen.flags_for('losses_multi.hip') == MAKEFILE_FLAGS + ['-fno-slp-vectorize'] + SURVEY_FLAGS
    assert _codegen.flags_for('losses.hip') == MAKEFILE_FLAGS + SURVEY_FLAGS    # a stem is not a prefix
