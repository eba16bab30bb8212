"""CPU tier: code-generation guard for csrc/dve_project.hip, in the manner of tests/test_codegen.py
(hipcc cross-compiles without a GPU).  The MFMA kernel keeps 16*PT x 16*NT accumulators per wave in
registers; a spill to scratch would put them into the memory stream the kernel is bound by."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'nicr_mt_scene_analysis_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
FLAGS = ['-O3', '-std=c++17', '--offload-arch=gfx950', '-fPIC', '-ffp-contract=off', '-Wno-unused-function',
         '--offload-device-only', '-Rpass-analysis=kernel-resource-usage', '-c', '-o', os.devnull]
FIELDS = (('vgpr', r' VGPRs: (\d+)'), ('agpr', r' AGPRs: (\d+)'),
          ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'), ('sgpr_spill', r'SGPRs Spill: (\d+)'),
          ('vgpr_spill', r'VGPRs Spill: (\d+)'), ('occupancy', r'Occupancy \[waves/SIMD\]: (\d+)'))


@pytest.fixture(scope='module')
def usage():
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not available')
    out = subprocess.run([HIPCC, *FLAGS, 'dve_project.hip'], cwd=CSRC, capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r'remark:\s+Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        for key, pat in FIELDS:
            m = re.search(pat, line)
            if m and name:
                kernels[name][key] = int(m.group(1))
    return kernels


def test_tuned_kernel_has_no_scratch_and_no_spills(usage):
    tuned = {k: v for k, v in usage.items() if 'k_dve_project' in k}
    assert len(tuned) == 3, sorted(usage)          # <8,3>, <4,3>, <4,6>
    for k, v in tuned.items():
        assert v['scratch'] == 0 and v['sgpr_spill'] == 0 and v['vgpr_spill'] == 0, (k, v)
        assert v['occupancy'] >= 2, (k, v)         # two waves per SIMD keep the MFMA pipe fed
        # 16 pixels x 16 classes per tile, four accumulator registers each, nothing duplicated
        pt, nt = (int(n) for n in re.search(r'k_dve_projectILi(\d)ELi(\d)E', k).groups())
        assert v['agpr'] == 4 * pt * nt, (k, v)


def test_generic_kernel_has_no_scratch(usage):
    generic = [v for k, v in usage.items() if 'k_dve_generic' in k]
    assert len(generic) == 1 and generic[0]['scratch'] == 0, generic
