"""CPU tier: code-generation guard for csrc/ln_transpose.hip, in the manner of
tests/test_codegen_upsampling.py (hipcc cross-compiles without a GPU).  The forward kernel holds a row
of up to 32 values per lane (and their squared deviations) for the two summation trees, the backward
kernel 16 row-sum partials per lane, all indexed by compile-time constants after unrolling: scratch
or spilled registers would mean a row went to memory."""
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
FIELDS = (('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'), ('sgpr_spill', r'SGPRs Spill: (\d+)'),
          ('vgpr_spill', r'VGPRs Spill: (\d+)'))


@pytest.fixture(scope='module')
def usage():
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not available')
    out = subprocess.run([HIPCC, *FLAGS, 'ln_transpose.hip'], cwd=CSRC, capture_output=True, text=True,
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


def test_every_fusion_kernel_has_no_scratch_and_no_spills(usage):
    # 5 dtype pairs x (vector, element) of the forward and of the backward kernel, and the reducer
    count = {stem: sum(stem in k for k in usage) for stem in ('k_lnt_fwd', 'k_lnt_bwd', 'k_lnt_reduce')}
    assert count == {'k_lnt_fwd': 10, 'k_lnt_bwd': 10, 'k_lnt_reduce': 1}, sorted(usage)
    assert len(usage) == 21, sorted(usage)
    for k, v in usage.items():
        assert v == {'scratch': 0, 'sgpr_spill': 0, 'vgpr_spill': 0}, (k, v)
