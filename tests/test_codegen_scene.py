"""CPU tier: code-generation guard for csrc/scene.hip, in the manner of
tests/test_codegen_augment.py (hipcc cross-compiles without a GPU).  The scene kernel keeps no
per-lane class array — a row is re-read for the maximum, the sum and the gradient — and its
float64 exponential and logarithm are inlined: scratch or spilled registers would mean one of
the two no longer holds."""
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
          ('vgpr_spill', r'VGPRs Spill: (\d+)'), ('vgprs', r' VGPRs: (\d+)'))


@pytest.fixture(scope='module')
def usage():
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not available')
    out = subprocess.run([HIPCC, *FLAGS, 'scene.hip'], cwd=CSRC, capture_output=True, text=True,
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


def test_scene_kernels_have_no_scratch_and_no_spills(usage):
    found = {k: v for k, v in usage.items() if 'k_scene_step' in k}
    assert len(found) == 3, sorted(usage)              # one per logits dtype: f32, bf16, f16
    for k, v in found.items():
        assert v['scratch'] == 0 and v['sgpr_spill'] == 0 and v['vgpr_spill'] == 0, (k, v)
        # 16 waves of one workgroup share a compute unit: 128 registers per lane at the most
        assert v['vgprs'] <= 128, (k, v)
