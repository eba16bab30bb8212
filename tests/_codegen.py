"""The code-generation harness of tests/test_codegen*.py: compile one csrc/*.hip file for the device
only, with the flags csrc/Makefile builds it with, and read LLVM's kernel-resource-usage remarks
(hipcc cross-compiles without a GPU).  `tools/isa_survey.sh` prints the same survey for people."""
import functools
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'nicr_mt_scene_analysis_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
SURVEY = ['--offload-device-only', '-Rpass-analysis=kernel-resource-usage', '-c', '-o', os.devnull]
FIELDS = (('vgpr', r' VGPRs: (\d+)'), ('agpr', r' AGPRs: (\d+)'),
          ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'), ('sgpr_spill', r'SGPRs Spill: (\d+)'),
          ('vgpr_spill', r'VGPRs Spill: (\d+)'), ('occupancy', r'Occupancy \[waves/SIMD\]: (\d+)'))


def flags_for(source):
    """the Makefile's HIPFLAGS for one source, its per-object additions included, plus the survey's"""
    with open(os.path.join(CSRC, 'Makefile')) as f:
        text = f.read()
    arch = re.search(r'^ARCH \?=\s*(\S+)', text, re.M).group(1)
    flags = re.search(r'^HIPFLAGS \?=\s*(.+)$', text, re.M).group(1).replace('$(ARCH)', arch).split()
    stem = re.escape(os.path.splitext(source)[0])
    for m in re.finditer(r'^%s\.o:\s*HIPFLAGS \+=\s*(.+)$' % stem, text, re.M):
        flags += m.group(1).split()
    return flags + SURVEY


def parse_usage(stderr_text):
    """{mangled kernel name: {'vgpr', 'agpr', 'scratch', 'sgpr_spill', 'vgpr_spill', 'occupancy'}}"""
    kernels, name = {}, None
    for line in stderr_text.splitlines():
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


@functools.lru_cache(maxsize=None)
def usage(source):
    """parse_usage of one source file, compiled once per session"""
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not available')
    out = subprocess.run([HIPCC, *flags_for(source), source], cwd=CSRC, capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    return parse_usage(out.stderr)


def usage_many(sources):
    """{source: usage(source)}, three compiles at a time"""
    with ThreadPoolExecutor(max_workers=3) as pool:
        return dict(zip(sources, pool.map(usage, sources)))


def assert_clean(kernels, stems=None, whole_file=False):
    """With stems = {substring: count}: exactly count kernels contain each substring (and, with
    whole_file, the file holds no others).  The kernels so selected (all of them without stems or with
    whole_file) have no scratch and no spilled registers; they are returned for further bounds."""
    found = kernels
    if stems is not None:
        count = {stem: sum(stem in k for k in kernels) for stem in stems}
        assert count == dict(stems), sorted(kernels)
        if whole_file:
            assert len(kernels) == sum(stems.values()), sorted(kernels)
        else:
            found = {k: v for k, v in kernels.items() if any(stem in k for stem in stems)}
    for k, v in found.items():
        assert v['scratch'] == 0 and v['sgpr_spill'] == 0 and v['vgpr_spill'] == 0, (k, v)
    return found
