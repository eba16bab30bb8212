"""CPU tier: code-generation guard for csrc/scene.hip (the harness is tests/_codegen.py).  The scene
kernel keeps no per-lane class array — a row is re-read for the maximum, the sum and the gradient —
and its float64 exponential and logarithm are inlined: scratch or spilled registers would mean one
of the two no longer holds."""
import pytest

import _codegen


@pytest.fixture(scope='module')
def usage():
    return _codegen.usage('scene.hip')


def test_scene_kernels_have_no_scratch_and_no_spills(usage):
    found = _codegen.assert_clean(usage, {'k_scene_step': 3})   # one per logits dtype: f32, bf16, f16
    for k, v in found.items():
        # 16 waves of one workgroup share a compute unit: 128 registers per lane at the most
        assert v['vgpr'] <= 128, (k, v)
