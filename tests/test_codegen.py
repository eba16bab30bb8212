"""CPU tier: code-generation guard for the hot kernels (hipcc cross-compiles without a GPU).

Round 4 found three kinds of silent regressions in the generated code, none of which changes a
result: register spills to scratch memory (100 B per lane were 8 % of the wide cross entropy's HBM
writes), hundreds of loop-invariant scalar plane offsets spilled to lane registers, and hash-probe
loops unrolled into 37 900 instructions.  This test compiles the three files that hold those
kernels with LLVM's resource-usage remarks and checks the hot instantiations.  (The harness is
tests/_codegen.py; `tools/isa_survey.sh` prints the same survey for every kernel of the library.)"""
import re

import pytest

import _codegen


@pytest.fixture(scope='module')
def usage():
    return _codegen.usage_many(('losses_split.hip', 'losses_cos.hip', 'metrics.hip'))


def test_wide_cross_entropy_has_no_scratch(usage):
    """every instantiation of k_ce_split (dtype x plane groups x smoothing x mode x row form)"""
    ks = {k: v for k, v in usage['losses_split.hip'].items() if 'k_ce_split' in k}
    assert len(ks) >= 48
    bad = {k: v for k, v in ks.items() if v['scratch'] != 0}
    assert not bad, bad
    # configs[4]: bf16, 150 classes (5 groups of 8 planes per wave), loss + gradient, 8-byte rows
    hot = [v for k, v in ks.items() if 'ILi1ELi5ELb0ELi0ELb1E' in k]
    assert len(hot) == 1 and hot[0]['occupancy'] >= 3 and hot[0]['sgpr_spill'] <= 16, hot


def test_cosine_kernels_keep_their_plane_offsets_out_of_lane_registers(usage):
    ks = usage['losses_cos.hip']
    split = {k: v for k, v in ks.items() if 'k_cos_split' in k}
    parts = {k: v for k, v in ks.items() if 'k_cos_parts' in k}
    assert split and parts
    for k, v in {**split, **parts}.items():
        # (the gradient-only instantiation — the recompute after a missed expectation — may keep a
        # few bytes: it sits at the 256-register limit)
        recompute = re.search(r'k_cos_(parts|split)ILi\dELi2E', k) is not None
        assert v['scratch'] <= (16 if recompute else 0), (k, v)
    for k, v in split.items():
        assert v['sgpr_spill'] <= 32, (k, v)                    # were 202-211: one base per plane
    # the non-ragged column kernels (the D % 64 == 0 instantiations: third template argument false)
    nonragged = {k: v for k, v in ks.items() if re.search(r'k_cos_partsILi\dELi\dELb0E', k)}
    assert len(nonragged) >= 6
    for k, v in nonragged.items():
        assert v['sgpr_spill'] <= 48, (k, v)                    # were 245-268


def test_pq_count_is_not_unrolled_into_its_probe_loops(usage):
    ks = {k: v for k, v in usage['metrics.hip'].items() if 'k_pq_count' in k}
    assert len(ks) == 5            # (with / without confusion matrix) x (pow2 / generic) on the map + k_pq_count_parts
    for k, v in ks.items():
        assert v['scratch'] == 0 and v['sgpr_spill'] <= 64, (k, v)   # the unrolled form: 4994-5467
