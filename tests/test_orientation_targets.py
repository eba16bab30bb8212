"""`OrientationTargetGenerator` / `ops.orientation_targets` / `nmsa_orientation_targets` against
tests/golden/orientation_targets.npz (tools/gen_golden_orientation_targets.py: the reference's own
generator per sample on CPU) and against a numpy restatement of its rule written here.

Everything is exact: foreground, the `orientations_present` dicts (key order included), and the
orientation image bit for bit (`.view(np.uint32)`) against biternions computed in the test process
with the reference's expression `np.array([np.cos(rad), np.sin(rad)], dtype='float32')`.  Against
the RECORDED image the comparison is within one float32 ulp: numpy's float64 cos / sin on another
machine may differ in the last bit before the rounding to float32.
"""
import itertools

import numpy as np
import pytest
import torch

from _golden import load, jload
from _gpu_support import dev
from _orientation_ref import (assert_bits_equal, pack_keys, paint_present, random_angles, restate,
                              ulp_distance)
from nicr_mt_scene_analysis_amd.testing import synthetic as syn

CASES = ('ragged__list', 'ragged__none', 'wire__list', 'wire__none')
_CACHE = {}


def _case(name):
    """regenerated inputs (digest-checked: a mismatch FAILS) and the recorded reference results"""
    if name not in _CACHE:
        g = load('orientation_targets')
        p = jload(g[f'{name}__params'])
        inp = syn.make_orientation_inputs(p['recipe'], p['seed'])
        pairs = [[[int(k), float(v)] for k, v in d.items()] for d in inp['orientations']]
        stored = jload(g[f'{name}__orientations'])
        assert pairs == stored, f'{name}: regenerated angle dicts differ'
        digest = syn.input_digest(inp['semantic'], inp['instance'], inp['estimate'],
                                  np.frombuffer(__import__('json').dumps(pairs).encode(), dtype=np.uint8))
        assert digest == p['digest'], f'{name}: regenerated inputs differ from the fixture generator\'s'
        B, H, W = inp['semantic'].shape
        want = {
            'orientation': np.ascontiguousarray(g[f'{name}__orientation'].transpose(0, 3, 1, 2)),
            'foreground': np.unpackbits(g[f'{name}__foreground'])[:B * H * W].reshape(B, H, W).astype(bool),
            'present': [{int(k): float(v) for k, v in img} for img in jload(g[f'{name}__present'])],
        }
        _CACHE[name] = (inp, inp['estimate'] if p['with_class_list'] else None, want)
    return _CACHE[name]


def check_against_fixture(name, ori, fg, present, inp, want):
    assert (fg == want['foreground']).all(), name
    assert [list(p.items()) for p in present] == [list(p.items()) for p in want['present']], name
    assert_bits_equal(ori, paint_present(inp['instance'], want['present']), name)
    assert ulp_distance(ori, want['orientation']).max() <= 1, name


def run_ops(sem_t, ins_t, n_classes, estimate, orientations, max_instances=1024):
    from nicr_mt_scene_analysis_amd import ops
    keys, n_keys, bit = pack_keys(orientations)
    est = None if estimate is None else dev(estimate.astype(np.uint8))
    r = ops.orientation_targets(sem_t, ins_t, n_classes, est, dev(keys), dev(n_keys), dev(bit),
                                max_instances=max_instances)
    torch.cuda.synchronize()
    return r, keys


def check_ops(r, keys, sem, ins, orientations, estimate, what):
    ori, fg, present = restate(sem, ins, orientations, estimate)
    assert int(r['status'].item()) == 0, (what, int(r['status'].item()))
    assert r['foreground'].dtype == torch.bool and r['orientation'].dtype == torch.float32
    assert (r['foreground'].cpu().numpy() == fg).all(), what
    assert_bits_equal(r['orientation'].cpu().numpy(), ori, what)
    flags = np.array([[int(k) in present[b] for k in keys[b]] for b in range(len(present))], np.uint8)
    assert (r['present'].cpu().numpy() == flags).all(), what


# ---------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize('name', CASES)
def test_restatement_reproduces_the_fixture(name):
    inp, estimate, want = _case(name)
    ori, fg, present = restate(inp['semantic'], inp['instance'], inp['orientations'], estimate)
    check_against_fixture(name, ori, fg, present, inp, want)


def test_np_rad2biternion_is_the_reference_expression():
    from nicr_mt_scene_analysis_amd.utils import np_rad2biternion
    for rad in (0.0, np.pi, -1.25, 7.0, np.float32(0.3)):
        got = np_rad2biternion(rad)
        assert got.dtype == np.float32 and got.shape == (2,)
        assert_bits_equal(got, np.array([np.cos(rad), np.sin(rad)], dtype='float32'), rad)


# ---------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_class_against_the_fixture(name):
    from nicr_mt_scene_analysis_amd.data.preprocessing import OrientationTargetGenerator
    inp, estimate, want = _case(name)
    B, H, W = inp['semantic'].shape
    batch = {'semantic': dev(inp['semantic']), 'instance': dev(inp['instance']),
             'orientations': [dict(d) for d in inp['orientations']]}
    # blocks of the output sizes, poisoned and handed back to the allocator: the outputs are
    # torch.empty, so a byte the call does not write shows up
    poison = [torch.full((B, 2, H, W), float('nan'), device='cuda'),
              torch.full((B, H, W), 0xFF, dtype=torch.uint8, device='cuda'),
              torch.full((B, 64), 0xFF, dtype=torch.uint8, device='cuda')]
    torch.cuda.synchronize()
    del poison
    gen = OrientationTargetGenerator(None if estimate is None else tuple(bool(f) for f in estimate))
    out = gen(batch, n_classes=len(inp['estimate']))
    assert out is batch
    assert out['orientation_foreground'].dtype == torch.bool
    assert out['orientation'].dtype == torch.float32 and tuple(out['orientation'].shape) == (B, 2, H, W)
    check_against_fixture(name, out['orientation'].cpu().numpy(), out['orientation_foreground'].cpu().numpy(),
                          out['orientations_present'], inp, want)
    for b, p in enumerate(out['orientations_present']):
        assert all(v is batch['orientations'][b][k] for k, v in p.items())      # the caller's objects


@pytest.mark.gpu
@pytest.mark.parametrize('with_list', [True, False])
def test_ops_more_than_1024_ids(with_list):
    """3000 small ellipses: more than 1024 distinct ids survive, so max_instances = 1024 reports
    status bit 1 and 4096 is clean; the class grows by itself"""
    from nicr_mt_scene_analysis_amd.data.preprocessing import OrientationTargetGenerator
    NC = 151
    maps = syn.make_label_maps(1, NC, 192, 256, n_instances=3000, seed=61, max_radius=5)
    sem, ins = maps['semantic'], maps['instance']
    assert len(np.unique(ins)) - 1 > 1024
    orientations = random_angles(ins, np.random.default_rng(62))
    estimate = (np.arange(NC) % 2 == 1) if with_list else None
    r, _ = run_ops(dev(sem), dev(ins), NC, estimate, orientations, max_instances=1024)
    assert int(r['status'].item()) & 1
    r, keys = run_ops(dev(sem), dev(ins), NC, estimate, orientations, max_instances=4096)
    check_ops(r, keys, sem, ins, orientations, estimate, 'max_instances=4096')
    gen = OrientationTargetGenerator(None if estimate is None else tuple(estimate.tolist()), max_instances=1024)
    out = gen({'semantic': dev(sem), 'instance': dev(ins), 'orientations': orientations}, n_classes=NC)
    assert gen._max_instances == 4096
    ori, fg, present = restate(sem, ins, orientations, estimate)
    assert (out['orientation_foreground'].cpu().numpy() == fg).all()
    assert_bits_equal(out['orientation'].cpu().numpy(), ori, 'class')
    assert [list(p.items()) for p in out['orientations_present']] == [list(p.items()) for p in present]


@pytest.mark.gpu
@pytest.mark.parametrize('layout', ['misaligned', 'int64'])
def test_ops_generic_layouts(layout):
    """W % 4 == 0 but the rows are not 16-byte aligned (a view offset by one element); a uint8
    semantic map with an int64 instance map"""
    NC, B, H, W = 9, 2, 32, 64
    maps = syn.make_label_maps(B, NC, H, W, n_instances=9, seed=63)
    sem, ins = maps['semantic'], maps['instance']
    orientations = random_angles(ins, np.random.default_rng(64))
    estimate = np.arange(NC) % 2 == 1
    if layout == 'misaligned':
        sem_t = torch.zeros((B * H * W + 1,), dtype=torch.uint8, device='cuda')[1:].view(B, H, W)
        ins_t = torch.zeros((B * H * W + 1,), dtype=torch.int32, device='cuda')[1:].view(B, H, W)
        sem_t.copy_(dev(sem))
        ins_t.copy_(dev(ins))
        assert ins_t.data_ptr() % 16 != 0 and ins_t.is_contiguous()
    else:
        sem_t, ins_t = dev(sem), dev(ins.astype(np.int64))
    for est in (estimate, None):
        r, keys = run_ops(sem_t, ins_t, NC, est, orientations)
        check_ops(r, keys, sem, ins, orientations, est, (layout, est is None))


@pytest.mark.gpu
def test_errors_and_passthrough():
    from nicr_mt_scene_analysis_amd.data.preprocessing import OrientationTargetGenerator
    NC, B, H, W = 9, 2, 32, 64
    maps = syn.make_label_maps(B, NC, H, W, n_instances=9, seed=65)
    sem, ins = maps['semantic'], maps['instance']
    orientations = random_angles(ins, np.random.default_rng(66))
    gen = OrientationTargetGenerator(tuple((np.arange(NC) % 2 == 1).tolist()))
    bad_sem = sem.copy()
    y, x = np.argwhere(ins[1] > 0)[0]                 # (labels are checked on instance pixels)
    bad_sem[1, y, x] = NC
    with pytest.raises(ValueError, match='semantic labels'):
        gen({'semantic': dev(bad_sem), 'instance': dev(ins), 'orientations': orientations})
    bad_ins = ins.copy()
    bad_ins[0, 3, 3] = -1
    with pytest.raises(ValueError, match='instance ids'):
        gen({'semantic': dev(sem), 'instance': dev(bad_ins), 'orientations': orientations})
    batch = {'semantic': dev(sem), 'instance': dev(ins)}
    entries = dict(batch)
    assert gen(batch) is batch
    assert set(batch) == set(entries) and all(batch[k] is v for k, v in entries.items())


@pytest.mark.gpu
def test_shared_workspace_in_every_order():
    """instance, orientation and panoptic targets on one on-wire batch share the cached workspace:
    the six orders, twice each, every result equal to what the same call gives first after the
    cached workspaces were dropped"""
    from nicr_mt_scene_analysis_amd import ops
    NC, B, H, W, sigma = 9, 2, 48, 64, 3
    maps = syn.make_label_maps(B, NC, H, W, n_instances=10, seed=67)
    sem, ins, is_thing = maps['semantic'], maps['instance'], maps['semantic_classes_is_thing']
    stuff = np.zeros((NC,), np.uint8)
    stuff[np.where(~is_thing)[0][1:]] = 1
    orientations = random_angles(ins, np.random.default_rng(68))
    keys, n_keys, bit = pack_keys(orientations)
    d = dict(sem=dev(sem), ins=dev(ins), th=dev(is_thing.astype(np.uint8)), st=dev(stuff),
             est=dev((np.arange(NC) % 2 == 1).astype(np.uint8)), keys=dev(keys), n_keys=dev(n_keys), bit=dev(bit))

    def instance():
        r = ops.instance_targets(d['sem'], d['ins'], NC, d['th'], d['st'], sigma, True, max_instances=64)
        n = r['n_encoded'].cpu()
        return [r['center'], r['offset'], r['foreground'], r['center_mask'], r['n_encoded'], r['status']] + \
            [r['encoded_ids'][b, :int(n[b])] for b in range(B)]

    def orientation():
        r = ops.orientation_targets(d['sem'], d['ins'], NC, d['est'], d['keys'], d['n_keys'], d['bit'],
                                    max_instances=64)
        return [r['orientation'], r['foreground'], r['present'], r['status']]

    def panoptic():
        r = ops.panoptic_targets(d['sem'], d['ins'], NC, d['th'], 1 << 16, 0, max_instances=64)
        n = r['n_ids'].cpu()
        return [r['panoptic'], r['n_ids'], r['status']] + \
            [r[k][b, :int(n[b])] for b in range(B) for k in ('ids_pan', 'ids_ins')]

    calls = {'instance': instance, 'orientation': orientation, 'panoptic': panoptic}
    first = {}
    for name, fn in calls.items():
        ops._TARGET_WORKSPACES.clear()
        first[name] = [t.clone() for t in fn()]
    ori, fg, _ = restate(sem, ins, orientations, np.arange(NC) % 2 == 1)
    assert_bits_equal(first['orientation'][0].cpu().numpy(), ori, 'first')
    assert (first['orientation'][1].cpu().numpy() == fg).all() and fg.any()
    for order in itertools.permutations(calls):
        ops._TARGET_WORKSPACES.clear()
        for rep in range(2):
            for name in order:
                got = calls[name]()
                assert len(got) == len(first[name])
                for i, (a, b) in enumerate(zip(got, first[name])):
                    assert torch.equal(a, b), (order, rep, name, i)
        assert len(ops._TARGET_WORKSPACES) == 1


@pytest.mark.gpu
def test_graph_capture_and_replay():
    """captured on static input buffers; the second replay has other labels and another number of
    keys within the same K"""
    from nicr_mt_scene_analysis_amd import ops
    NC, B, H, W = 9, 2, 48, 64
    estimate = np.arange(NC) % 2 == 1
    batches = []
    for seed, n_inst in ((69, 6), (70, 14)):
        maps = syn.make_label_maps(B, NC, H, W, n_instances=n_inst, seed=seed)
        orientations = random_angles(maps['instance'], np.random.default_rng(seed + 100), fraction=0.8)
        batches.append((maps['semantic'], maps['instance'], orientations, pack_keys(orientations)))
    assert batches[0][3][0].shape == batches[1][3][0].shape == (B, 64)
    assert (batches[0][3][1] != batches[1][3][1]).any()
    s = dict(sem=torch.zeros((B, H, W), dtype=torch.uint8, device='cuda'),
             ins=torch.zeros((B, H, W), dtype=torch.int32, device='cuda'),
             keys=torch.zeros((B, 64), dtype=torch.int32, device='cuda'),
             n_keys=torch.zeros((B,), dtype=torch.int32, device='cuda'),
             bit=torch.zeros((B, 64, 2), dtype=torch.float32, device='cuda'),
             est=dev(estimate.astype(np.uint8)))

    def step():
        return ops.orientation_targets(s['sem'], s['ins'], NC, s['est'], s['keys'], s['n_keys'], s['bit'],
                                       max_instances=64)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    torch.cuda.synchronize()
    for i, (sem, ins, orientations, (keys, n_keys, bit)) in enumerate(batches):
        s['sem'].copy_(dev(sem))
        s['ins'].copy_(dev(ins))
        s['keys'].copy_(dev(keys))
        s['n_keys'].copy_(dev(n_keys))
        s['bit'].copy_(dev(bit))
        graph.replay()
        torch.cuda.synchronize()
        check_ops(out, keys, sem, ins, orientations, estimate, ('replay', i))
