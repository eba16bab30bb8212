"""Side-output targets on the device: `MultiscaleSupervisionGenerator` (one gather launch for all
keys and scales, `nmsa_multiscale_nearest`) and the multiscale behaviour of the target generators,
against tests/golden/multiscale_supervision.npz — the reference's own preprocessing chain run per
sample (tools/gen_golden_multiscale.py; its `cv2.resize` is a numpy stand-in written from
OpenCV's nearest rule, see the tool's docstring).

CPU tier: the index rule and the host logic.  GPU tier (`-m gpu`): resized keys bit-identical to
the fixture (raw bits: u8, bool, i16, i32, i64, f32 [B,3,H,W] with NaN payloads and -0.0), the
whole chain at the parity bar of target generation (bit-exact, the Gauss
heat-map within 1e-6), repeated / alternating shapes, hipGraph capture and replay, and a training
step of the task helpers on a batch the chain built.
"""
import functools

import numpy as np
import pytest
import torch

from _golden import jload, load
from nicr_mt_scene_analysis_amd.testing import synthetic as syn

CASES = ('A', 'B', 'C')


@functools.lru_cache(maxsize=None)
def case(name):
    """(params, regenerated inputs, fixture); the inputs are read-only for every test"""
    g = load('multiscale_supervision')
    p = jload(g[f'{name}__params'])
    inp = syn.make_multiscale_inputs(p['recipe'], p['seed'])
    assert syn.multiscale_input_digest(inp) == p['digest'], f'{name}: regenerated inputs differ'
    for v in inp.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p, inp, g


def shape_of(name):
    _, _, H, W = syn.MULTISCALE_RECIPES[name][:4]
    return H, W


# --------------------------------------------------------------------------------------- CPU tier
def test_fixture_cases_are_the_ones_asked_for():
    assert jload(load('multiscale_supervision')['names']) == list(CASES)
    want = {'A': (2, 58, 116, [4, 8]), 'B': (3, 50, 70, [8, 16, 32]), 'C': (1, 48, 64, [2, 4])}
    for name, (B, H, W, downscales) in want.items():
        p, inp, g = case(name)
        assert inp['semantic'].shape == (B, H, W) and p['downscales'] == downscales
    assert case('B')[2]['B__d32__msg__semantic'].shape == (3, 1, 2)


@pytest.mark.parametrize('name', CASES)
def test_nearest_map_equals_fixture_maps(name):
    from nicr_mt_scene_analysis_amd.data.preprocessing import cv2_nearest_map
    p, _, g = case(name)
    H, W = shape_of(name)
    for d in p['downscales']:
        rows, cols = cv2_nearest_map(H, int(H / d)), cv2_nearest_map(W, int(W / d))
        assert rows.dtype == np.int32 and cols.dtype == np.int32
        assert np.array_equal(rows, g[f'{name}__d{d}__rows']), d
        assert np.array_equal(cols, g[f'{name}__d{d}__cols']), d


def test_nearest_map_is_a_stride_when_the_downscale_divides_the_side():
    from nicr_mt_scene_analysis_amd.data.preprocessing import cv2_nearest_map
    for src in (1, 2, 48, 64, 96, 480, 640, 1024, 1920):
        for d in (1, 2, 3, 4, 5, 8, 16, 32, 64):
            if src % d == 0:
                assert np.array_equal(cv2_nearest_map(src, src // d), np.arange(src // d) * d), (src, d)


def test_nearest_map_pinned_deviations_from_integer_arithmetic():
    from nicr_mt_scene_analysis_amd.data.preprocessing import cv2_nearest_map
    assert int(116 / 8) == 14 and int(58 / 4) == 14
    assert cv2_nearest_map(116, 14)[7] == 57 and 7 * 116 // 14 == 58
    assert cv2_nearest_map(58, 14)[7] == 28 and 7 * 58 // 14 == 29
    for src, dst in ((116, 14), (58, 14), (70, 8), (50, 6), (7, 3), (5, 5), (3, 1)):
        m = cv2_nearest_map(src, dst)
        assert m.shape == (dst,) and m.min() >= 0 and m.max() < src and (np.diff(m) >= 0).all()
    with pytest.raises(ValueError):
        cv2_nearest_map(4, 0)


def test_generator_error_paths():
    from nicr_mt_scene_analysis_amd import ops
    from nicr_mt_scene_analysis_amd._lib import NmsaError
    from nicr_mt_scene_analysis_amd.data.preprocessing import (InstanceTargetGenerator,
                                                               MultiscaleSupervisionGenerator)
    gen = MultiscaleSupervisionGenerator(downscales=(4, 8), keys=('semantic', 'scene'))
    assert gen.downscales == (4, 8)
    with pytest.raises(KeyError, match='missing'):
        gen({'semantic': torch.zeros((1, 8, 8), dtype=torch.uint8)})
    with pytest.raises(NotImplementedError, match='INTER_LINEAR'):
        MultiscaleSupervisionGenerator((2,), ('rgb', 'scene'))(
            {'rgb': torch.zeros((1, 3, 8, 8)), 'scene': torch.zeros((1,))})
    # an empty scale: int(8 / 16) == 0 (the reference would hand cv2 an empty size)
    with pytest.raises(ValueError, match='empty'):
        ops.multiscale_nearest({}, (2, 16), (8, 32))
    with pytest.raises(ValueError, match='empty'):
        MultiscaleSupervisionGenerator((16,), ('scene',))(
            {'depth': torch.zeros((1, 8, 32)), 'scene': torch.zeros((1,))})
    # host tensors are rejected, not resized some other way
    with pytest.raises(NmsaError):
        ops.multiscale_nearest({'semantic': torch.zeros((1, 8, 8), dtype=torch.uint8)}, (2,), (8, 8))
    # a downscale without a sigma: the reference's KeyError
    igen = InstanceTargetGenerator(sigma=4, sigma_for_additional_downscales={4: 2})
    with pytest.raises(KeyError):
        igen({'_down_8': {'instance': torch.zeros((1, 2, 2), dtype=torch.int32)}})


def test_entries_that_are_not_spatial_are_deep_copied():
    from nicr_mt_scene_analysis_amd.data.preprocessing import (MultiscaleSupervisionGenerator,
                                                               get_downscale)
    batch = {'depth': torch.zeros((2, 58, 116)), 'orientations': [{3: 0.5}, {}],
             'scene': torch.tensor([4, 1]), 'luts': [torch.ones((2, 3)), torch.ones((1, 3))]}
    gen = MultiscaleSupervisionGenerator((4, 8), ('orientations', 'scene', 'luts'))
    assert gen(batch) is batch
    assert gen.last_dynamic_parameters == {'shapes': {4: (14, 29), 8: (7, 14)}}
    for d in (4, 8):
        sub = get_downscale(batch, d)
        assert list(sub) == ['orientations', 'scene', 'luts']
        assert sub['orientations'] == batch['orientations'] and sub['orientations'] is not batch['orientations']
        assert sub['orientations'][0] is not batch['orientations'][0]
        assert torch.equal(sub['scene'], batch['scene']) and sub['scene'].data_ptr() != batch['scene'].data_ptr()
        assert all(torch.equal(a, b) and a is not b for a, b in zip(sub['luts'], batch['luts']))


def test_multiscale_call_leaves_a_sub_batch_without_inputs_untouched():
    from nicr_mt_scene_analysis_amd.data import preprocessing as pre
    flags = (False, True, True)
    gens = (pre.InstanceClearStuffIDs(flags), pre.InstanceTargetGenerator(2, flags, sigma_for_additional_downscales={4: 1}),
            pre.OrientationTargetGenerator(flags), pre.PanopticTargetGenerator(flags),
            pre.DenseVisualEmbeddingTargetGenerator())
    for gen in gens:
        scene = torch.tensor([1])
        sub = {'scene': scene}
        batch = {'scene': scene, '_down_4': sub}
        assert gen(batch) is batch and batch['_down_4'] is sub
        assert list(batch) == ['scene', '_down_4'] and list(sub) == ['scene'] and sub['scene'] is scene
    # off unless sigmas for the downscales are given: the sub-batch is not even looked at
    off = pre.InstanceTargetGenerator(2, flags)
    batch = {'_down_4': {'instance': 'not a tensor'}}
    assert off(batch) is batch


def test_entry_point_checks_the_table_before_anything_is_enqueued():
    """every field and map entry is checked on the host copy first: a bad table is NMSA_ERR_ARG
    (-1) without a device (nothing below reaches a HIP call)"""
    import ctypes as C
    from nicr_mt_scene_analysis_amd import _lib as L
    from nicr_mt_scene_analysis_amd.data.preprocessing import cv2_nearest_map
    rows, cols = cv2_nearest_map(58, 14), cv2_nearest_map(116, 14)
    good = np.zeros((16 + 28,), np.int32)
    good[:4].view(np.uint64)[:] = (0x1000, 0x2000)             # never dereferenced by the checks
    good[4:12] = (2, 58, 116, 14, 14, 2, 0, 14)
    good[16:30], good[30:] = rows, cols
    fn = L.lib().nmsa_multiscale_nearest

    def rc(words, n_desc=1, n_words=None, device=0x3000):
        buf = np.ascontiguousarray(words)
        return fn(C.c_void_p(buf.ctypes.data), C.c_void_p(device), n_desc,
                  len(buf) if n_words is None else n_words, None)

    def broken(at, value):
        bad = good.copy()
        bad[at] = value
        return bad

    assert rc(good, n_desc=0) == -1 and rc(good, n_desc=1025) == -1 and rc(good, device=0) == -1
    assert rc(good, n_words=15) == -1
    for at, value in ((4, 0), (5, -1), (7, 0), (9, 4), (9, -1), (10, -1), (10, 15), (11, 15),
                      (16 + 13, 58), (16 + 3, -1), (30 + 13, 116), (0, 0), (2, 0), (2, 0x2002)):
        assert rc(broken(at, value)) == -1, (at, value)
    assert rc(broken(4, 1 << 30)) == -1                        # planes * h * w above 2^31 - 1


# --------------------------------------------------------------------------------------- GPU tier
def device_batch(inp):
    """the collated device batch: on-wire dtypes, `segment_ids` as int64"""
    batch = {k: torch.from_numpy(np.array(inp[k])).cuda() for k in
             ('semantic', 'instance', 'depth', 'normal', 'valid', 'scene')}
    batch['segment_ids'] = torch.from_numpy(inp['segment_ids'].astype(np.int64)).cuda()
    batch['orientations'] = [dict(d) for d in inp['orientations']]
    return batch


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def as_device_dtype(key, golden):
    """fixture array in the dtype the device batch holds the key in (equal values)"""
    return golden.astype({'instance': np.int32, 'segment_ids': np.int64, 'panoptic': np.int64}.get(key, golden.dtype))


def check_resized(name, batch, what):
    p, inp, g = case(name)
    dtypes = {'semantic': torch.uint8, 'instance': torch.int32, 'depth': torch.int16, 'normal': torch.float32,
              'valid': torch.bool, 'segment_ids': torch.int64}
    for d in p['downscales']:
        sub = batch[f'_down_{d}']
        for k in syn.MULTISCALE_SPATIAL_KEYS:
            want = as_device_dtype(k, g[f'{name}__d{d}__msg__{k}'])
            got = sub[k]
            assert got.dtype == dtypes[k] and got.is_contiguous() and tuple(got.shape) == want.shape, (what, d, k)
            assert np.array_equal(raw(got.cpu().numpy()), raw(want)), (what, d, k)


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_resized_keys_are_bit_identical_to_the_reference(name):
    from nicr_mt_scene_analysis_amd.data.preprocessing import MultiscaleSupervisionGenerator
    p, inp, g = case(name)
    H, W = shape_of(name)
    batch = device_batch(inp)
    before = {k: v.clone() for k, v in batch.items() if isinstance(v, torch.Tensor)}
    gen = MultiscaleSupervisionGenerator(tuple(p['downscales']), syn.MULTISCALE_KEYS)
    assert gen(batch) is batch
    check_resized(name, batch, 'first call')
    assert gen.last_dynamic_parameters == {'shapes': {d: (int(H / d), int(W / d)) for d in p['downscales']}}
    for k, v in before.items():                                # the main scale is only read
        assert torch.equal(batch[k].view(torch.uint8), v.view(torch.uint8)), k
    for d in p['downscales']:
        sub = batch[f'_down_{d}']
        assert list(sub) == list(syn.MULTISCALE_KEYS)
        copied = jload(g[f'{name}__d{d}__copied'])
        assert [[[k, v] for k, v in o.items()] for o in sub['orientations']] == copied['orientations']
        assert sub['orientations'] is not batch['orientations']
        assert sub['scene'].cpu().tolist() == copied['scene']
        assert sub['scene'].data_ptr() != batch['scene'].data_ptr()
        bits = sub['normal'].cpu().numpy().view(np.uint32)
        if bits.size > 40:          # NaN payloads and -0.0 made it through (compared as bits above)
            assert (bits == 0xffc00001).any() and (bits == 0x7f800123).any() and (bits == 0x80000000).any()


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_generator_chain_matches_the_reference_at_every_scale(name):
    from nicr_mt_scene_analysis_amd.data import preprocessing as pre
    p, inp, g = case(name)
    is_thing = tuple(bool(f) for f in inp['semantic_classes_is_thing'])
    estimate = tuple(bool(f) for f in inp['estimate'])
    sigma_down = {d: s for d, s in p['sigma_for_additional_downscales']}

    def generators():
        return (pre.InstanceClearStuffIDs(semantic_classes_is_thing=is_thing),
                pre.InstanceTargetGenerator(sigma=p['sigma'], semantic_classes_is_thing=is_thing,
                                            sigma_for_additional_downscales=sigma_down),
                pre.OrientationTargetGenerator(semantic_classes_estimate_orientation=estimate),
                pre.PanopticTargetGenerator(semantic_classes_is_thing=is_thing))

    batch = device_batch(inp)
    batch = pre.MultiscaleSupervisionGenerator(tuple(p['downscales']), syn.MULTISCALE_KEYS)(batch)
    chain = generators()
    for gen in chain:
        batch = gen(batch)
    for d in p['downscales']:
        sub, pfx = batch[f'_down_{d}'], f'{name}__d{d}__'
        for k in ('instance', 'instance_offset', 'instance_foreground', 'instance_center_mask',
                  'orientation', 'orientation_foreground', 'panoptic'):
            want = as_device_dtype(k, g[pfx + k])
            got = sub[k].cpu().numpy()
            assert got.dtype == want.dtype and got.shape == want.shape, (d, k)
            assert np.array_equal(raw(got), raw(want)), (d, k)
        center = sub['instance_center'].cpu().numpy()
        assert center.dtype == np.float32
        np.testing.assert_allclose(center, g[pfx + 'instance_center'], rtol=0, atol=1e-6, err_msg=f'{d}')
        dicts = jload(g[pfx + 'dicts'])
        assert [[[k, v] for k, v in o.items()] for o in sub['orientations_present']] == dicts['orientations_present']
        assert [[[int(k), int(v)] for k, v in o.items()] for o in sub['panoptic_ids_to_instance_dict']] == \
            dicts['panoptic_ids_to_instance_dict']
        assert chain[1].last_dynamic_parameters[f'_down_{d}']['encoded_instances'] == dicts['encoded_instances']
    # the main scale is what a batch without side-output entries gets
    plain = device_batch(inp)
    for gen in generators():
        plain = gen(plain)
    assert not any(k.startswith('_down_') for k in plain)
    for k in ('instance', 'instance_center', 'instance_offset', 'instance_foreground', 'instance_center_mask',
              'orientation', 'orientation_foreground', 'panoptic'):
        assert torch.equal(plain[k], batch[k]), k
    assert plain['orientations_present'] == batch['orientations_present']
    assert plain['panoptic_ids_to_instance_dict'] == batch['panoptic_ids_to_instance_dict']


@pytest.mark.gpu
def test_repeated_and_alternating_shapes_and_graph_replay():
    from nicr_mt_scene_analysis_amd.data.preprocessing import MultiscaleSupervisionGenerator
    gens = {n: MultiscaleSupervisionGenerator(tuple(case(n)[0]['downscales']), syn.MULTISCALE_KEYS) for n in 'AB'}
    # the same shapes twice, then different shapes in turn: every call as good as the first
    for turn, name in enumerate('AABAB'):
        batch = gens[name](device_batch(case(name)[1]))
        check_resized(name, batch, f'call {turn}')
    # capture and replay (the generator alone: one copy node + one kernel node, no host sync)
    p, inp, g = case('A')
    static = device_batch(inp)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gens['A'](static)
    captured = {d: dict(static[f'_down_{d}']) for d in p['downscales']}
    # an eager call with the same shapes between capture and replay must not disturb the graph
    eager = gens['A'](device_batch(inp))
    check_resized('A', eager, 'eager after capture')
    graph.replay()
    torch.cuda.synchronize()
    check_resized('A', static, 'replay')
    # new contents in the captured inputs: the replay gathers them, as an eager call does
    for k in syn.MULTISCALE_SPATIAL_KEYS:
        static[k].copy_(static[k].flip(-1).flip(-2))
    graph.replay()
    flipped = gens['A']({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in static.items()
                         if not k.startswith('_down_')})
    torch.cuda.synchronize()
    for d in p['downscales']:
        for k in syn.MULTISCALE_SPATIAL_KEYS:
            assert torch.equal(captured[d][k].view(torch.uint8), flipped[f'_down_{d}'][k].view(torch.uint8)), (d, k)
            assert not torch.equal(captured[d][k].view(torch.uint8), eager[f'_down_{d}'][k].view(torch.uint8)), (d, k)


@pytest.mark.gpu
def test_training_step_on_a_batch_built_by_the_chain():
    from nicr_mt_scene_analysis_amd.data import preprocessing as pre
    from nicr_mt_scene_analysis_amd.task_helper import InstanceTaskHelper, SemanticTaskHelper
    p, inp, g = case('A')
    B, C, H, W = syn.MULTISCALE_RECIPES['A'][:4]
    is_thing = tuple(bool(f) for f in inp['semantic_classes_is_thing'])
    batch = device_batch(inp)
    for gen in (pre.MultiscaleSupervisionGenerator(tuple(p['downscales']), syn.MULTISCALE_KEYS),
                pre.InstanceClearStuffIDs(semantic_classes_is_thing=is_thing),
                pre.InstanceTargetGenerator(sigma=p['sigma'], semantic_classes_is_thing=is_thing,
                                            sigma_for_additional_downscales=dict(p['sigma_for_additional_downscales'])),
                pre.OrientationTargetGenerator(tuple(bool(f) for f in inp['estimate']))):
        batch = gen(batch)
    rng = torch.Generator(device='cuda').manual_seed(7)
    sizes = [(H, W)] + [(int(H / d), int(W / d)) for d in p['downscales']]

    def outputs(channels):
        return [torch.randn((B, channels, h, w), device='cuda', generator=rng) for h, w in sizes]

    sem, cen, off, ori = outputs(C - 1), outputs(1), outputs(2), outputs(2)
    preds = {'semantic_output': sem[0].requires_grad_(True), 'semantic_side_outputs': tuple(sem[1:]),
             'instance_output': tuple(x[0].requires_grad_(True) for x in (cen, off, ori)),
             'instance_side_outputs': tuple((cen[i], off[i], ori[i]) for i in (1, 2))}
    losses = {}
    for helper in (SemanticTaskHelper(n_classes=C - 1), InstanceTaskHelper(C, is_thing)):
        helper.initialize(torch.device('cuda'))
        losses.update(helper.training_step(batch, 0, preds)[0])
    scales = ['main'] + [f'down_{d}' for d in p['downscales']]
    want = {f'semantic_loss_{s}' for s in scales} | {'semantic_total_loss'}
    for k in ('center', 'offset', 'orientation'):
        want |= {f'instance_{k}_loss_{s}' for s in scales} | {f'instance_{k}_total_loss'}
    assert set(losses) == want
    for k, v in losses.items():
        assert torch.isfinite(v).all(), k
