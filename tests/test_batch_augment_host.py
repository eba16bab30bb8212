"""CPU tier of `BatchAugmentation` (data/preprocessing/augmentation.py): the host logic against
tests/golden/batch_augment.npz — the reference's own crop / flip / normalise / to-tensor chain run
per sample under `np.random.seed` (tools/gen_golden_augment.py).  The regenerated inputs are
checked against the fixture's digests, the drawn parameter tables and the mirrored orientations
against what the reference recorded, and the two refusals (a batch that already holds
`orientations_present`, an image smaller than the crop) are raised before any device work."""
import functools

import numpy as np
import pytest
import torch

from _golden import jload, load
from nicr_mt_scene_analysis_amd.testing import synthetic as syn

CASES = ('A', 'B', 'C', 'C1', 'D', 'E')


@functools.lru_cache(maxsize=None)
def case(name):
    """(params, regenerated inputs, fixture); the inputs are read-only for every test"""
    g = load('batch_augment')
    p = jload(g[f'{name}__params'])
    inp = syn.make_augment_inputs(p['recipe'], p['seed'])
    assert syn.augment_input_digest(inp) == p['digest'], f'{name}: regenerated inputs differ'
    for v in inp.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p, inp, g


def augmentation(p, **kwargs):
    from nicr_mt_scene_analysis_amd.data.preprocessing import BatchAugmentation
    return BatchAugmentation(p['crop'][0], p['crop'][1], p['p'], depth_mean=p['depth_mean'], depth_std=p['depth_std'],
                             raw_depth=p['raw_depth'], invalid_depth_value=p['invalid_depth_value'], **kwargs)


@pytest.mark.parametrize('name', CASES)
def test_regenerated_inputs_match_the_fixture_digest(name):
    p, inp, g = case(name)
    assert p['recipe'] == name and inp['rgb'].dtype == np.uint8


def test_fixture_cases_are_the_ones_asked_for():
    assert jload(load('batch_augment')['names']) == list(CASES)
    want = {'A': (4, 41, 67, 37, 50, 0.5), 'B': (2, 33, 64, 33, 64, 1.0), 'C': (3, 20, 23, 5, 7, 0.0),
            'C1': (3, 20, 23, 1, 1, 0.0), 'D': (2, 40, 301, 33, 263, 0.5), 'E': (4, 21, 76, 16, 68, 0.5)}
    for name, (B, H, W, h, w, flip_p) in want.items():
        p, inp, g = case(name)
        assert inp['rgb'].shape == (B, H, W, 3) and p['crop'] == [h, w] and p['p'] == flip_p
        assert g[f'{name}__out__rgb'].shape == (B, 3, h, w) and g[f'{name}__out__depth'].shape == (B, 1, h, w)
        assert (inp['rgb'] == 0).any() and (inp['rgb'] == 255).any()
    for name in ('A', 'E'):                     # both flip values, both parities of x0
        table = case(name)[2][f'{name}__table']
        assert set(table[:, 2]) == {0, 1} and set(table[:, 1] % 2) == {0, 1}
    assert (case('B')[2]['B__table'] == (0, 0, 1)).all()
    assert set(case('D')[2]['D__table'][:, 2]) == {0, 1}
    for name in ('A', 'B', 'D', 'E'):
        depth = case(name)[1]['depth']
        assert depth.dtype == np.uint16 and (depth == 0).any() and (depth == 65535).any()
    # C: float32 depth; inside the crop windows the source holds 0.0, -0.0 and the mean
    p, inp, g = case('C')
    assert inp['depth'].dtype == np.float32 and p['raw_depth'] and p['invalid_depth_value'] == 0.0
    seen = np.concatenate([inp['depth'][b, y0:y0 + 5, x0:x0 + 7].ravel() for b, (y0, x0, _) in enumerate(g['C__table'])])
    bits = seen.view(np.uint32)
    assert (bits == 0).any() and (bits == 0x80000000).any() and (seen == np.float32(p['depth_mean'])).any()
    out = g['C__out__depth']
    assert (out.view(np.uint32) == 0x80000000).sum() == 0 and (out == 0).sum() == (seen == 0).sum() + \
        (seen == np.float32(p['depth_mean'])).sum()
    nbits = case('A')[1]['normal'].view(np.uint32)
    assert (nbits == 0xffc00001).any() and (nbits == 0x80000000).any() and (nbits == 0x00000001).any()


@pytest.mark.parametrize('name', CASES)
def test_drawing_under_the_seed_gives_the_reference_table(name):
    p, inp, g = case(name)
    B, H, W = inp['rgb'].shape[:3]
    np.random.seed(p['seed'])
    table = augmentation(p).draw_params(B, H, W)
    assert table.dtype == np.int32 and np.array_equal(table, g[f'{name}__table'])
    # a generator of the caller's gives the same draws and leaves the module-level one alone
    np.random.seed(1)
    state = np.random.get_state()[1].copy()
    table = augmentation(p, rng=np.random.RandomState(p['seed'])).draw_params(B, H, W)
    assert np.array_equal(table, g[f'{name}__table'])
    assert np.array_equal(np.random.get_state()[1], state)


@pytest.mark.parametrize('name', CASES)
def test_orientation_mirroring_equals_the_reference(name):
    from nicr_mt_scene_analysis_amd.data.preprocessing import BatchAugmentation
    p, inp, g = case(name)
    orientations = [dict(d) for d in inp['orientations']]
    BatchAugmentation.mirror_orientations(orientations, [bool(f) for f in g[f'{name}__table'][:, 2]])
    assert [[[k, v] for k, v in d.items()] for d in orientations] == jload(g[f'{name}__orientations'])
    if name == 'B':         # every sample flipped: no angle stayed, all of them in [0, 2 pi)
        assert all(0.0 <= v < 2 * np.pi and v != inp['orientations'][b][k]
                   for b, d in enumerate(orientations) for k, v in d.items())


def test_refusals_come_before_any_device_work():
    from nicr_mt_scene_analysis_amd._lib import NmsaError
    from nicr_mt_scene_analysis_amd.data.preprocessing import BatchAugmentation
    aug = BatchAugmentation(5, 7, 0.5)
    rgb = torch.zeros((1, 5, 9, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='OrientationTargetGenerator'):
        aug({'rgb': rgb, 'orientations_present': [{}]})
    for shape in ((1, 4, 9, 3), (1, 5, 6, 3), (1, 4, 6, 3)):
        with pytest.raises(NotImplementedError, match='cv2'):
            aug({'rgb': torch.zeros(shape, dtype=torch.uint8)})
    with pytest.raises(NotImplementedError, match='cv2'):
        aug({'depth': torch.zeros((1, 4, 9))})
    # H == crop_h is not that case (the reference's scale stays 1.0): the call goes on to the
    # device path, which refuses host tensors
    with pytest.raises(NmsaError):
        aug({'rgb': rgb})
    with pytest.raises(NmsaError):
        BatchAugmentation(5, 9, 0.5)({'rgb': rgb})
    # a spatial tensor of another size would be cropped by the reference: refused
    with pytest.raises(ValueError, match='keys_to_ignore'):
        aug({'rgb': rgb, 'lut': torch.zeros((1, 3, 4))})
    with pytest.raises(NmsaError):
        BatchAugmentation(5, 7, 0.5, keys_to_ignore=('lut',))({'rgb': rgb, 'lut': torch.zeros((1, 3, 4))})
    with pytest.raises(ValueError):
        BatchAugmentation(5, 7, 0.5, depth_mean=1.0, depth_std=0.0)
    # supplied tables are checked: a window that leaves the source, a flip of 2
    for bad in ([[1, 0, 0]], [[0, 3, 0]], [[-1, 0, 0]], [[0, 0, 2]], [[0, 0]]):
        with pytest.raises(ValueError):
            aug({'rgb': rgb}, params=bad)
