"""GPU tier of `BatchAugmentation` (one launch of `nmsa_batch_augment` for every key of a batch)
against tests/golden/batch_augment.npz — the reference's own RandomCrop -> RandomHorizontalFlip ->
NormalizeRGB -> NormalizeDepth -> ToTorchTensors run per sample under `np.random.seed`
(tools/gen_golden_augment.py).  Every comparison is bit-exact on integer views of the outputs:
the moves are raw bits, and the normalisation is one IEEE subtract and one IEEE divide of float32
values on both sides.

Recipes (testing.synthetic.AUGMENT_RECIPES): A crop width % 4 == 2, both flip values, both
parities of x0; B crop equals image, every row reversed, whole-wave rows; C / C1 float32 depth
with invalid values kept, 5 x 7 and 1 x 1 crops; D rows longer than a wave, odd width; E crop
width % 4 == 0 at odd offsets (the four-pixels-per-lane path with and without flip)."""
import numpy as np
import pytest
import torch

from nicr_mt_scene_analysis_amd.testing import synthetic as syn
from test_batch_augment_host import CASES, augmentation, case

pytestmark = pytest.mark.gpu

DTYPES = {'rgb': torch.float32, 'depth': torch.float32, 'semantic': torch.uint8, 'instance': torch.int32,
          'normal': torch.float32, 'valid': torch.bool, 'segment_ids': torch.int64}


def device_batch(inp):
    """the collated raw device batch: on-wire dtypes, `segment_ids` as int64"""
    batch = {k: torch.from_numpy(np.array(inp[k])).cuda() for k in syn.AUGMENT_SPATIAL_KEYS if k != 'segment_ids'}
    batch['segment_ids'] = torch.from_numpy(inp['segment_ids'].astype(np.int64)).cuda()
    batch['orientations'] = [dict(d) for d in inp['orientations']]
    return batch


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def check_outputs(name, batch, what):
    p, inp, g = case(name)
    for k in syn.AUGMENT_SPATIAL_KEYS:
        want, got = g[f'{name}__out__{k}'], batch[k]
        assert got.dtype == DTYPES[k] and got.is_contiguous() and tuple(got.shape) == want.shape, (what, k)
        assert np.array_equal(raw(got.cpu().numpy()), raw(want)), (what, k)


@pytest.mark.parametrize('name', CASES)
def test_drawn_under_the_seed_the_batch_is_bit_identical_to_the_reference(name):
    p, inp, g = case(name)
    batch = device_batch(inp)
    before = {k: v for k, v in batch.items() if isinstance(v, torch.Tensor)}
    kept = {k: v.clone() for k, v in before.items()}
    aug = augmentation(p)
    np.random.seed(p['seed'])
    assert aug(batch) is batch
    check_outputs(name, batch, 'drawn')
    for k, v in before.items():                                # the raw tensors are only read
        assert torch.equal(v.view(torch.uint8), kept[k].view(torch.uint8)), k
    h, w = p['crop']
    assert aug.last_dynamic_parameters == [
        {'crop_slice_y': slice(int(y0), int(y0) + h), 'crop_slice_x': slice(int(x0), int(x0) + w),
         'was_flipped': bool(f)} for y0, x0, f in g[f'{name}__table']]
    from _golden import jload
    assert [[[k, v] for k, v in d.items()] for d in batch['orientations']] == jload(g[f'{name}__orientations'])
    if name == 'A':          # NaN payloads, -0.0 and denormals made it through (compared as bits above)
        bits = batch['normal'].cpu().numpy().view(np.uint32)
        assert (bits == 0xffc00001).any() and (bits == 0x7f800123).any() and (bits == 0x80000000).any() and \
            (bits == 0x00000001).any()


@pytest.mark.parametrize('name', CASES)
def test_supplied_parameters_replay_the_drawn_result(name):
    p, inp, g = case(name)
    np.random.seed(12345)                                      # not the fixture's: nothing may be drawn
    state = np.random.get_state()[1].copy()
    batch = augmentation(p)(device_batch(inp), params=g[f'{name}__table'])
    check_outputs(name, batch, 'replayed')
    assert np.array_equal(np.random.get_state()[1], state)


def test_a_call_on_another_stream_matches_the_default_stream():
    # the side stream every capture of this process runs on: a non-default stream that exists
    # anyway, so that this file takes no further stream (and no further hardware queue slot) out
    # of torch's pool ahead of the tests that time two streams against each other
    torch.cuda.graph(torch.cuda.CUDAGraph())
    stream = torch.cuda.graph.default_capture_stream
    assert stream is not None and stream != torch.cuda.default_stream()
    for name in ('A', 'E'):
        p, inp, g = case(name)
        batch = device_batch(inp)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            augmentation(p)(batch, params=g[f'{name}__table'])
        stream.synchronize()
        check_outputs(name, batch, 'side stream')
        check_outputs(name, augmentation(p)(device_batch(inp), params=g[f'{name}__table']), 'default stream again')


def test_a_captured_call_replays_with_a_new_parameter_table():
    p, inp, g = case('A')
    table = g['A__table']
    other = np.array([[0, 0, 0], [3, 15, 0], [2, 1, 1], [1, 16, 1]], np.int32)
    assert not np.array_equal(other, table)
    aug = augmentation(p)
    static = device_batch(inp)
    keep = dict(static)
    aug(dict(static), params=table)                            # the eager call a capture needs first
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    captured = dict(static)
    with torch.cuda.graph(graph):
        aug(captured, params=table)
    staging = aug.captured_staging
    assert staging is not None
    # an eager call with the same shapes between capture and replay must not disturb the graph
    check_outputs('A', augmentation(p)(device_batch(inp), params=table), 'eager after capture')
    graph.replay()
    torch.cuda.synchronize()
    check_outputs('A', captured, 'replay')
    staging.write_params(other)
    graph.replay()
    torch.cuda.synchronize()
    want = augmentation(p)(dict(keep), params=other)
    for k in syn.AUGMENT_SPATIAL_KEYS:
        assert torch.equal(captured[k].view(torch.uint8), want[k].view(torch.uint8)), k
        assert not np.array_equal(raw(captured[k].cpu().numpy()), raw(g[f'A__out__{k}'])), k
    with pytest.raises(ValueError):                            # a window that leaves the source
        staging.write_params([[5, 0, 0]] * 4)


def test_targets_of_the_augmented_batch_equal_targets_of_the_fixture_batch():
    from nicr_mt_scene_analysis_amd.data import preprocessing as pre
    p, inp, g = case('A')
    is_thing = tuple(bool(f) for f in inp['semantic_classes_is_thing'])

    def targets(batch):
        for gen in (pre.InstanceClearStuffIDs(semantic_classes_is_thing=is_thing),
                    pre.InstanceTargetGenerator(sigma=4, semantic_classes_is_thing=is_thing)):
            batch = gen(batch)
        return batch

    np.random.seed(p['seed'])
    got = targets(augmentation(p)(device_batch(inp)))
    want = targets({k: torch.from_numpy(g[f'A__out__{k}']).cuda() for k in ('semantic', 'instance')})
    keys = ('instance', 'instance_center', 'instance_offset', 'instance_foreground', 'instance_center_mask')
    assert (want['instance'] != 0).any() and want['instance_center'].max() > 0.5
    for k in keys:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k


def test_every_element_size_and_channel_count_against_the_numpy_formulation():
    """the paths the fixture's keys do not take: 2- and 8-byte elements with channels, channel
    counts that are not unrolled (2, 5), unnormalised depth, at a crop width that is a multiple
    of 4 and at one that is not — all keys of a width in one launch, against
    `np.flip(src[y0:y0 + h, x0:x0 + w], axis=1).transpose(2, 0, 1)`"""
    from nicr_mt_scene_analysis_amd import ops
    from nicr_mt_scene_analysis_amd.data.preprocessing import BatchAugmentation
    rng = np.random.default_rng(5)
    B, H, W = 3, 9, 23
    src = {}
    for dtype in (np.uint8, np.int16, np.int32, np.int64):
        for C in (None, 1, 2, 3, 5):
            shape = (B, H, W) if C is None else (B, H, W, C)
            info = np.iinfo(dtype)
            src[f'{np.dtype(dtype).name}_{C}'] = rng.integers(info.min, info.max, shape, dtype=dtype, endpoint=True)
    dev = {k: torch.from_numpy(v).cuda() for k, v in src.items()}
    for h, w, table in ((6, 12, [[0, 11, 1], [3, 0, 0], [2, 5, 1]]), (6, 11, [[3, 12, 1], [0, 0, 0], [1, 7, 1]]),
                        (9, 23, [[0, 0, 1], [0, 0, 0], [0, 0, 1]])):
        got = ops.batch_augment(dev, np.array(table), (h, w))
        for k, v in src.items():
            chw = v if v.ndim == 4 else v[..., None]
            want = np.stack([(np.flip(chw[b, y0:y0 + h, x0:x0 + w], axis=1) if f else chw[b, y0:y0 + h, x0:x0 + w])
                             .transpose(2, 0, 1) for b, (y0, x0, f) in enumerate(table)])
            want = want if v.ndim == 4 else want[:, 0]
            assert got[k].dtype == dev[k].dtype and tuple(got[k].shape) == want.shape, (w, k)
            assert np.array_equal(got[k].cpu().numpy(), want), (w, k)
        # depth without normalisation constants: cropped and flipped bits, [B,1,h,w]
        depth = torch.from_numpy(src['int16_None'].view(np.uint16)).cuda()
        out = BatchAugmentation(h, w, 0.5)({'depth': depth}, params=table)['depth']
        assert out.dtype == torch.uint16 and tuple(out.shape) == (B, 1, h, w)
        assert np.array_equal(out.cpu().numpy().view(np.int16)[:, 0], got['int16_None'].cpu().numpy()), w
