"""GPU tier: the staging caches of `ops.batch_augment` and `ops.multiscale_nearest` (`_AUG_STAGING`,
`_MS_STAGING`: LRUs of 8 keyed by shape set and stream, eviction that waits on the event of the
last copy, stagings taken out for good by a hipGraph capture), and sources that are views.

Every result is compared bit for bit with the numpy formulations of tests/_desc_tables.py.  The
multiscale shapes are multiples of their downscales, where OpenCV's nearest rule is the plain
stride `arange(n // d) * d` (test_multiscale_supervision.py pins that on the CPU), so the maps on
the reference side are numpy's too."""
import numpy as np
import pytest
import torch

import _desc_tables as dt
from nicr_mt_scene_analysis_amd import ops

pytestmark = pytest.mark.gpu

SIGNED = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}
RGB_MEAN = np.array((0.485, 0.456, 0.406), dtype='float32') * 255
RGB_STD = np.array((0.229, 0.224, 0.225), dtype='float32') * 255
DEPTH = (1.5, 0.75, True, 0.0)
NORM = {'rgb': ('rgb_norm', RGB_MEAN, RGB_STD), 'depth': ('depth_norm',) + DEPTH}


def raw(t):
    return dt.raw_bytes(t.cpu().numpy())


def to_device(arrays):
    return {k: torch.from_numpy(v).cuda() for k, v in arrays.items()}


# ------------------------------------------------------------------------------- augment
def augment_set(i, rng, B=2):
    """shape set i: its own H, W and crop (widths 12 and 11 in turn: both lane routes), an rgb
    key, a float32 depth key and two moved keys -> (arrays, (h, w))"""
    H, W = 7 + i, 14 + i
    arrays = {'rgb': dt.random_bits(rng, (B, H, W, 3), 1),
              'depth': dt.random_bits(rng, (B, H, W), 4).view(np.float32),
              'ids': dt.random_bits(rng, (B, H, W), 8).view(np.int64),
              'pair': dt.random_bits(rng, (B, H, W, 2), 2).view(np.int16)}
    return arrays, (5, 12 if i % 2 == 0 else 11)


def draw_table(rng, B, H, W, h, w):
    return np.stack([rng.integers(0, H - h, B, endpoint=True), rng.integers(0, W - w, B, endpoint=True),
                     rng.integers(0, 2, B)], axis=1).astype(np.int32)


def augment_want(arrays, table, hw):
    want = {}
    for k, a in arrays.items():
        src = a if a.ndim == 4 else a[..., None]
        if k == 'rgb':
            want[k] = dt.augment_reference(src, table, hw, dt.RGB_NORM, RGB_MEAN, RGB_STD)
        elif k == 'depth':
            want[k] = dt.augment_reference(src, table, hw, dt.DEPTH_NORM, DEPTH[:1], DEPTH[1:2], DEPTH[2], DEPTH[3])
        else:
            want[k] = dt.augment_reference(src, table, hw) if a.ndim == 4 else dt.augment_reference(src, table, hw)[:, 0]
    return want


def check_augment(got, want, what):
    assert list(got) == list(want)
    for k in want:
        assert tuple(got[k].shape) == want[k].shape and got[k].element_size() == want[k].dtype.itemsize, (what, k)
        assert np.array_equal(raw(got[k]), dt.raw_bytes(want[k])), (what, k)


def test_augment_lru_eviction_without_synchronisation():
    """ten shape sets round-robin three times, nothing synchronised in between: every call
    misses the cache of 8, builds a staging and drops the oldest while its copy may be in flight"""
    rng = np.random.default_rng(20)
    sets = [augment_set(i, rng) for i in range(10)]
    device = [to_device(arrays) for arrays, _ in sets]
    tables = [[draw_table(rng, 2, *arrays['rgb'].shape[1:3], *hw) for arrays, hw in sets] for _ in range(3)]
    torch.cuda.synchronize()
    results = []
    for turn in range(3):
        for i, (arrays, hw) in enumerate(sets):
            results.append((turn, i, ops.batch_augment(device[i], tables[turn][i], hw, NORM)))
            assert len(ops._AUG_STAGING) <= 8
    torch.cuda.synchronize()
    assert len(ops._AUG_STAGING) == 8
    for turn, i, got in results:
        check_augment(got, augment_want(sets[i][0], tables[turn][i], sets[i][1]), (turn, i))


def test_augment_captured_staging_survives_eviction_and_an_eager_rebuild():
    rng = np.random.default_rng(21)
    arrays, hw = augment_set(12, rng, B=3)
    H, W = arrays['rgb'].shape[1:3]
    t0, t1, t2 = (draw_table(rng, 3, H, W, *hw) for _ in range(3))
    assert not np.array_equal(t0, t1) and not np.array_equal(t0, t2) and not np.array_equal(t1, t2)
    static = to_device(arrays)
    check_augment(ops.batch_augment(static, t0, hw, NORM), augment_want(arrays, t0, hw), 'the eager call a capture needs first')
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured, staging = ops.batch_augment(static, t0, hw, NORM, return_staging=True)
    assert any(s is staging for s in ops._AUG_CAPTURED) and all(s is not staging for s in ops._AUG_STAGING.values())
    # nine other shape sets: the cache of 8 turns over completely
    others = [augment_set(i, rng) for i in range(9)]
    for i, (other, other_hw) in enumerate(others):
        table = draw_table(rng, 2, *other['rgb'].shape[1:3], *other_hw)
        check_augment(ops.batch_augment(to_device(other), table, other_hw, NORM), augment_want(other, table, other_hw), i)
        assert len(ops._AUG_STAGING) <= 8
    graph.replay()
    torch.cuda.synchronize()
    check_augment(captured, augment_want(arrays, t0, hw), 'replay after eviction pressure')
    # the same shape set, eagerly: a staging of its own, the captured one untouched
    eager, rebuilt = ops.batch_augment(static, t1, hw, NORM, return_staging=True)
    assert rebuilt is not staging and rebuilt.host.data_ptr() != staging.host.data_ptr()
    assert any(s is rebuilt for s in ops._AUG_STAGING.values())
    assert np.array_equal(staging.params, t0)
    check_augment(eager, augment_want(arrays, t1, hw), 'eager after capture')
    graph.replay()
    torch.cuda.synchronize()
    check_augment(captured, augment_want(arrays, t0, hw), 'replay after the eager call')
    for table in (t2, t1, t0):
        staging.write_params(table)
        graph.replay()
        again = ops.batch_augment(static, t1, hw, NORM)              # the eager staging is rewritten in between
        torch.cuda.synchronize()
        check_augment(captured, augment_want(arrays, table, hw), 'replay with written parameters')
        check_augment(again, augment_want(arrays, t1, hw), 'eager between replays')


def view_after_first(array):
    """`big[1:]` along the leading axis: contiguous, at a storage offset of one sample"""
    big = torch.from_numpy(np.concatenate([np.full_like(array[:1], 0x5a), array])).cuda()
    view = big[1:]
    assert view.is_contiguous() and view.storage_offset() == array[0].size
    return view


def view_at_odd_offset(array):
    """a contiguous tensor one element into its storage: its address is aligned to the element
    size only"""
    flat = torch.from_numpy(np.concatenate([np.full((1,), 0x5a, array.dtype), array.reshape(-1)])).cuda()
    view = flat[1:].view(array.shape)
    size = array.dtype.itemsize
    assert view.is_contiguous() and view.storage_offset() == 1 and view.data_ptr() % (2 * size) == size
    return view


@pytest.mark.parametrize('make_view', (view_after_first, view_at_odd_offset))
@pytest.mark.parametrize('w', (12, 11))
def test_augment_sources_that_are_views(w, make_view):
    rng = np.random.default_rng(22 + w)
    B, H, W, h = 3, 6, 17, 5
    arrays = {f'move{size}_{C}': dt.random_bits(rng, (B, H, W) + ((C,) if C else ()), size).view(SIGNED[size])
              for size in (1, 2, 4, 8) for C in (0, 3, 2)}
    arrays['rgb'] = dt.random_bits(rng, (B, H, W, 3), 1)
    arrays['depth'] = dt.random_bits(rng, (B, H, W), 4).view(np.float32)
    table = draw_table(rng, B, H, W, h, w)
    views = {k: make_view(v) for k, v in arrays.items()}
    kept = {k: v.clone() for k, v in views.items()}
    got = ops.batch_augment(views, table, (h, w), NORM)
    check_augment(got, augment_want(arrays, table, (h, w)), make_view.__name__)
    for k in views:
        assert np.array_equal(raw(views[k]), raw(kept[k])), k
    assert all(t.data_ptr() % 256 == 0 for t in got.values())      # the outputs of ops start on 256 bytes


def side_stream():
    # the side stream every capture of this process runs on: a non-default stream that exists
    # anyway, so that this file takes no further stream (and no further hardware queue slot) out
    # of torch's pool ahead of the tests that time two streams against each other
    torch.cuda.graph(torch.cuda.CUDAGraph())
    stream = torch.cuda.graph.default_capture_stream
    assert stream is not None and stream != torch.cuda.default_stream()
    return stream


def test_augment_on_two_streams():
    rng = np.random.default_rng(23)
    stream = side_stream()
    for i in (13, 14):                                               # both lane routes
        arrays, hw = augment_set(i, rng)
        device = to_device(arrays)
        tables = [draw_table(rng, 2, *arrays['rgb'].shape[1:3], *hw) for _ in range(4)]
        torch.cuda.synchronize()
        for turn, table in enumerate(tables):
            if turn % 2 == 0:
                with torch.cuda.stream(stream):
                    got = ops.batch_augment(device, table, hw, NORM)
                stream.synchronize()
            else:
                got = ops.batch_augment(device, table, hw, NORM)
                torch.cuda.synchronize()
            check_augment(got, augment_want(arrays, table, hw), (i, 'side' if turn % 2 == 0 else 'default', turn))


# ------------------------------------------------------------------------------- multiscale
DOWNSCALES = (2, 4)


def multiscale_set(i, rng):
    """shape set i: its own H x W (multiples of 4), one key of every element size"""
    H, W = 8 + 4 * i, 12 + 4 * i
    return {'u8': dt.random_bits(rng, (2, H, W), 1), 'i16': dt.random_bits(rng, (1, 2, H, W), 2).view(np.int16),
            'f32': dt.random_bits(rng, (2, 3, H, W), 4).view(np.float32), 'i64': dt.random_bits(rng, (2, H, W), 8).view(np.int64)}


def multiscale_want(arrays):
    want = {d: {} for d in DOWNSCALES}
    for d in DOWNSCALES:
        for k, a in arrays.items():
            H, W = a.shape[-2:]
            assert H % d == 0 and W % d == 0
            out = dt.multiscale_reference(a.reshape(-1, H, W), np.arange(H // d) * d, np.arange(W // d) * d)
            want[d][k] = out.reshape(a.shape[:-2] + (H // d, W // d))
    return want


def check_multiscale(got, want, what):
    assert list(got) == list(want)
    for d in want:
        assert list(got[d]) == list(want[d])
        for k in want[d]:
            assert tuple(got[d][k].shape) == want[d][k].shape and got[d][k].element_size() == want[d][k].dtype.itemsize
            assert np.array_equal(raw(got[d][k]), dt.raw_bytes(want[d][k])), (what, d, k)


def hw_of(arrays):
    return tuple(arrays['u8'].shape[-2:])


def test_multiscale_lru_eviction_without_synchronisation():
    rng = np.random.default_rng(24)
    sets = [[multiscale_set(i, rng) for i in range(10)] for _ in range(3)]          # new contents every turn
    device = [[to_device(arrays) for arrays in turn] for turn in sets]
    torch.cuda.synchronize()
    results = []
    for turn in range(3):
        for i in range(10):
            results.append((turn, i, ops.multiscale_nearest(device[turn][i], DOWNSCALES, hw_of(sets[turn][i]))))
            assert len(ops._MS_STAGING) <= 8
    torch.cuda.synchronize()
    assert len(ops._MS_STAGING) == 8
    for turn, i, got in results:
        check_multiscale(got, multiscale_want(sets[turn][i]), (turn, i))


def test_multiscale_captured_staging_survives_eviction_and_an_eager_rebuild():
    rng = np.random.default_rng(25)
    arrays = multiscale_set(12, rng)
    hw = hw_of(arrays)
    static = to_device(arrays)
    check_multiscale(ops.multiscale_nearest(static, DOWNSCALES, hw), multiscale_want(arrays), 'the eager call a capture needs first')
    torch.cuda.synchronize()
    n_captured = len(ops._MS_CAPTURED)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ops.multiscale_nearest(static, DOWNSCALES, hw)
    assert len(ops._MS_CAPTURED) == n_captured + 1
    staging = ops._MS_CAPTURED[-1]
    assert all(s is not staging for s in ops._MS_STAGING.values())
    for i in range(9):
        other = multiscale_set(i, rng)
        check_multiscale(ops.multiscale_nearest(to_device(other), DOWNSCALES, hw_of(other)), multiscale_want(other), i)
        assert len(ops._MS_STAGING) <= 8
    graph.replay()
    torch.cuda.synchronize()
    check_multiscale(captured, multiscale_want(arrays), 'replay after eviction pressure')
    # the same shape set, eagerly, on other tensors: a staging of its own
    moved = multiscale_set(12, rng)
    eager = ops.multiscale_nearest(to_device(moved), DOWNSCALES, hw)
    rebuilt = next(reversed(ops._MS_STAGING.values()))
    assert rebuilt is not staging and rebuilt['host'].data_ptr() != staging['host'].data_ptr()
    assert rebuilt['outputs'] == staging['outputs']
    check_multiscale(eager, multiscale_want(moved), 'eager after capture')
    graph.replay()
    torch.cuda.synchronize()
    check_multiscale(captured, multiscale_want(arrays), 'replay after the eager call')
    # new contents in the captured inputs: the replay gathers them
    for k, v in moved.items():
        static[k].copy_(torch.from_numpy(v))
    graph.replay()
    torch.cuda.synchronize()
    check_multiscale(captured, multiscale_want(moved), 'replay on new contents')


@pytest.mark.parametrize('make_view', (view_after_first, view_at_odd_offset))
def test_multiscale_sources_that_are_views(make_view):
    rng = np.random.default_rng(26)
    arrays = multiscale_set(3, rng)
    views = {k: make_view(v) for k, v in arrays.items()}
    kept = {k: v.clone() for k, v in views.items()}
    check_multiscale(ops.multiscale_nearest(views, DOWNSCALES, hw_of(arrays)), multiscale_want(arrays), make_view.__name__)
    for k in views:
        assert np.array_equal(raw(views[k]), raw(kept[k])), k


def test_multiscale_on_two_streams():
    rng = np.random.default_rng(27)
    stream = side_stream()
    for turn in range(4):
        arrays = multiscale_set(13, rng)
        device = to_device(arrays)
        torch.cuda.synchronize()
        if turn % 2 == 0:
            with torch.cuda.stream(stream):
                got = ops.multiscale_nearest(device, DOWNSCALES, hw_of(arrays))
            stream.synchronize()
        else:
            got = ops.multiscale_nearest(device, DOWNSCALES, hw_of(arrays))
            torch.cuda.synchronize()
        check_multiscale(got, multiscale_want(arrays), ('side' if turn % 2 == 0 else 'default', turn))
