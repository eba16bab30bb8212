"""GPU tier: `nmsa_batch_augment` (csrc/augment.hip) and `nmsa_multiscale_nearest`
(csrc/multiscale.hip) straight at the C ABI, at the edges of their shared design — a descriptor
table in a pinned staging buffer, a block prefix (and, for augment, a lane route) filled in by the
entry point, and a binary search of every workgroup for its descriptor.

Every source and every destination lies in an arena of tests/_desc_tables.py: poison on both
sides of each range, so a store one group too far or a source index one row or column outside
the window shows.  Every launch ends with the guard check and the sources-unchanged check (inside
`run_augment` / `run_multiscale`), and every comparison is bit-exact against the numpy
formulations that test_desc_tables_reference.py proves against the recorded fixtures: the
kernels move bits, or do one IEEE subtract and one IEEE divide."""
import numpy as np
import pytest

import _desc_tables as dt

pytestmark = pytest.mark.gpu

UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
DEPTH_MEAN, DEPTH_STD = 2841.94941272766, 1417.2594281672277
RGB_MEAN = np.array((0.485, 0.456, 0.406), dtype='float32') * 255
RGB_STD = np.array((0.229, 0.224, 0.225), dtype='float32') * 255


def groups_of(words):
    """work items of every augment descriptor read back: B * h * (w / pixels_per_lane)"""
    return [int(d[dt.A_B]) * int(d[dt.A_CROP_H]) * (int(d[dt.A_CROP_W]) // int(d[dt.A_PPL])) for d in words]


# =============================================================================== augment
# (h, w, destination misaligned) -> work items with B = 1; 256, 512 and 1000 take the four-pixel route
PREFIX_SHAPES = (((257, 1, False), 257), ((1, 1, False), 1), ((8, 256, False), 512), ((15, 17, False), 255),
                 ((10, 30, False), 300), ((27, 19, False), 513), ((16, 64, False), 256), ((8, 500, False), 1000),
                 ((7, 73, False), 511), ((16, 16, True), 256), ((4, 128, True), 512))


def prefix_cases(rng, shapes):
    cases = []
    for (h, w, misaligned), items in shapes:
        src = dt.random_bits(rng, (1, h + 1, w + 1, 1), 4)
        cases.append({'src': src, 'hw': (h, w), 'align': 16, 'misalign': 4 if misaligned else 0})
    return cases


def check_augment_prefix(shapes, words):
    want_ppl = [4 if w % 4 == 0 and not misaligned else 1 for (h, w, misaligned), _ in shapes]
    assert words[:, dt.A_PPL].tolist() == want_ppl
    assert groups_of(words) == [items for _, items in shapes]
    assert words[:, dt.A_BLOCK_BEGIN].tolist() == dt.block_prefix([items for _, items in shapes])


def test_augment_block_prefix_at_workgroup_boundaries():
    """descriptors that end one short of, on and one past a multiple of 256 work items, not
    sorted by size, every source different: the wrong descriptor at a block boundary gives other
    bits.  The same shapes alone and in tables of 2, 3 and 5 (the search at sizes that are and
    are not powers of two)."""
    rng = np.random.default_rng(11)
    assert sorted(items for _, items in PREFIX_SHAPES[:9]) == [1, 255, 256, 257, 300, 511, 512, 513, 1000]
    words, _ = dt.run_augment(prefix_cases(rng, PREFIX_SHAPES), [[1, 1, 0]])
    check_augment_prefix(PREFIX_SHAPES, words)
    assert words[:, dt.A_BLOCK_BEGIN].tolist() == [0, 2, 3, 5, 6, 8, 11, 12, 16, 18, 19]
    print('augment block_begin', words[:, dt.A_BLOCK_BEGIN].tolist(), 'pixels_per_lane', words[:, dt.A_PPL].tolist())
    for shape in PREFIX_SHAPES:
        words, _ = dt.run_augment(prefix_cases(rng, [shape]), [[0, 1, 1]])
        check_augment_prefix([shape], words)
    for n in (2, 3, 5):
        for first in (0, 3, 6):
            shapes = PREFIX_SHAPES[first:first + n]
            words, _ = dt.run_augment(prefix_cases(rng, shapes), [[1, 0, 1]])
            check_augment_prefix(shapes, words)


def test_augment_table_limit():
    """NMSA_AUGMENT_MAX_DESC descriptors of a 1 x 1 crop in one launch: descriptor i writes i"""
    n = dt.AUG_MAX_DESC
    cases = []
    for i in range(n):
        src = np.array([[[1000 + i], [2000 + i]], [[3000 + i], [i]]], np.uint32)[None]         # [1,2,2,1]
        cases.append({'src': src, 'hw': (1, 1), 'align': 4, 'src_align': 4})
    words, outs = dt.run_augment(cases, [[1, 1, 0]])
    assert [int(o.ravel()[0]) for o in outs] == list(range(n))
    assert words[:, dt.A_BLOCK_BEGIN].tolist() == list(range(n)) and (words[:, dt.A_PPL] == 1).all()


@pytest.mark.parametrize('flip', (0, 1))
@pytest.mark.parametrize('size', (1, 2, 4, 8))
def test_augment_lane_route_of_every_element_size_and_channel_count(size, flip):
    """w = 12 on an aligned destination takes four pixels per lane; the same width one element
    off 16-byte alignment (one byte off 4-byte alignment for 1-byte elements) and w = 11 take
    one.  The misaligned destination cannot be reached through ops.batch_augment."""
    rng = np.random.default_rng(100 * size + flip)
    B, H, W, h = 3, 5, 15, 4
    table = [[1, 3, flip], [0, 2, flip], [1, 0, flip]]
    cases, want_ppl = [], []
    for channels in (1, 2, 3, 4, 5):
        routes = [(12, 0, 4), (12, 1 if size == 1 else size, 1), (11, 0, 1)]
        if dt.vec_bytes(size) < 16:              # a destination on the store's own alignment only
            routes.append((12, dt.vec_bytes(size), 4))
        for w, misalign, ppl in routes:
            cases.append({'src': dt.random_bits(rng, (B, H, W, channels), size), 'hw': (h, w), 'align': 16,
                          'misalign': misalign, 'src_align': size * 2, 'src_misalign': size})
            want_ppl.append(ppl)
    words, _ = dt.run_augment(cases, table)
    assert words[:, dt.A_PPL].tolist() == want_ppl
    assert words[:, dt.A_BLOCK_BEGIN].tolist() == dt.block_prefix(groups_of(words))


@pytest.mark.parametrize('flip', (0, 1))
def test_augment_lane_route_of_the_normalising_modes(flip):
    """RGB_NORM and both DEPTH_NORM sources on a destination 4 bytes off 16-byte alignment (one
    pixel per lane at w = 12), next to the aligned one (four)"""
    rng = np.random.default_rng(7 + flip)
    B, H, W, h, w = 2, 6, 14, 5, 12
    table = [[1, 2, flip], [0, 1, flip]]
    depth32 = (rng.random((B, H, W, 1)) * 4000).astype(np.float32)
    cases, want_ppl = [], []
    for misalign, ppl in ((0, 4), (4, 1), (8, 1), (12, 1)):
        place = {'hw': (h, w), 'align': 16, 'misalign': misalign}
        cases += [dict(place, src=dt.random_bits(rng, (B, H, W, 3), 1), mode=dt.RGB_NORM, mean=RGB_MEAN, std=RGB_STD),
                  dict(place, src=dt.random_bits(rng, (B, H, W, 1), 2), mode=dt.DEPTH_NORM, mean=(DEPTH_MEAN,),
                       std=(DEPTH_STD,), src_align=4, src_misalign=2),
                  dict(place, src=depth32, mode=dt.DEPTH_NORM, mean=(DEPTH_MEAN,), std=(DEPTH_STD,), raw_depth=1)]
        want_ppl += [ppl] * 3
    words, _ = dt.run_augment(cases, table)
    assert words[:, dt.A_PPL].tolist() == want_ppl


WINDOWS = {
    # name: (B, H, W, h, w, table)
    'last_row_and_column': (3, 9, 23, 6, 12, [[3, 11, 1], [3, 11, 0], [0, 0, 1]]),
    'last_row_and_column_odd_width': (2, 9, 23, 6, 11, [[3, 12, 0], [3, 12, 1]]),
    'one_pixel': (2, 4, 5, 1, 1, [[3, 4, 1], [0, 0, 0]]),
    'one_group_per_row': (2, 5, 7, 3, 4, [[2, 3, 1], [1, 0, 0]]),
    'row_longer_than_a_workgroup': (2, 3, 1030, 2, 1028, [[1, 2, 1], [0, 1, 0]]),
    'one_sample': (1, 7, 13, 5, 8, [[2, 5, 1]]),
    'parities_and_flips': (8, 6, 19, 4, 12, [[0, 0, 0], [1, 1, 1], [2, 2, 1], [0, 3, 0], [1, 4, 1], [2, 5, 0],
                                             [0, 6, 1], [2, 7, 0]]),
    'crop_is_the_image': (2, 3, 8, 3, 8, [[0, 0, 1], [0, 0, 0]]),
}


@pytest.mark.parametrize('name', sorted(WINDOWS))
def test_augment_windows(name):
    """windows at the last row and column of the source (poison behind them), one pixel, one
    group per row, a row longer than a workgroup's 1024 pixels, one sample, both parities of x0
    with both flips in one table — each at every element size, unrolled and walked channel
    counts, both normalising modes, on both lane routes where the width allows the wide one"""
    B, H, W, h, w, table = WINDOWS[name]
    rng = np.random.default_rng(sorted(WINDOWS).index(name))
    cases = []
    for misalign in (0, 4) if w % 4 == 0 else (0,):
        for size, channels in ((1, 3), (1, 1), (2, 1), (2, 4), (4, 3), (4, 2), (8, 1), (8, 5)):
            cases.append({'src': dt.random_bits(rng, (B, H, W, channels), size), 'hw': (h, w), 'align': 16,
                          'misalign': (misalign // 4) * (1 if size == 1 else max(size, 4)),    # one element, or one byte
                          'src_align': 2 * size, 'src_misalign': size})
        place = {'hw': (h, w), 'align': 16, 'misalign': misalign}
        cases += [dict(place, src=dt.random_bits(rng, (B, H, W, 3), 1), mode=dt.RGB_NORM, mean=RGB_MEAN, std=RGB_STD),
                  dict(place, src=dt.random_bits(rng, (B, H, W, 1), 2), mode=dt.DEPTH_NORM, mean=(DEPTH_MEAN,),
                       std=(DEPTH_STD,), raw_depth=1, invalid=0.0)]
    words, _ = dt.run_augment(cases, table)
    want_ppl = [4 if w % 4 == 0 and c.get('misalign', 0) == 0 else 1 for c in cases]
    assert words[:, dt.A_PPL].tolist() == want_ppl
    assert words[:, dt.A_BLOCK_BEGIN].tolist() == dt.block_prefix(groups_of(words))


@pytest.mark.parametrize('raw_depth', (0, 1))
@pytest.mark.parametrize('invalid', (0, 65535))
def test_augment_depth_norm_uint16(invalid, raw_depth):
    """uint16 depth with the invalid value 0 and 65535, kept and not kept, on both lane routes
    and with both flips"""
    rng = np.random.default_rng(invalid + raw_depth)
    B, H, W, h, w = 4, 5, 14, 4, 12
    src = dt.random_bits(rng, (B, H, W, 1), 2)
    src[rng.random(src.shape) < 0.2] = 0
    src[rng.random(src.shape) < 0.2] = 65535
    table = [[1, 2, 0], [0, 1, 1], [1, 0, 1], [0, 2, 0]]
    consts = {'mode': dt.DEPTH_NORM, 'mean': (DEPTH_MEAN,), 'std': (DEPTH_STD,), 'raw_depth': raw_depth,
              'invalid': float(invalid), 'hw': (h, w), 'align': 16}
    words, outs = dt.run_augment([dict(consts, src=src, misalign=0), dict(consts, src=src, misalign=4),
                                  dict(consts, src=src, hw=(h, 11))], table)
    assert words[:, dt.A_PPL].tolist() == [4, 1, 1]
    window = np.stack([src[b, y0:y0 + h, x0:x0 + w, 0] for b, (y0, x0, _) in enumerate(table)])
    assert (window == invalid).any() and (window == 65535 - invalid).any()
    # no normalised value equals either invalid value (the mean is no integer, 65535 is far off)
    for out in outs[:2]:
        assert (out == np.float32(invalid)).sum() == ((window == invalid).sum() if raw_depth else 0)


F32_SPECIALS = (0x7fc00000, 0xffc00001, 0x7f800123, 0x7fc12345, 0x7f800000, 0xff800000, 0x80000000, 0x00000000,
                0x00000001, 0x807fffff, 0x00400000)


@pytest.mark.parametrize('mean, std', ((1.5, 0.75), (0.0, 3.0)))
@pytest.mark.parametrize('raw_depth', (0, 1))
def test_augment_depth_norm_float32_specials(raw_depth, mean, std):
    """float32 depth holding NaNs with payloads, infinities, -0.0, denormals and the invalid
    value 0.0 itself: with raw_depth, 0.0 and -0.0 both come out as +0.0 (as bits)"""
    rng = np.random.default_rng(3)
    B, H, W, h, w = 2, 5, 14, 4, 12
    src = (rng.random((B, H, W, 1)) * 4.0).astype(np.float32)
    strewn = rng.permutation(src.size)[:8 * len(F32_SPECIALS)]              # eight of each among the 140
    for k, bits in enumerate(F32_SPECIALS):
        src.view(np.uint32).reshape(-1)[strewn[k::len(F32_SPECIALS)]] = bits
    table = [[1, 2, 0], [0, 1, 1]]
    consts = {'mode': dt.DEPTH_NORM, 'mean': (mean,), 'std': (std,), 'raw_depth': raw_depth, 'invalid': 0.0,
              'hw': (h, w), 'align': 16}
    words, outs = dt.run_augment([dict(consts, src=src, misalign=0), dict(consts, src=src, misalign=4),
                                  dict(consts, src=src, hw=(h, 11))], table)
    assert words[:, dt.A_PPL].tolist() == [4, 1, 1]
    window = np.stack([src[b, y0:y0 + h, x0:x0 + w, 0] for b, (y0, x0, _) in enumerate(table)])
    for bits in F32_SPECIALS:
        assert (window.view(np.uint32) == bits).any(), hex(bits)
    zeros = np.stack([np.flip(v, axis=1) if f else v for v, (_, _, f) in zip(window, table)]) == 0
    assert (window.view(np.uint32) == 0x80000000).sum() > 0
    for out in outs[:2]:
        if raw_depth:
            assert (out[:, 0].view(np.uint32)[zeros] == 0).all()          # -0.0 against 0.0 gives +0.0
        else:
            assert (out[:, 0][zeros] == np.float32((0.0 - mean) / std)).all()


def test_augment_depth_norm_nan_invalid_value_keeps_nothing():
    """a NaN invalid value never compares equal: every element is normalised, NaN sources too"""
    rng = np.random.default_rng(4)
    B, H, W, h, w = 2, 5, 14, 4, 12
    src32 = (rng.random((B, H, W, 1)) * 4.0).astype(np.float32)
    src32.view(np.uint32)[rng.random(src32.shape) < 0.3] = 0x7fc00000
    src16 = dt.random_bits(rng, (B, H, W, 1), 2)
    consts = {'mode': dt.DEPTH_NORM, 'mean': (1.5,), 'std': (0.75,), 'raw_depth': 1, 'invalid': float('nan'),
              'hw': (h, w), 'align': 16}
    words, outs = dt.run_augment([dict(consts, src=src32), dict(consts, src=src32, misalign=4), dict(consts, src=src16),
                                  dict(consts, src=src16, hw=(h, 11))], [[1, 2, 0], [0, 1, 1]])
    assert words[:, dt.A_PPL].tolist() == [4, 1, 4, 1]
    assert not np.isnan(outs[2]).any() and not np.isnan(outs[3]).any()
    want = dt.augment_reference(src16, [[1, 2, 0], [0, 1, 1]], (h, w), dt.DEPTH_NORM, (1.5,), (0.75,), 0, 0.0)
    assert np.array_equal(outs[2], want)


# =============================================================================== multiscale
def map_kinds(rng, side):
    """maps OpenCV would never produce, over a source side of `side` elements"""
    return {'identity': np.arange(side), 'reversed': np.arange(side)[::-1], 'zero': np.zeros((5,), np.int64),
            'last': np.full((side + 3,), side - 1), 'permutation': rng.permutation(side),
            'repeats': rng.integers(0, side, (2 * side + 1,))}


MAP_PAIRS = (('identity', 'reversed'), ('reversed', 'identity'), ('zero', 'last'), ('last', 'zero'),
             ('permutation', 'repeats'), ('repeats', 'permutation'), ('permutation', 'permutation'),
             ('identity', 'identity'))


@pytest.mark.parametrize('planes', (1, 3, 6))
@pytest.mark.parametrize('size', (1, 2, 4, 8))
def test_multiscale_arbitrary_maps(size, planes):
    """dst[p, y, x] = src[p, rows[y], cols[x]] for maps that are not monotone, not injective and
    longer than the source side, different for rows and columns, on a 7 x 11 and on a square
    source (rows and columns swapped is wrong there too)"""
    rng = np.random.default_rng(10 * size + planes)
    cases = []
    for H, W in ((7, 11), (9, 9)):
        rows_of, cols_of = map_kinds(rng, H), map_kinds(rng, W)
        for rows, cols in MAP_PAIRS:
            cases.append({'src': dt.random_bits(rng, (planes, H, W), size), 'rows': rows_of[rows], 'cols': cols_of[cols],
                          'align': size, 'src_align': 2 * size, 'src_misalign': size})
    square = cases[-2]
    assert len(square['rows']) == len(square['cols']) and not np.array_equal(square['rows'], square['cols'])
    words, outs = dt.run_multiscale(cases)
    assert words[:, dt.M_BLOCK_BEGIN].tolist() == dt.block_prefix([o.size for o in outs])
    if size >= 4:               # NaN payloads and -0.0 made it through (compared as bytes above)
        bits = np.concatenate([o.ravel() for o in outs])
        for special in (dt.SPECIAL_BITS32 if size == 4 else dt.SPECIAL_BITS64)[1:4]:
            assert (bits == special).any(), hex(special)


# (planes, h, w) -> planes * h * w output elements
MS_PREFIX_SHAPES = ((1, 257, 1), (1, 1, 1), (2, 16, 16), (3, 5, 17), (3, 9, 19), (1, 16, 16), (2, 10, 15))


def ms_prefix_cases(rng, shapes):
    cases = []
    for i, (planes, h, w) in enumerate(shapes):
        H, W = h + 2, w + 1
        cases.append({'src': dt.random_bits(rng, (planes, H, W), (4, 1, 2, 8)[i % 4]),
                      'rows': rng.integers(0, H, (h,)), 'cols': rng.integers(0, W, (w,))})
    return cases


def test_multiscale_block_prefix_at_workgroup_boundaries():
    rng = np.random.default_rng(12)
    totals = [p * h * w for p, h, w in MS_PREFIX_SHAPES]
    assert totals == [257, 1, 512, 255, 513, 256, 300]
    words, _ = dt.run_multiscale(ms_prefix_cases(rng, MS_PREFIX_SHAPES))
    assert words[:, dt.M_BLOCK_BEGIN].tolist() == dt.block_prefix(totals) == [0, 2, 3, 5, 6, 9, 10]
    print('multiscale block_begin', words[:, dt.M_BLOCK_BEGIN].tolist())
    for shape in MS_PREFIX_SHAPES:
        words, _ = dt.run_multiscale(ms_prefix_cases(rng, [shape]))
        assert words[:, dt.M_BLOCK_BEGIN].tolist() == [0]
    for n in (2, 3, 5):
        for first in (0, 2):
            shapes = MS_PREFIX_SHAPES[first:first + n]
            words, _ = dt.run_multiscale(ms_prefix_cases(rng, shapes))
            assert words[:, dt.M_BLOCK_BEGIN].tolist() == dt.block_prefix([p * h * w for p, h, w in shapes])


def test_multiscale_table_limit():
    """NMSA_MULTISCALE_MAX_DESC descriptors of one output element each, all reading one shared
    map: descriptor i gathers element (i // 32, i % 32) of its own source, which holds i there"""
    n = dt.MS_MAX_DESC
    rng = np.random.default_rng(13)
    base = rng.integers(1 << 20, 1 << 30, (1, 32, 32)).astype(np.uint32)
    cases = []
    for i in range(n):
        src = base + np.uint32(i)
        src[0, i // 32, i % 32] = i
        cases.append({'src': src, 'h': 1, 'w': 1, 'row_map': i // 32, 'col_map': i % 32, 'align': 4, 'src_align': 4})
    words, outs = dt.run_multiscale(cases, shared_maps=np.arange(32))
    assert [int(o.ravel()[0]) for o in outs] == list(range(n))
    assert words[:, dt.M_BLOCK_BEGIN].tolist() == list(range(n))


def test_multiscale_map_placement():
    """two descriptors on one map region, row_map == col_map for a square output, a map whose
    last entry is the last word of the staging buffer, and n_words beyond the used words with
    garbage there"""
    rng = np.random.default_rng(14)
    H = W = 9
    square = rng.integers(0, 9, (6,))
    rows, cols = rng.integers(0, 9, (4,)), rng.integers(0, 9, (7,))
    maps = np.concatenate([square, rows, cols])                      # words 0..5 | 6..9 | 10..16
    sources = [dt.random_bits(rng, (2, H, W), size) for size in (4, 2, 8, 1)]
    shared = [{'src': sources[0], 'h': 4, 'w': 7, 'row_map': 6, 'col_map': 10},
              {'src': sources[1], 'h': 4, 'w': 7, 'row_map': 6, 'col_map': 10},
              {'src': sources[2], 'h': 6, 'w': 6, 'row_map': 0, 'col_map': 0},
              {'src': sources[3], 'h': 7, 'w': 4, 'row_map': 10, 'col_map': 6},      # the rows of one are the columns of another
              {'src': sources[0], 'h': 3, 'w': 7, 'row_map': 3, 'col_map': 10}]      # overlapping regions
    # the last map ends exactly at the last staging word (row_map + h == col_map + w == map words)
    assert shared[0]['col_map'] + shared[0]['w'] == len(maps) == shared[3]['row_map'] + shared[3]['h']
    dt.run_multiscale([dict(c) for c in shared], shared_maps=maps)
    # words the table does not use follow the maps: entries no side could index, never read
    garbage = [-1, 1 << 30, -(1 << 31), 9, 12345]
    dt.run_multiscale([dict(c) for c in shared], shared_maps=maps, tail=garbage)
