"""GPU tier: the target generators (csrc/targets.hip) off the on-wire path and at its limits.

Label dtype, alignment, W % 4, H*W % 4, max_instances and sigma select among the one-launch scan,
the classic launches with vectorised or per-element loaders, three paint kernels and two places
for the heat-map table.  Every case first asserts, through `ops.targets_route`
(`nmsa_targets_route`), the route it means to take — a case that lands elsewhere fails — and that
`ops._targets_on_wire`, which decides in Python whether the status word is SET and the workspace
kept, agrees with the query's scan bit.  Then `instance_targets` (normalised and int16 offsets, and
once on the uncleared map), `panoptic_targets` (cleared and uncleared map) and `orientation_targets` are compared bit for bit
with `oracle.instance_targets` / `oracle.naive_merge` / the numpy restatement of the orientation
rule, twice in a row on the same stream so that a table left dirty by the first round shows.

  a  dense maps: ~250 ids and > 256 (id, class) pairs per 1024-pixel workgroup (the LDS tables of
     the classic kernels hold 64 and 256: the global-atomic fallback), ~1984 ids per image
     (max_instances = 4096: four table entries per thread in rank / decide / naive ranks)
  b  sigma 14 | 15 | 20 | 64: the heat-map table in LDS, then in global memory up to the ABI's limit
  c  the 16 combinations of semantic x instance dtype
  d  label views moved off their alignment: the scan must not run, the status word must be zeroed
  e  status bits 1, 32, 64, 128 on every route, and the clean call after them
"""
import numpy as np
import pytest
import torch

from _golden import ids_from_arrays
from _gpu_support import dev
from _orientation_ref import assert_bits_equal, pack_keys, random_angles, restate

pytestmark = pytest.mark.gpu

SCAN, FAST, TILED, VECTOR, LUT_LDS, SCAN_16 = 1, 2, 4, 8, 16, 32
TORCH_OF = {np.uint8: torch.uint8, np.int16: torch.int16, np.int32: torch.int32, np.int64: torch.int64}
MAX_PER_CAT = 1 << 16


def want_route(kind, sigma, max_inst):
    """the mask `nmsa_targets_route` must report: `kind` is scan | fast | generic"""
    lut = LUT_LDS if 2 * (3 * sigma + 1) ** 2 + 1 <= 4096 else 0
    cap = -(-max_inst // 1024) * 1024
    if kind == 'scan':
        return SCAN | FAST | TILED | lut | (SCAN_16 if cap > 1024 else 0)
    return (FAST | VECTOR | lut) if kind == 'fast' else lut


def kind_of(H, W):
    return 'scan' if W % 4 == 0 else 'fast' if (H * W) % 4 == 0 else 'generic'


# ------------------------------------------------------------------------------------ content
def thing_flags(rng, NC):
    is_thing = rng.random(NC) < 0.7
    is_thing[0] = False
    is_thing[1], is_thing[2] = True, False                      # at least one of each
    return is_thing


def stuff_lut(is_thing):
    st = np.zeros((len(is_thing),), np.uint8)
    st[np.where(~is_thing)[0][1:]] = 1
    return st


def sparse_ids(rng, n, hi=65536):
    return rng.choice(np.arange(1, hi), size=n, replace=False).astype(np.int32)


def rect_maps(rng, B, H, W, NC, n_inst, id_hi=65536):
    """`n_inst` ordinary rectangles with sparse ids over a random semantic map"""
    sem = rng.integers(0, NC, (B, H, W)).astype(np.uint8)
    ins = np.zeros((B, H, W), np.int32)
    for b in range(B):
        for iid in sparse_ids(rng, n_inst, id_hi):
            ya, xa = rng.integers(0, H), rng.integers(0, W)
            yb, xb = rng.integers(ya, H) + 1, rng.integers(xa, W) + 1
            ins[b, ya:yb, xa:xb] = iid
            if rng.random() < 0.7:
                sem[b, ya:yb, xa:xb] = rng.integers(0, NC)
    return sem, ins


def dense_maps(rng, B, H, W, NC):
    """left half: 2 x 2 cells, each its own id and class, one in eight split between two classes
    (1, 2 or 3 of its pixels: majorities and ties); right half: three bands over all rows (every
    workgroup meets them) with 10 % foreign labels and 5 % holes"""
    sem = rng.integers(0, NC, (B, H, W)).astype(np.uint8)
    ins = np.zeros((B, H, W), np.int32)
    Wl = (W // 2) // 2 * 2
    ch, cw = -(-H // 2), Wl // 2
    for b in range(B):
        ids = sparse_ids(rng, ch * cw).reshape(ch, cw)
        cls = rng.integers(0, NC, (ch, cw))
        other = (cls + rng.integers(1, NC, (ch, cw))) % NC
        split = rng.random((ch, cw)) < 0.125
        up = lambda a: np.repeat(np.repeat(a, 2, axis=0), 2, axis=1)[:H, :Wl]
        bits = rng.integers(0, 2, (2 * ch, 2 * cw))[:H, :Wl].astype(bool)
        ins[b, :, :Wl] = up(ids)
        sem[b, :, :Wl] = np.where(up(split) & bits, up(other), up(cls))
        edges = np.linspace(Wl, W, 4).astype(int)
        for k, iid in enumerate(sparse_ids(rng, 3)):
            band = (slice(None), slice(edges[k], edges[k + 1]))
            ins[b][band] = np.where(rng.random(ins[b][band].shape) < 0.05, 0, iid)
            sem[b][band] = np.where(rng.random(sem[b][band].shape) < 0.1, sem[b][band], 1 + k % (NC - 1))
    return sem, ins


def patch_maps(rng, B, H, W, NC, n_inst):
    """small thing-class rectangles anywhere (at these sigmas all patches overlap), then one in
    each of two opposite corners (centers within 2 px of a corner: patches clipped on two sides).
    Among several patches the nearest center decides a pixel, so one more image holds a single
    corner instance: there the far end of the table decides the far pixels"""
    sem = rng.integers(2, NC, (B + 1, H, W)).astype(np.uint8)
    ins = np.zeros((B + 1, H, W), np.int32)
    ins[B, :3, :3] = sparse_ids(rng, 1)[0]
    sem[B, :3, :3] = 1
    for b in range(B):
        for k, iid in enumerate(sparse_ids(rng, n_inst)):
            if k == n_inst - 2:
                ya, xa, h, w = 0, 0, 3, 3
            elif k == n_inst - 1:
                ya, xa, h, w = H - 3, W - 4, 3, 4
            else:
                h, w = rng.integers(2, 7), rng.integers(2, 9)
                ya, xa = rng.integers(4, H - h - 4), rng.integers(4, W - w - 4)
            ins[b, ya:ya + h, xa:xa + w] = iid
            sem[b, ya:ya + h, xa:xa + w] = 1                    # class 1 is a thing (thing_flags)
    return sem, ins


def centers_of(ins_b):
    return [(int(ys.mean()), int(xs.mean())) for ys, xs in (np.nonzero(ins_b == i) for i in np.unique(ins_b)[1:])]


def largest_deciding_lut_index(ins, sigma):
    """the largest table index that decides a pixel of the heat-map: per pixel the smallest
    squared distance to a center whose patch covers it (the table falls with the distance)"""
    radius, best = 3 * sigma + 1, 0
    B, H, W = ins.shape
    yy, xx = np.mgrid[:H, :W]
    for b in range(B):
        d2 = np.full((H, W), np.iinfo(np.int64).max)
        for cy, cx in centers_of(ins[b]):
            inside = (np.abs(yy - cy) <= radius) & (np.abs(xx - cx) <= radius)
            d2 = np.where(inside, np.minimum(d2, (yy - cy) ** 2 + (xx - cx) ** 2), d2)
        best = max(best, int(d2[d2 < np.iinfo(np.int64).max].max()))
    return best


# ------------------------------------------------------------------------------- expectations
_EXPECT = {}


def expect(oracle, key, make, NC, sigma, thing_seed, with_orientation=True):
    """content and every reference result of a case, computed once per session and left unchanged"""
    if key not in _EXPECT:
        sem, ins = make()
        is_thing = thing_flags(np.random.default_rng(thing_seed), NC)
        stuff = stuff_lut(is_thing)
        cleared = ins.copy()
        cleared[~is_thing[sem]] = 0                             # InstanceClearStuffIDs
        thing_ids = np.where(is_thing)[0]
        e = dict(sem=sem, ins=ins, cleared=cleared, is_thing=is_thing, stuff=stuff, NC=NC, sigma=sigma)
        e['it'] = {n: oracle.instance_targets(sem, cleared, NC, is_thing, stuff, sigma, n) for n in (True, False)}
        # (the uncleared map too: there the majority vote decides between encoded and skipped)
        e['it_raw'] = oracle.instance_targets(sem, ins, NC, is_thing, stuff, sigma, True)
        e['pan'] = {which: oracle.naive_merge(sem, m, MAX_PER_CAT, thing_ids, 0, cap=16384)
                    for which, m in (('cleared', cleared), ('raw', ins))}
        e['max_segments'] = max(1, max(len(d) for _, dicts in e['pan'].values() for d in dicts))
        if with_orientation:
            e['angles'] = random_angles(cleared, np.random.default_rng(thing_seed + 1))
            e['estimate'] = np.arange(NC) % 2 == 1
            e['ori'] = restate(sem, cleared, e['angles'], e['estimate'])
        _EXPECT[key] = e
    return _EXPECT[key]


def check_instance(r, o, B, what):
    assert int(r['status'].item()) == 0, (what, int(r['status'].item()))
    assert_bits_equal(r['center'].cpu().numpy(), o['center'], (what, 'center'))
    off = r['offset'].cpu().numpy()
    assert off.dtype == o['offset'].dtype, what
    if off.dtype == np.float32:
        assert_bits_equal(off, o['offset'], (what, 'offset'))
    else:
        assert np.array_equal(off, o['offset']), (what, 'offset')
    assert np.array_equal(r['foreground'].cpu().numpy(), o['foreground']), (what, 'foreground')
    assert np.array_equal(r['center_mask'].cpu().numpy(), o['center_mask']), (what, 'center_mask')
    ne, ns = r['n_encoded'].cpu().numpy(), r['n_skipped'].cpu().numpy()
    for b in range(B):
        assert r['encoded_ids'][b, :ne[b]].cpu().tolist() == o['encoded'][b], (what, 'encoded', b)
        assert r['skipped_ids'][b, :ns[b]].cpu().tolist() == o['skipped'][b], (what, 'skipped', b)


def check_panoptic(p, want, what):
    pan, dicts = want
    assert int(p['status'].item()) == 0, (what, int(p['status'].item()))
    assert np.array_equal(p['panoptic'].cpu().numpy(), pan), what
    got = ids_from_arrays(p['n_ids'].cpu().numpy(), p['ids_pan'].cpu().numpy(), p['ids_ins'].cpu().numpy())
    assert [list(d.items()) for d in got] == [list(d.items()) for d in dicts], what


def assert_route(d_sem, d_ins, NC, sigma, max_inst, want, what):
    """the route of the call that follows, and the Python side's idea of it"""
    from nicr_mt_scene_analysis_amd import ops
    B, H, W = d_sem.shape
    got = ops.targets_route(d_sem, d_ins, NC, sigma, max_inst)
    assert got == want, (what, f'route {got:#x}, wanted {want:#x}')
    assert ops._targets_on_wire(d_sem, d_ins, H, W, NC) == bool(got & SCAN), (what, got)


def run_all(e, d_sem, d_cleared, d_raw, max_inst, want, what, rounds=2):
    """every generator on one stream, `rounds` times in a row, each result exact"""
    from nicr_mt_scene_analysis_amd import ops
    NC, sigma, B = e['NC'], e['sigma'], e['sem'].shape[0]
    th, st = dev(e['is_thing'].astype(np.uint8)), dev(e['stuff'])
    for d_ins in (d_cleared, d_raw):
        assert_route(d_sem, d_ins, NC, sigma, max_inst, want, what)
    if 'ori' in e:
        keys, n_keys, bit = pack_keys(e['angles'])
        d_est, d_keys, d_nk, d_bit = dev(e['estimate'].astype(np.uint8)), dev(keys), dev(n_keys), dev(bit)
        flags = np.array([[int(k) in e['ori'][2][b] for k in keys[b]] for b in range(B)], np.uint8)
    for rnd in range(rounds):
        for normalized in (True, False):
            r = ops.instance_targets(d_sem, d_cleared, NC, th, st, sigma, normalized, max_instances=max_inst)
            check_instance(r, e['it'][normalized], B, (what, rnd, 'instance', normalized))
        r = ops.instance_targets(d_sem, d_raw, NC, th, st, sigma, True, max_instances=max_inst)
        check_instance(r, e['it_raw'], B, (what, rnd, 'instance', 'uncleared'))
        for which, d_ins in (('cleared', d_cleared), ('raw', d_raw)):
            p = ops.panoptic_targets(d_sem, d_ins, NC, th, MAX_PER_CAT, 0, max_instances=max_inst,
                                     max_segments=e['max_segments'])
            check_panoptic(p, e['pan'][which], (what, rnd, 'panoptic', which))
        if 'ori' in e:
            r = ops.orientation_targets(d_sem, d_cleared, NC, d_est, d_keys, d_nk, d_bit, max_instances=max_inst)
            assert int(r['status'].item()) == 0, (what, rnd, 'orientation')
            assert (r['foreground'].cpu().numpy() == e['ori'][1]).all(), (what, rnd, 'orientation')
            assert_bits_equal(r['orientation'].cpu().numpy(), e['ori'][0], (what, rnd, 'orientation'))
            assert (r['present'].cpu().numpy() == flags).all(), (what, rnd, 'orientation')


def run_plain(e, max_inst, what):
    """the case in the on-wire dtypes at its own geometry: the route follows from H and W"""
    B, H, W = e['sem'].shape
    run_all(e, dev(e['sem']), dev(e['cleared']), dev(e['ins']), max_inst,
            want_route(kind_of(H, W), e['sigma'], max_inst), what)


# ========================================================================================== a
@pytest.mark.parametrize('H,W', [(64, 248), (64, 250), (63, 251)])
def test_dense_maps_on_every_front_end(oracle, H, W):
    """~1984 ids per image, ~250 per workgroup of the classic kernels: both LDS tables of
    k_tg_presence / k_tg_stats overflow into global atomics, rank / decide / naive ranks run four
    entries per thread, the scan (the control) its 16-slot instantiation"""
    B, NC, sigma = 2, 19, 2
    e = expect(oracle, ('dense', H, W), lambda: dense_maps(np.random.default_rng(9100 + W), B, H, W, NC),
               NC, sigma, 9200)
    per_image = [len(np.unique(e['ins'][b])) - 1 for b in range(B)]
    assert all(1900 <= n <= 2000 for n in per_image), per_image
    rows_per_wg = -(-1024 // W)                                 # a 1024-pixel chunk of the classic kernels
    assert (rows_per_wg // 2) * ((W // 2) // 2) > 64            # ids per chunk > TG_H1
    assert not np.array_equal(e['ins'][0], e['ins'][1])
    run_plain(e, 4096, ('dense', H, W))


@pytest.mark.parametrize('H,W', [(40, 64), (40, 62), (39, 61)])
def test_ordinary_maps_with_small_tables(oracle, H, W):
    """20 rectangles, max_instances = 64: the 1024-entry instantiations on the same three routes"""
    B, NC, sigma = 2, 9, 3
    e = expect(oracle, ('rects', H, W), lambda: rect_maps(np.random.default_rng(9300 + W), B, H, W, NC, 20),
               NC, sigma, 9400)
    run_plain(e, 64, ('rects', H, W))


# ========================================================================================== b
def test_gauss_lut_route_bit_flips_between_sigma_14_and_15():
    from nicr_mt_scene_analysis_amd import ops
    sem = torch.zeros((1, 48, 64), dtype=torch.uint8, device='cuda')
    ins = torch.zeros((1, 48, 64), dtype=torch.int32, device='cuda')
    assert ops.targets_route(sem, ins, 5, 14) & LUT_LDS
    assert not ops.targets_route(sem, ins, 5, 15) & LUT_LDS
    assert not ops.targets_route(sem, ins, 5, 64) & LUT_LDS


@pytest.mark.parametrize('H,W', [(48, 64), (48, 62), (47, 61)])
@pytest.mark.parametrize('sigma', [14, 15, 20])
def test_heat_map_table_in_and_out_of_lds(oracle, sigma, H, W):
    """six instances per image, two of them in corners, and an image with one; from sigma = 15 the three paint kernels read the
    table from global memory, and pixels further than sqrt(4096) from a center index past what the
    LDS copy held"""
    B, NC = 2, 6
    e = expect(oracle, ('patch', sigma, H, W),
               lambda: patch_maps(np.random.default_rng(9500 + W), B, H, W, NC, 6), NC, sigma, 9600,
               with_orientation=False)
    for b in range(B):
        assert len(e['it'][True]['encoded'][b]) == 6            # every patch is painted
        centers = centers_of(e['ins'][b])
        assert min(max(cy, cx) for cy, cx in centers) <= 2 and min(max(H - 1 - cy, W - 1 - cx) for cy, cx in centers) <= 2
    assert len(e['it'][True]['encoded'][B]) == 1
    # entries past the LDS copy's 4096 decide pixels from sigma = 15 on
    assert (largest_deciding_lut_index(e['ins'], sigma) >= 4096) == (sigma >= 15)
    run_plain(e, 64, ('patch', sigma, H, W))


@pytest.mark.parametrize('H,W', [(48, 64), (48, 62), (47, 61)])
def test_heat_map_table_at_the_largest_sigma(oracle, H, W):
    """sigma = 64, the ABI's limit: every pixel lies inside every patch (radius 193), the table has
    74499 entries; three instances, and an image with one"""
    B, NC, sigma = 1, 6, 64
    e = expect(oracle, ('patch', sigma, H, W),
               lambda: patch_maps(np.random.default_rng(9700 + W), B, H, W, NC, 3), NC, sigma, 9600,
               with_orientation=False)
    assert (e['it'][True]['center'] > 0).all() and len(e['it'][True]['encoded'][0]) == 3
    assert largest_deciding_lut_index(e['ins'], sigma) > 5000
    run_plain(e, 64, ('patch', sigma, H, W))


# ========================================================================================== c
DTYPES = (np.uint8, np.int16, np.int32, np.int64)
_REFERENCE_RUN = {}


def _dtype_case(oracle):
    return expect(oracle, ('dtypes',),
                  lambda: rect_maps(np.random.default_rng(9800), 2, 24, 36, 7, 14, id_hi=256), 7, 2, 9900)


def _all_bits(e, d_sem, d_cleared, d_raw):
    """every output of every generator as one list of host arrays"""
    from nicr_mt_scene_analysis_amd import ops
    NC, sigma, B = e['NC'], e['sigma'], e['sem'].shape[0]
    th, st = dev(e['is_thing'].astype(np.uint8)), dev(e['stuff'])
    keys, n_keys, bit = pack_keys(e['angles'])
    out = []
    for normalized in (True, False):
        r = ops.instance_targets(d_sem, d_cleared, NC, th, st, sigma, normalized, max_instances=256)
        ne, ns = r['n_encoded'].cpu(), r['n_skipped'].cpu()
        out += [r[k].cpu().numpy() for k in ('center', 'offset', 'foreground', 'center_mask', 'n_encoded',
                                             'n_skipped', 'status')]
        out += [r['encoded_ids'][b, :int(ne[b])].cpu().numpy() for b in range(B)]
        out += [r['skipped_ids'][b, :int(ns[b])].cpu().numpy() for b in range(B)]
    for d_ins in (d_cleared, d_raw):
        p = ops.panoptic_targets(d_sem, d_ins, NC, th, MAX_PER_CAT, 0, max_instances=256,
                                 max_segments=e['max_segments'])
        n = p['n_ids'].cpu()
        out += [p['panoptic'].cpu().numpy(), n.numpy(), p['status'].cpu().numpy()]
        out += [p[k][b, :int(n[b])].cpu().numpy() for b in range(B) for k in ('ids_pan', 'ids_ins')]
    r = ops.orientation_targets(d_sem, d_cleared, NC, dev(e['estimate'].astype(np.uint8)), dev(keys),
                                dev(n_keys), dev(bit), max_instances=256)
    out += [r[k].cpu().numpy() for k in ('orientation', 'foreground', 'present', 'status')]
    return out


@pytest.mark.parametrize('ins_dtype', DTYPES, ids=lambda d: 'ins_' + np.dtype(d).name)
@pytest.mark.parametrize('sem_dtype', DTYPES, ids=lambda d: 'sem_' + np.dtype(d).name)
def test_every_label_dtype(oracle, sem_dtype, ins_dtype):
    """one map with ids <= 255 in the 16 dtype combinations the ABI accepts: the same bits as the
    oracle and as the (uint8, int32) run; only that one may take the scan"""
    from nicr_mt_scene_analysis_amd import ops
    e = _dtype_case(oracle)
    assert e['ins'].max() <= 255 and len(np.unique(e['ins'])) > 8
    wire = (sem_dtype, ins_dtype) == (np.uint8, np.int32)
    want = want_route('scan' if wire else 'generic', e['sigma'], 256)
    d_sem = dev(e['sem'].astype(sem_dtype))
    d_cleared, d_raw = dev(e['cleared'].astype(ins_dtype)), dev(e['ins'].astype(ins_dtype))
    # InstanceClearStuffIDs in these dtypes
    d_work = d_raw.clone()
    ops.instance_clear_stuff(d_sem, d_work, dev((~e['is_thing']).astype(np.uint8)))
    assert d_work.dtype == TORCH_OF[ins_dtype] and torch.equal(d_work, d_cleared)
    run_all(e, d_sem, d_cleared, d_raw, 256, want, (np.dtype(sem_dtype).name, np.dtype(ins_dtype).name))
    if 'bits' not in _REFERENCE_RUN:
        _REFERENCE_RUN['bits'] = _all_bits(e, dev(e['sem']), dev(e['cleared']), dev(e['ins']))
    got = _all_bits(e, d_sem, d_cleared, d_raw)
    assert len(got) == len(_REFERENCE_RUN['bits'])
    for i, (a, b) in enumerate(zip(got, _REFERENCE_RUN['bits'])):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), i


# ========================================================================================== d
def shifted(a, torch_dtype, shift_elems, pad_elems=8):
    """`a` as a contiguous view that starts `shift_elems` elements into a larger flat buffer"""
    flat = torch.zeros((a.size + pad_elems,), dtype=torch_dtype, device='cuda')
    view = flat[shift_elems:shift_elems + a.size].view(*a.shape)
    view.copy_(dev(a))
    assert view.is_contiguous() and view.data_ptr() == flat.data_ptr() + shift_elems * flat.element_size()
    return view


def poison_small_blocks():
    """small blocks full of ones handed back to the allocator: a `torch.empty` status word that
    nobody zeroes reads as non-zero"""
    blocks = [torch.full((128,), -1, dtype=torch.int32, device='cuda') for _ in range(256)]
    torch.cuda.synchronize()
    del blocks


@pytest.mark.parametrize('which,shift_bytes', [('semantic', 1), ('semantic', 2), ('semantic', 3),
                                               ('instance', 4), ('instance', 8), ('instance', 12)])
def test_misaligned_label_views_leave_the_scan(oracle, which, shift_bytes):
    """on-wire content whose semantic base is not 4-byte or whose instance base is not 16-byte
    aligned: the C side and `ops._targets_on_wire` must both say off-wire, so the status word is a
    zeroed one (exactly 0 although the allocator's free blocks are full of ones) and the cached
    workspace is not marked clean — the aligned call behind it is exact too"""
    from nicr_mt_scene_analysis_amd import ops
    B, H, W, NC, sigma = 2, 32, 48, 8, 3
    e = expect(oracle, ('wire',), lambda: rect_maps(np.random.default_rng(10000), B, H, W, NC, 12), NC, sigma, 10100)
    run_all(e, dev(e['sem']), dev(e['cleared']), dev(e['ins']), 64, want_route('scan', sigma, 64), 'aligned', rounds=1)
    if which == 'semantic':
        d_sem = shifted(e['sem'], torch.uint8, shift_bytes)
        d_cleared, d_raw = dev(e['cleared']), dev(e['ins'])
        assert d_sem.data_ptr() % 4 == shift_bytes
    else:
        d_sem = dev(e['sem'])
        d_cleared = shifted(e['cleared'], torch.int32, shift_bytes // 4)
        d_raw = shifted(e['ins'], torch.int32, shift_bytes // 4)
        assert d_cleared.data_ptr() % 16 == shift_bytes and d_raw.data_ptr() % 16 == shift_bytes
    for d_ins in (d_cleared, d_raw):
        assert not ops.targets_route(d_sem, d_ins, NC, sigma, 64) & SCAN
        assert not ops._targets_on_wire(d_sem, d_ins, H, W, NC)
    poison_small_blocks()
    run_all(e, d_sem, d_cleared, d_raw, 64, want_route('generic', sigma, 64), (which, shift_bytes))
    run_all(e, dev(e['sem']), dev(e['cleared']), dev(e['ins']), 64, want_route('scan', sigma, 64),
            ('aligned after', which, shift_bytes), rounds=1)


# ========================================================================================== e
STATUS_GEOMETRIES = [(36, 40), (36, 42), (35, 41)]
ST_NC, ST_SIGMA, ST_B = 6, 2, 2


def _clean_case(oracle, H, W):
    return expect(oracle, ('clean', H, W),
                  lambda: rect_maps(np.random.default_rng(10200 + W), ST_B, H, W, ST_NC, 20, id_hi=32768),
                  ST_NC, ST_SIGMA, 10300)               # (ids that an int16 map can hold)


def _clean_after(e, max_inst, sem_dtype, ins_dtype, what):
    """the next call on the same stream and workspace key (B, classes, max_instances) is clean
    and exact"""
    H, W = e['sem'].shape[1:]
    wire = (sem_dtype, ins_dtype) == (np.uint8, np.int32)
    run_all(e, dev(e['sem'].astype(sem_dtype)), dev(e['cleared'].astype(ins_dtype)), dev(e['ins'].astype(ins_dtype)),
            max_inst, want_route(kind_of(H, W) if wire else 'generic', ST_SIGMA, max_inst), what, rounds=1)


def _status_of_all(sem, ins, max_inst, max_segments=2048):
    """status word of the three generators for one pair of device maps"""
    from nicr_mt_scene_analysis_amd import ops
    B = sem.shape[0]
    keys = torch.zeros((B, 64), dtype=torch.int32, device='cuda')
    keys[:, 0] = 5
    n_keys = torch.ones((B,), dtype=torch.int32, device='cuda')
    bit = torch.ones((B, 64, 2), dtype=torch.float32, device='cuda')
    out = {'instance': ops.instance_targets(sem, ins, ST_NC, None, None, ST_SIGMA, True, max_instances=max_inst),
           'panoptic': ops.panoptic_targets(sem, ins, ST_NC, None, MAX_PER_CAT, 0, max_instances=max_inst,
                                            max_segments=max_segments),
           'orientation': ops.orientation_targets(sem, ins, ST_NC, None, keys, n_keys, bit, max_instances=max_inst)}
    return {k: int(r['status'].item()) for k, r in out.items()}


@pytest.mark.parametrize('H,W', STATUS_GEOMETRIES)
def test_status_bit_1_starts_past_the_table(oracle, H, W):
    """one id per pixel over the first 1024 pixels with max_instances = 1024 fills the tables to
    the last entry and is clean and exact; one id more raises bit 1 in all three generators; the
    clean call behind it is exact"""
    def full(n_ids):
        def make():
            rng = np.random.default_rng(10400 + W)
            sem = rng.integers(0, ST_NC, (ST_B, H, W)).astype(np.uint8)
            ins = np.zeros((ST_B, H, W), np.int32)
            ins[0].reshape(-1)[:n_ids] = sparse_ids(rng, n_ids)
            ins[1, 3:9, 2:30] = 77
            return sem, ins
        return make
    e = expect(oracle, ('full', H, W), full(1024), ST_NC, ST_SIGMA, 10500)
    assert len(np.unique(e['ins'][0])) - 1 == 1024
    run_plain(e, 1024, ('1024 ids', H, W))
    sem, ins = full(1025)()
    assert len(np.unique(ins[0])) - 1 == 1025
    d_sem, d_ins = dev(sem), dev(ins)
    assert_route(d_sem, d_ins, ST_NC, ST_SIGMA, 1024, want_route(kind_of(H, W), ST_SIGMA, 1024), '1025 ids')
    status = _status_of_all(d_sem, d_ins, 1024, max_segments=4096)
    assert all(s == 1 for s in status.values()), status
    run_plain(e, 1024, ('1024 ids after 1025', H, W))


@pytest.mark.parametrize('H,W', STATUS_GEOMETRIES)
def test_status_bit_128_starts_past_max_segments(oracle, H, W):
    """max_segments equal to the largest id dict is clean and exact (run_all sizes it so); one
    segment fewer raises bit 128, n_ids stops at max_segments and the lists keep the dict's first
    entries; the clean call behind it is exact"""
    from nicr_mt_scene_analysis_amd import ops
    e = _clean_case(oracle, H, W)
    _clean_after(e, 64, np.uint8, np.int32, ('before', H, W))
    pan, dicts = e['pan']['raw']
    ms = max(len(d) for d in dicts)
    d_sem, d_ins, th = dev(e['sem']), dev(e['ins']), dev(e['is_thing'].astype(np.uint8))
    assert_route(d_sem, d_ins, ST_NC, ST_SIGMA, 64, want_route(kind_of(H, W), ST_SIGMA, 64), 'bit 128')
    p = ops.panoptic_targets(d_sem, d_ins, ST_NC, th, MAX_PER_CAT, 0, max_instances=64, max_segments=ms)
    check_panoptic(p, (pan, dicts), ('max_segments = largest dict', H, W))
    p = ops.panoptic_targets(d_sem, d_ins, ST_NC, th, MAX_PER_CAT, 0, max_instances=64, max_segments=ms - 1)
    assert int(p['status'].item()) == 128
    assert np.array_equal(p['panoptic'].cpu().numpy(), pan)      # the map does not depend on the lists
    n = p['n_ids'].cpu().numpy()
    got = ids_from_arrays(n, p['ids_pan'].cpu().numpy(), p['ids_ins'].cpu().numpy())
    for b, d in enumerate(dicts):
        assert n[b] == min(len(d), ms - 1)
        assert list(got[b].items()) == list(d.items())[:ms - 1]
    _clean_after(e, 64, np.uint8, np.int32, ('after', H, W))


@pytest.mark.parametrize('H,W', STATUS_GEOMETRIES)
@pytest.mark.parametrize('dtype', [np.int16, np.int32, np.int64], ids=lambda d: np.dtype(d).name)
def test_status_bits_32_and_64_for_negative_values(oracle, dtype, H, W):
    """a negative id in a signed instance map raises bit 32, a negative label on an instance pixel
    of a signed semantic map bit 64 — alone; the clean call behind each is exact"""
    e = _clean_case(oracle, H, W)
    assert e['ins'].max() < 32768
    y, x = np.argwhere(e['ins'][1] > 0)[len(np.argwhere(e['ins'][1] > 0)) // 2]
    # bit 32: semantic uint8, instance `dtype`
    ins = e['ins'].astype(dtype)
    ins[1, y, x] = -3
    d_sem, d_ins = dev(e['sem']), dev(ins)
    wire = dtype == np.int32
    assert_route(d_sem, d_ins, ST_NC, ST_SIGMA, 64,
                 want_route(kind_of(H, W) if wire else 'generic', ST_SIGMA, 64), 'negative id')
    status = _status_of_all(d_sem, d_ins, 64)
    assert all(s == 32 for s in status.values()), status
    _clean_after(e, 64, np.uint8, dtype, ('after a negative id', H, W))
    # bit 64: semantic `dtype`, instance int32
    sem = e['sem'].astype(dtype)
    sem[1, y, x] = -1
    d_sem, d_ins = dev(sem), dev(e['ins'])
    assert_route(d_sem, d_ins, ST_NC, ST_SIGMA, 64, want_route('generic', ST_SIGMA, 64), 'negative label')
    status = _status_of_all(d_sem, d_ins, 64)
    assert all(s == 64 for s in status.values()), status
    _clean_after(e, 64, dtype, np.int32, ('after a negative label', H, W))
