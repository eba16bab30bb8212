"""GPU tier: the capped-grid kernels of the model side past the first trip of their grid-stride loops.

These kernels launch min(items, k x compute units) workgroups and walk the rest of the work in a loop.
On a whole MI355X the cap is 2048 workgroups (1024 for the LayerNorm-transpose backward), which none of
the edge-sized shapes of the sibling test files reaches, while the shapes of a training step do.
`NMSA_ASSUME_CUS` (csrc/api.hip `device_geometry`, read at every call) shrinks the cap instead of
growing the tensors: with ONE compute unit assumed the caps are 8 and 4 workgroups and small shapes
run many trips.  Every kernel runs under assumed counts of 1, 3 (strides of 24 / 12 workgroups: no power
of two) and the device's own count (one trip: the baseline).

Held under every count: what is computed per element is bit-identical across the three counts; every
result equals the float64 oracle cast once on the modules' exact-tier inputs (sums across workgroups
included: those inputs make every sum exact in any order) and lies within the modules' own `bounds` on
normal inputs.  Oracles, input makers and tolerances are those of the sibling files (test_fusion.py,
test_context_module.py, test_mlp_decoder.py, test_normal_task.py, test_upsampling.py); none is new.

Launch geometry the shapes are picked from, and the trips reached under one assumed compute unit
(`assert_trips` holds every line below: each workgroup makes `full` >= 3 trips, and a ragged trip
follows in which only `rest` != 0 workgroups have an item):

  csrc/ln_transpose.hip   an item is a tile of 32 pixels of one image: items = B * ceil(P / 32).
      B = 2, P = 408 (vector route; 13 tiles per image, the last one of 24 pixels) and P = 411 (odd:
      element route): 26 tiles.  k_lnt_fwd, cap 8: 3 trips + 2 workgroups in a 4th.  k_lnt_bwd, cap 4:
      6 trips + 2 workgroups in a 7th; the partials line [2][C] of a workgroup is written on its first
      trip and added to on the others, once per chunk of 128 channels (C = 160: two chunks), and
      k_lnt_reduce sums nwg = cap lines (read back from the workspace size).  3 assumed: 24 / 12
      workgroups, 2 of them make one trip more.
  csrc/context_module.hip   k_ppm_pool_fwd, k_ppm_upcat_bwd: a wave owns a plane, 4 planes per
      workgroup, items = ceil(planes / 4) with planes = B * C / B * sum Cr, uniform trip count with
      barriers inside.  B = 2, C = 51, three branches of Cr = 17: 102 planes = 26 workgroup items, cap 8:
      3 trips + 2 workgroups in a 4th, the last of which holds planes 100, 101 and two waves without a
      plane.  (Three branches, not four: B * 4 * Cr is always a multiple of four planes.)
      k_ppm_upcat_fwd: an item is 1024 pixels of one output plane, items = B * (C + sum Cr) *
      ceil(HW / 1024) = 204 (8x16) and 612 (48x64), cap 8: 25 / 76 trips + 4 workgroups.
      k_ppm_pool_bwd launches one item per wave, no cap: it rides along in the comparisons.
  csrc/mlp_decoder.hip   k_mlpdec_upcat_fwd: an item is 256 * VEC pixels of one output plane (VEC = 4
      float32 / 8 half on the vector route, 1 on the element route), items = B * sum c * ceil(HW /
      (256 VEC)).  (3, 2, 1, 5) channels at 40x56: 66 (float32), 44 (half), 198 (element) items, cap 8:
      8 / 5 / 24 trips + 2 / 4 / 6 workgroups.  k_mlpdec_upcat_bwd: an item is 256 source pixels of one
      branch's flat array, items = sum over the wanted branches with a factor above 1 of
      ceil(B c h w / 256).  (64, 3) at 36x40: 180 items; (3, 5, 10, 2) at 40x56: 51 items, and 45 with
      the middle branch unwanted (`first[]` then holds a branch without items).
  csrc/normal.hip   k_normal_valid_mask, k_rmse: a lane owns a unit of 4 pixels, items (per lane) =
      B * ceil(HW / 4) over cap * 256 lanes.  B = 2 at 95x131 (HW % 4 = 1: per-pixel loads) and 96x132
      (16-byte loads): 6224 / 6336 units over 2048 lanes: 3 trips + 80 / 192 lanes in a 4th.
  csrc/upsampling.hip   an item is 256 lane units of one plane, items = B * C * chunks.  B = 2, C = 13,
      9x8 (vector route) and 9x7 (one-pixel route): 26 items, cap 8: 3 trips + 2 workgroups.
"""
import numpy as np
import pytest
import torch

from nicr_mt_scene_analysis_amd import _lib as L
from nicr_mt_scene_analysis_amd import ops
from nicr_mt_scene_analysis_amd.testing import context_ref as RC
from nicr_mt_scene_analysis_amd.testing import fusion_ref as RF
from nicr_mt_scene_analysis_amd.testing import mlp_decoder_ref as RM
from nicr_mt_scene_analysis_amd.testing import synthetic as syn
from nicr_mt_scene_analysis_amd.testing import upsampling_ref as RU

from _gpu_support import assume_cus  # noqa: F401
import test_context_module as TC
import test_fusion as TF
import test_mlp_decoder as TM
import test_normal_task as TN
import test_upsampling as TU

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = (F32, BF16, F16)
COUNTS = (1, 3, None)                       # assumed compute units; None: the device's own count
# workgroups per compute unit of the capped grids
LNT_FWD_BLOCKS_PER_CU = 8                   # csrc/ln_transpose.hip LNT_FWD_BLOCKS_PER_CU
LNT_BWD_BLOCKS_PER_CU = 4                   # csrc/ln_transpose.hip LNT_BWD_BLOCKS_PER_CU
PPM_BLOCKS_PER_CU = 8                       # csrc/context_module.hip PPM_BLOCKS_PER_CU
MLD_BLOCKS_PER_CU = 8                       # csrc/mlp_decoder.hip MLD_BLOCKS_PER_CU
NRM_BLOCKS_PER_CU = 8                       # csrc/normal.hip NRM_BLOCKS_PER_CU
UP_BLOCKS_PER_CU = 8                        # csrc/upsampling.hip UP_BLOCKS_PER_CU
LNT_TILE = 32                               # csrc/ln_transpose.hip LNT_TP: pixels of a tile
PPM_WAVES = 4                               # csrc/context_module.hip PPM_WAVES: planes of a workgroup
PPM_CAT_ITEM = 1024                         # csrc/context_module.hip PPM_THREADS * PPM_CAT_RUN
THREADS = 256                               # MLD_THREADS, NRM_THREADS, UP_THREADS: lanes of a workgroup
UP_TILE_H = 8                               # csrc/upsampling.hip UP_TILE_H: input rows a lane walks


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------ the switch
def trips(items, per_cu, cus):
    """(workgroups, trips every workgroup makes, workgroups with an item in the trip after those)"""
    grid = min(items, per_cu * cus)
    return grid, items // grid, items % grid


def assert_trips(items, per_cu, what):
    """non-vacuity.  One compute unit assumed: every workgroup makes at least 3 trips and the last
    trip is ragged (some workgroups have an item, some have none).  Three: more than one trip, the
    last one ragged.  The device's own count: one trip."""
    grid, full, rest = trips(items, per_cu, 1)
    assert grid == per_cu and full >= 3 and rest != 0, (what, items, grid, full, rest)
    grid, full, rest = trips(items, per_cu, 3)
    assert grid == 3 * per_cu and full >= 1 and rest != 0, (what, items, grid, full, rest)
    own = torch.cuda.get_device_properties(0).multi_processor_count
    assert trips(items, per_cu, own) == (items, 1, 0), (what, items, own)


def assert_same_bits(results, keys, tag):
    """`results`: one dict per assumed count; tensors (or tuples of tensors, None allowed) under `keys`"""
    base = results[0]
    for other in results[1:]:
        for key in keys:
            a, b = base[key], other[key]
            a, b = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
            assert len(a) == len(b), (tag, key)
            for i, (ta, tb) in enumerate(zip(a, b)):
                assert (ta is None) == (tb is None), (tag, key, i)
                assert ta is None or torch.equal(ta, tb), (tag, key, i)


# ------------------------------------------------------------------------------ LayerNorm + NHWC -> NCHW
LNT_B = 2
LNT_PS = ((408, False), (408, True), (411, False))      # (P, x one element off 16 bytes)


def lnt_run(x, gamma, beta, eps, add, gy, dy, element, need=(True, True, True)):
    xd, gd, bd, ad, gyd = TF.dev(x, gamma, beta, add, gy)
    if element:
        xd = TF.off_by_one(xd)
    y, mean, rstd = ops.ln_nhwc_to_nchw(xd, gd, bd, eps, add=ad, out_dtype=dy, save_stats=True)
    gx, gg, gb = ops.ln_nhwc_to_nchw_backward(gyd, xd, gd, mean, rstd, *need)
    return {'y': y, 'mean': mean, 'rstd': rstd, 'gx': gx, 'ggamma': gg, 'gbeta': gb,
            'route': ops.ln_nhwc_to_nchw_route(xd, y)}


def lnt_workgroups(B, P, C):
    """the backward grid, read back from the workspace size: nwg lines of [2][C] floats"""
    nbytes = L.lib().nmsa_ln_nhwc_nchw_bwd_workspace_bytes(B, P, C)
    assert nbytes % (2 * C * 4) == 0
    return nbytes // (2 * C * 4)


@pytest.mark.parametrize('C', (64, 160))
@pytest.mark.parametrize('pair', TF.PAIRS, ids=TF.PAIR_IDS)
def test_ln_transpose_over_several_trips(assume_cus, pair, C):
    """k_lnt_fwd, k_lnt_bwd, k_lnt_reduce.  C = 160: two chunks of 128 channels, so a workgroup's
    partials line is written (first trip) or added to (later trips) once per chunk"""
    dx, dy = pair
    B = LNT_B
    for P, element in LNT_PS:
        tiles = B * cdiv(P, LNT_TILE)
        assert P % LNT_TILE != 0                                    # every image ends in a partial tile
        assert_trips(tiles, LNT_FWD_BLOCKS_PER_CU, ('k_lnt_fwd', P))
        assert_trips(tiles, LNT_BWD_BLOCKS_PER_CU, ('k_lnt_bwd', P))
        want_route = TF.expected_route(P, C, dx, dy, element)
        assert want_route == (TF.ELEMENT if element or P % 2 else TF.VECTOR)
        for tier in ('exact', 'normal'):
            tag = (dx, dy, C, P, element, tier)
            if tier == 'exact':
                x, gamma, beta, add, gy = TF.exact_inputs(B, P, C, dx, dy, seed=C + P)
                eps = 0.0
            else:
                x, gamma, beta, gy, add = RF.make_inputs('normal', B, P, C, seed=C + P, dtype=dx)
                gy, add, eps = gy.to(dy), add.to(dy), 1e-5
            ref = RF.reference64(x, gamma, beta, eps, add, gy)
            bd = RF.bounds(x, gamma, beta, eps, add, gy, dtype_y=dy, dtype_x=dx) if tier == 'normal' else None
            results = []
            for assumed in COUNTS:
                cus = assume_cus(assumed)
                assert lnt_workgroups(B, P, C) == min(tiles, LNT_BWD_BLOCKS_PER_CU * cus), (tag, assumed)
                if assumed is not None:
                    assert lnt_workgroups(B, P, C) == LNT_BWD_BLOCKS_PER_CU * assumed
                got = lnt_run(x, gamma, beta, eps, add, gy, dy, element)
                assert got['route'] == want_route, (tag, assumed)
                results.append(got)
                if tier == 'exact':
                    assert torch.equal(got['y'].cpu(), ref['y'].to(dy)), (tag, assumed)      # cast once
                    assert torch.equal(got['mean'].cpu().double().view(B, P), ref['mean']), (tag, assumed)
                    assert torch.equal(got['rstd'].cpu().double().view(B, P), ref['rstd']), (tag, assumed)
                    assert torch.equal(got['ggamma'].cpu().double(), ref['ggamma']), (tag, assumed)
                    assert torch.equal(got['gbeta'].cpu().double(), ref['gbeta']), (tag, assumed)
                    if C & (C - 1) == 0:                            # mean_c(a) is exact: a division by 2^k
                        assert torch.equal(got['gx'].cpu(), ref['gx'].to(dx)), (tag, assumed)
                    # gx only: no partials; ggamma / gbeta only: no gx and no phase A
                    only_gx = lnt_run(x, gamma, beta, eps, add, gy, dy, element, (True, False, False))
                    assert only_gx['ggamma'] is None and only_gx['gbeta'] is None
                    assert torch.equal(only_gx['gx'], got['gx']), (tag, assumed)
                    sums = lnt_run(x, gamma, beta, eps, add, gy, dy, element, (False, True, True))
                    assert sums['gx'] is None
                    assert torch.equal(sums['ggamma'], got['ggamma']), (tag, assumed)
                    assert torch.equal(sums['gbeta'], got['gbeta']), (tag, assumed)
                else:
                    for key in ('y', 'gx', 'ggamma', 'gbeta'):
                        ratio = RF.worst_ratio(got[key], ref[key], bd[key])
                        print(tag, assumed, key, '%.3f of the bound' % ratio)
                        assert ratio <= 1.0, (tag, assumed, key, ratio)
            assert_same_bits(results, ('y', 'mean', 'rstd', 'gx'), tag)


# ------------------------------------------------------------------------------ context module
PPM_B, PPM_C, PPM_CR = 2, 51, 17
PPM_EXACT_SIZES = ((2, 2), (4, 4), (8, 8))              # of the exact tier's bins (1, 2, 4, 8)
PPM_NORMAL_SIZES = ((2, 2), (3, 3), (6, 6))             # of the bounds tier's bins (1, 2, 3, 6)


@pytest.mark.parametrize('mode', TC.MODES)
@pytest.mark.parametrize('dtype', DTYPES, ids=('f32', 'bf16', 'f16'))
@pytest.mark.parametrize('hw,lds', (((8, 16), True), ((48, 64), False)), ids=('8x16-lds', '48x64-global'))
def test_context_module_over_several_trips(assume_cus, hw, lds, dtype, mode):
    """k_ppm_pool_fwd and k_ppm_upcat_bwd (a barrier-synchronised loop that reuses a wave's LDS plane
    and row sums; the last trip's last workgroup has two waves with a plane and two without),
    k_ppm_upcat_fwd (the plane -> branch search per item), and k_ppm_pool_bwd alongside"""
    B, C, CR = PPM_B, PPM_C, PPM_CR
    n = len(PPM_EXACT_SIZES)
    for planes, what in ((B * C, 'k_ppm_pool_fwd'), (B * n * CR, 'k_ppm_upcat_bwd')):
        assert_trips(cdiv(planes, PPM_WAVES), PPM_BLOCKS_PER_CU, what)
        assert planes % PPM_WAVES != 0                  # the last workgroup: valid and invalid waves
    assert_trips(B * (C + n * CR) * cdiv(hw[0] * hw[1], PPM_CAT_ITEM), PPM_BLOCKS_PER_CU, 'k_ppm_upcat_fwd')
    tiers = (('exact', PPM_EXACT_SIZES), ('normal', PPM_NORMAL_SIZES)) if lds else (('normal', PPM_NORMAL_SIZES),)
    for tier, sizes in tiers:
        tag = (hw, dtype, mode, tier)
        assert ops.ppm_route(hw, sizes) == (TC.LDS if lds else TC.GLOBAL)
        assert tier != 'exact' or RC.is_power_of_two_geometry(hw, sizes)
        x, ys, g_out, gps = RC.make_inputs(B, C, CR, hw, sizes, seed=hw[0], dtype=dtype, integer=tier == 'exact')
        ref = RC.reference64(x, sizes, ys, mode, g_out, gps)
        bd = RC.bounds(x, sizes, ys, mode, g_out, gps, dtype=dtype) if tier == 'normal' else None
        shapes = [tuple(y.shape) for y in ys]
        results = []
        for assumed in COUNTS:
            assume_cus(assumed)
            got = TC.run_ops(x, ys, g_out, gps, sizes, mode)
            # the middle branch unwanted: its planes are waves without work in the middle of a trip
            got['gys_part'] = ops.ppm_upsample_concat_backward(g_out.to(DEV), C, shapes, mode, need=(True, False, True))
            results.append(got)
            assert got['gys_part'][1] is None
            for i in (0, 2):
                assert torch.equal(got['gys_part'][i], got['gys'][i]), (tag, assumed, i)
            if tier == 'exact':
                for key, g, r in TC.pairs(got, ref):
                    assert g.dtype == dtype and torch.equal(g.cpu(), r.to(dtype)), (tag, assumed, key)
            else:
                worst = {key: RC.worst_ratio(g, r, b)
                         for (key, g, r), (_, _, b) in zip(TC.pairs(got, ref), TC.pairs(got, bd))}
                print(tag, assumed, {k: round(v, 3) for k, v in worst.items()})
                assert max(worst.values()) <= 1.0, (tag, assumed, worst)
        assert_same_bits(results, ('pooled', 'cat', 'gys', 'gx_pool', 'gys_part'), tag)


# ------------------------------------------------------------------------------ MLP decoders
MLD_B = TM.B
MLD_FWD_CASE = ((3, 2, 1, 5), (8, 4, 2, 1), (40, 56))
# (channels, factors, output size, need subsets of the backward call)
MLD_BWD_CASES = (((64, 3), (2, 1), (36, 40), (None,)),
                 ((3, 5, 10, 2), (8, 4, 2, 1), (40, 56), (None, (True, False, True, True))))


def mld_fwd_items(channels, hw, dtype, vector):
    vec = (4 if dtype == F32 else 8) if vector else 1
    return MLD_B * sum(channels) * cdiv(hw[0] * hw[1], THREADS * vec)


def mld_bwd_items(channels, factors, hw, need):
    need = (True,) * len(channels) if need is None else need
    return sum(cdiv(MLD_B * c * (hw[0] // f) * (hw[1] // f), THREADS)
               for c, f, n in zip(channels, factors, need) if n and f > 1)


def mld_check(assume_cus, channels, factors, hw, dtype, mode, element, needs):
    everything = (-1,) + tuple(range(len(channels)))    # every tensor one element into a larger buffer
    for tier in ('exact', 'normal'):
        tag = (channels, factors, hw, dtype, mode, element, tier)
        ys, g_out = RM.make_inputs(MLD_B, channels, factors, hw, seed=hw[1], dtype=dtype, integer=tier == 'exact')
        out = torch.empty((MLD_B, sum(channels)) + hw, dtype=dtype, device=DEV)
        moved = tuple(TM.off_by_one(y.to(DEV)) if element else y.to(DEV) for y in ys)
        assert ops.mlpdec_route(moved, out) == (TM.ELEMENT if element else TM.VECTOR), tag
        ref = RM.reference64(ys, mode, g_out, size=hw)
        bd = RM.bounds(ys, mode, g_out, dtype=dtype, size=hw) if tier == 'normal' else None
        for need in needs:
            results = []
            for assumed in COUNTS:
                assume_cus(assumed)
                got = TM.run_ops(ys, g_out, mode, hw, shift=everything if element else (), need=need)
                results.append(got)
                for i in range(len(channels)):
                    assert (got['gys'][i] is None) == (need is not None and not need[i]), (tag, need, i)
                for (key, g, r), (_, _, b) in zip(TM.pairs(got, ref), TM.pairs(got, bd or ref)):
                    if g is None:
                        continue
                    assert g.dtype == dtype and tuple(g.shape) == tuple(r.shape), (tag, key)
                    if tier == 'exact':
                        assert torch.equal(g.cpu(), r.to(dtype)), (tag, need, assumed, key)      # cast once
                    else:
                        ratio = RM.worst_ratio(g, r, b)
                        assert ratio <= 1.0, (tag, need, assumed, key, ratio)
            assert_same_bits(results, ('cat', 'gys'), (tag, need))


@pytest.mark.parametrize('mode', TM.MODES)
@pytest.mark.parametrize('dtype', DTYPES, ids=('f32', 'bf16', 'f16'))
@pytest.mark.parametrize('element', (False, True), ids=('vector', 'element'))
def test_mlp_decoder_forward_over_several_trips(assume_cus, element, dtype, mode):
    """k_mlpdec_upcat_fwd: the plane -> branch search per item over four branches, and lanes behind
    the plane's end leaving the loop body in the last chunk of every plane (2240 pixels)"""
    channels, factors, hw = MLD_FWD_CASE
    assert_trips(mld_fwd_items(channels, hw, dtype, not element), MLD_BLOCKS_PER_CU, 'k_mlpdec_upcat_fwd')
    assert all((hw[0] * hw[1]) % (THREADS * vec) != 0 for vec in (1, 4, 8))
    mld_check(assume_cus, channels, factors, hw, dtype, mode, element, (None,))


@pytest.mark.parametrize('mode', TM.MODES)
@pytest.mark.parametrize('dtype', DTYPES, ids=('f32', 'bf16', 'f16'))
@pytest.mark.parametrize('case', MLD_BWD_CASES, ids=('64-3', '3-5-10-2'))
def test_mlp_decoder_backward_over_several_trips(assume_cus, case, dtype, mode):
    """k_mlpdec_upcat_bwd: the `first[]` search per item; items that span planes; with the middle
    branch unwanted two branches share their first item; lanes behind the last plane of a branch"""
    channels, factors, hw, needs = case
    for need in needs:
        assert_trips(mld_bwd_items(channels, factors, hw, need), MLD_BLOCKS_PER_CU, ('k_mlpdec_upcat_bwd', need))
    for element in (False, True):           # g_out (and every branch) off 16 bytes: the backward has one route
        mld_check(assume_cus, channels, factors, hw, dtype, mode, element, needs)


# ------------------------------------------------------------------------------ surface normals
NRM_B = 2
NRM_HW = ((95, 131), (96, 132))             # HW % 4 == 1: per-pixel loads; HW % 4 == 0: 16-byte loads
NRM_NET, NRM_CROP = (50, 70), (1, 49, 2, 68)            # the network-resolution map and its valid region


def nrm_assert_trips(hw, what):
    units = NRM_B * cdiv(hw[0] * hw[1], 4)
    lanes = NRM_BLOCKS_PER_CU * THREADS                 # of one assumed compute unit
    assert units // lanes >= 3 and units % lanes != 0, (what, units)             # per lane
    assert_trips(cdiv(units, THREADS), NRM_BLOCKS_PER_CU, what)                  # per workgroup


def nrm_inputs(hw):
    rng = np.random.default_rng(hw[1])
    target = syn._normal_target(rng, NRM_B, hw[0], hw[1], False)
    pred = rng.standard_normal((NRM_B, 3) + NRM_NET, dtype=np.float32)
    given = rng.random((NRM_B,) + hw) < 0.6
    return target, pred, given


@pytest.mark.parametrize('hw', NRM_HW, ids=('95x131', '96x132'))
def test_normal_valid_mask_over_several_trips(assume_cus, hw):
    nrm_assert_trips(hw, 'k_normal_valid_mask')
    target, _, _ = nrm_inputs(hw)
    want = TN._valid_np(target)
    assert want.any() and not want.all()
    td = TN._dev(target)
    assert (td.data_ptr() % 16 == 0) and ((hw[0] * hw[1]) % 4 == 0) == (hw == NRM_HW[1])
    masks = []
    for assumed in COUNTS:
        assume_cus(assumed)
        masks.append(ops.normal_valid_mask(td))
        assert np.array_equal(masks[-1].cpu().numpy(), want), assumed
    assert torch.equal(masks[0], masks[1]) and torch.equal(masks[0], masks[2])


@pytest.mark.parametrize('tag', ('derived', 'none', 'given'))
@pytest.mark.parametrize('hw', NRM_HW, ids=('95x131', '96x132'))
def test_rmse_update_over_several_trips(assume_cus, hw, tag):
    """k_rmse, prediction at the target's resolution and at the network resolution (crop + nearest
    resize folded in), the three mask modes: the exact count and the tolerance test_normal_task.py
    holds `rmse_update` to, under every assumed count (the sum's grouping follows the grid)"""
    nrm_assert_trips(hw, 'k_rmse')
    target, pred, given = nrm_inputs(hw)
    recipe = (NRM_B, NRM_NET, NRM_CROP, hw, (1,))
    full = TN._fullres_np(pred, recipe)
    mask_np, mask_arg = {'derived': (TN._valid_np(target), 'target'), 'none': (None, None),
                         'given': (given, TN._dev(given))}[tag]
    truth = TN._truth64(full, target, mask_np)
    count = NRM_B * hw[0] * hw[1] if mask_np is None else int(mask_np.sum())
    td, fd, pd = TN._dev(target), TN._dev(full), TN._dev(pred)
    for assumed in COUNTS:
        assume_cus(assumed)
        for form, preds, crop in (('same size', fd, None), ('resized', pd, TN._slices(recipe))):
            s = torch.zeros((), dtype=torch.float64, device=DEV)
            n = torch.zeros((), dtype=torch.int64, device=DEV)
            ops.rmse_update(s, n, preds, td, mask_arg, crop=crop)
            print(f'{hw}/{tag}/{form}/{assumed}: sum {float(s)!r} truth64 {truth!r} n {int(n)}')
            assert int(n) == count, (form, assumed)
            assert abs(float(s) - truth) <= TN.RMSE_RTOL * truth, (form, assumed)


# ------------------------------------------------------------------------------ learned upsampling
UP_B, UP_C, UP_H = 2, 13, 9


def up_items(h, w, run):
    return UP_B * UP_C * cdiv(cdiv(h, UP_TILE_H) * (w // run), THREADS)


@pytest.mark.parametrize('zeropad', TU.MODES)
@pytest.mark.parametrize('dtype', DTYPES, ids=('f32', 'bf16', 'f16'))
def test_upsampling_over_several_trips(assume_cus, dtype, zeropad):
    """k_up_fwd, k_up_bwd, k_up_reduce: w = 8 the vector route of every dtype, w = 7 the one-pixel route"""
    for w in (8, 7):
        run = TU.RUN[dtype] if w % TU.RUN[dtype] == 0 else 1
        assert_trips(up_items(UP_H, w, run), UP_BLOCKS_PER_CU, ('k_up', w))
        for tier in ('exact', 'normal'):
            tag = (dtype, zeropad, w, tier)
            make = TU.grid_inputs if tier == 'exact' else TU.normal_inputs
            x, gy, wt, b = make(UP_B, UP_C, UP_H, w, dtype, seed=w)
            want = dict(zip(('y', 'gx', 'gw', 'gb'), RU.reference64(x, wt, b, gy, zeropad)))
            bound = RU.bounds(x, wt, b, gy, zeropad, dtype) if tier == 'normal' else None
            results = []
            for assumed in COUNTS:
                assume_cus(assumed)
                y, gx, gw, gb, routes = TU.run_op(x, gy, wt, b, zeropad)
                assert routes[0] == routes[1] == (TU.VECTOR if run > 1 else TU.PIXEL), (tag, assumed)
                got = {'y': y, 'gx': gx, 'gw': gw, 'gb': gb}
                results.append(got)
                for key in ('y', 'gx', 'gw', 'gb'):
                    if tier == 'exact':
                        cast = dtype if key in ('y', 'gx') else F32
                        assert got[key].dtype == cast
                        assert torch.equal(got[key].cpu(), want[key].to(cast)), (tag, assumed, key)
                    else:
                        TU.assert_within(got[key], want[key], bound[key], f'{tag} {assumed} {key}')
            assert_same_bits(results, ('y', 'gx'), tag)


# ------------------------------------------------------------------------------ the workspace cache
def test_ln_backward_workspace_follows_the_grid(assume_cus):
    """`ops._workspace` caches the partial sums of a backward call per (device, stream, op, shape),
    and the LayerNorm-transpose backward needs workgroups x 2 x C floats: the same shape under one
    assumed compute unit (4 lines), the device's own count (one line per tile) and three (12 lines)
    on one stream.  Every call must succeed and give the oracle's sums"""
    dx, dy = BF16, F32
    B, P, C = 2, 392, 96                    # 26 tiles; a shape no other test of this file caches
    tiles = B * cdiv(P, LNT_TILE)
    assert tiles > 3 * LNT_BWD_BLOCKS_PER_CU
    x, gamma, beta, add, gy = TF.exact_inputs(B, P, C, dx, dy, seed=5)
    ref = RF.reference64(x, gamma, beta, 0.0, add, gy)
    sizes = []
    for assumed in (1, None, 3):
        cus = assume_cus(assumed)
        sizes.append(lnt_workgroups(B, P, C))
        assert sizes[-1] == min(tiles, LNT_BWD_BLOCKS_PER_CU * cus)
        got = lnt_run(x, gamma, beta, 0.0, add, gy, dy, False)
        assert torch.equal(got['y'].cpu(), ref['y'].to(dy)), assumed
        assert torch.equal(got['ggamma'].cpu().double(), ref['ggamma']), assumed
        assert torch.equal(got['gbeta'].cpu().double(), ref['gbeta']), assumed
    assert sizes == [LNT_BWD_BLOCKS_PER_CU, tiles, 3 * LNT_BWD_BLOCKS_PER_CU]


def test_upsampling_backward_workspace_does_not_follow_the_grid(assume_cus):
    """the learned upsampling's backward keeps one partial per work item, whatever the grid: its size
    query answers the same under every count, and the same three calls succeed"""
    B, C, h, w = 2, 11, 9, 8
    x, gy, wt, b = TU.grid_inputs(B, C, h, w, F32, seed=3)
    y64, gx64, gw64, gb64 = RU.reference64(x, wt, b, gy, False)
    sizes = []
    for assumed in (1, None, 3):
        assume_cus(assumed)
        sizes.append(L.lib().nmsa_upsample2x_dw3x3_bwd_workspace_bytes(B, C, h, w))
        y, gx, gw, gb, _ = TU.run_op(x, gy, wt, b, False)
        assert torch.equal(gx.cpu(), gx64.float()), assumed
        assert torch.equal(gw.cpu().double(), gw64) and torch.equal(gb.cpu().double(), gb64), assumed
    assert sizes[0] == sizes[1] == sizes[2] > 0
