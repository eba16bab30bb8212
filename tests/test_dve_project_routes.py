"""Every route of `nmsa_dve_project` (csrc/dve_project.hip) under an assertion: the three
`k_dve_project<PT, NT>` instantiations and `k_dve_generic`, at the pixel tails (H*W % 128, % 64),
the channel tail (D % 16 = 4), the class-tile edges and on both sides of every condition of the
route rule.  `ops.dve_project_route` / `nmsa_dve_project_route` say which kernel a call takes
(0 generic, PT * 16 + NT tuned), so no row can silently test another kernel than it names.

Yardstick: the float64 chain x / ||x||, einsum with the float64 weights.  Bounds (those of
tests/test_dve_postprocessing.py, derived, none measured on the code under test): any summation
order of D float32 products of two unit vectors errs by at most gamma_D ||x^|| ||w||, so
  |logit - truth|  <= (D + 4) 2^-24 ||w_c||
  |xn - truth|     <= (D + 4) 2^-24 |truth|          (an exact 0 of the truth must be an exact 0)
  NaN exactly where the truth is non-finite.
There is no "4 x the reference's error" bound here: at D = 4 that error is too small a yardstick.
Inputs: emb ~ N(0, 1), w ~ N(0, 1) / sqrt(D), numpy generators with fixed seeds.

Bitwise checks follow from the kernel's description (one fmaf chain per output element, the norm
summed in a fixed order): a pixel's results depend neither on the instantiation, nor on its place
in the wave tile, nor on how the class rows are split over heads, passes or calls.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

GENERIC, R83, R43, R46 = 0, 8 * 16 + 3, 4 * 16 + 3, 4 * 16 + 6
ERR_ARG = -1

# id: (B, D, (H, W), Ca, Cb, route, seed); B 'big' = ceil(8 cus / ceil(HW / 128)), the fewest
# images that reach <8,3>; Ca / Cb None = head off
ROWS = {
    'prod_tails_hw4104_d20': ('big', 20, (54, 76), 40, None, R83, 11),     # HW % 128 = 8, D % 16 = 4
    'prod_half_masked_hw4160': ('big', 16, (52, 80), 17, 16, R83, 12),     # HW % 128 = 64, T = 3 of two heads
    'prod_full_tiles_c48': ('big', 16, (128, 128), 48, None, R83, 13),
    'under_threshold': ('big-1', 20, (54, 76), 40, None, R43, 11),         # the first row less one image
    'smallest_3x4x4_c1': (3, 4, (2, 2), 1, None, R43, 14),
    'tail_hw60': (2, 20, (4, 15), 16, 17, R43, 15),
    'tail_hw68': (2, 20, (4, 17), 16, 17, R43, 16),
    'tail_hw124': (2, 20, (4, 31), 16, 17, R43, 17),
    't4_c49': (2, 36, (12, 16), 49, None, R46, 18),
    'head_b_only_c97_hw196': (2, 36, (14, 14), None, 97, R46, 19),         # T = 7: two passes
    'limits_d1024_c256_c256': (1, 1024, (8, 8), 256, 256, R46, 20),        # T = 32: six passes
    'generic_d1028': (1, 1028, (8, 8), 40, None, GENERIC, 21),
    'generic_c257': (1, 64, (8, 8), 257, None, GENERIC, 22),
    'generic_hw66': (2, 16, (6, 11), 40, None, GENERIC, 23),
    'generic_emb_4_byte_aligned': (2, 16, (8, 8), 40, None, GENERIC, 24),
    'generic_weight_4_byte_aligned': (2, 16, (8, 8), 40, None, GENERIC, 24),
}


def _cus():
    from nicr_mt_scene_analysis_amd import _lib as L
    return L.device_geometry()[0]


def _big_b(hw):
    tiles = -(-hw // 128)
    return -(-8 * _cus() // tiles)


def _truth64(emb, w):
    x = torch.from_numpy(emb).double()
    xn = x / x.norm(dim=1, keepdim=True)
    return xn, torch.einsum('bdhw,cd->bchw', xn, torch.from_numpy(w).double())


def _ceiling(w, D):
    """per class: (D + 4) 2^-24 ||w_c||"""
    return (D + 4) * 2.0 ** -24 * np.linalg.norm(w.astype(np.float64), axis=1)


def _make(B, D, H, W, Ca, Cb, seed):
    rng = np.random.default_rng(seed)
    emb = rng.standard_normal((B, D, H, W), dtype=np.float32)
    ws = [None if C is None else (rng.standard_normal((C, D), dtype=np.float32) / np.float32(np.sqrt(D)))
          for C in (Ca, Cb)]
    return emb, ws


@functools.lru_cache(maxsize=None)
def _row(name):
    """(emb, [weight_a, weight_b], xn64, [l64_a, l64_b], route): computed once per row and shared
    by the self-check and the GPU tests; nobody writes to these arrays"""
    B, D, (H, W), Ca, Cb, route, seed = ROWS[name]
    if B == 'big-1':                                    # the same images less the last one
        emb, ws, xn64, l64, _ = _row('prod_tails_hw4104_d20')
        return emb[:-1], ws, xn64[:-1], [None if l is None else l[:-1] for l in l64], route
    if B == 'big':
        B = _big_b(H * W)
    emb, ws = _make(B, D, H, W, Ca, Cb, seed)
    assert emb.nbytes <= 64 << 20
    xn64, l64 = None, []
    for w in ws:
        if w is None:
            l64.append(None)
            continue
        xn64, l = _truth64(emb, w)
        l64.append(l)
    return emb, ws, xn64, l64, route


def _check(label, D, ws, xn64, l64, xn, logits):
    """the two ceilings and NaN exactly where the truth is non-finite; returns and prints the
    largest error / ceiling of the logits and of the normalised map"""
    worst = 0.0
    for h, w, want, got in zip('ab', ws, l64, logits):
        if w is None:
            assert got is None
            continue
        assert got.dtype == torch.float32 and got.shape == want.shape
        finite = torch.isfinite(want)
        assert torch.equal(torch.isnan(got), ~finite), f'{label}/{h}: NaN pattern of the logits'
        ceil = torch.from_numpy(_ceiling(w, D)).view(1, -1, 1, 1)
        ratio = torch.where(finite, (got.double() - want).abs(), torch.zeros((), dtype=torch.float64)) / ceil
        worst = max(worst, float(ratio.max()))
        print(f'{label}/{h}: logits max error / ceiling {float(ratio.max()):.3f}')
        assert (ratio <= 1.0).all(), f'{label}/{h}: logits beyond (D + 4) 2^-24 ||w_c||'
    finite = torch.isfinite(xn64)
    assert xn.dtype == torch.float32 and xn.shape == xn64.shape
    assert torch.equal(torch.isnan(xn), ~finite), f'{label}: NaN pattern of the normalised map'
    err = (xn.double() - xn64).abs()[finite]
    bound = (D + 4) * 2.0 ** -24 * xn64.abs()[finite]
    assert (err <= bound).all(), f'{label}: normalised map beyond (D + 4) 2^-24 |truth|'
    nz = bound > 0
    ratio_n = float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0
    print(f'{label}: normalised map max error / ceiling {ratio_n:.3f}')
    return worst, ratio_n


# ------------------------------------------------------------------------------------ CPU tier
@pytest.mark.parametrize('name', list(ROWS))
def test_reference_self_check(name):
    """the yardstick itself: torch's float32 CPU chain lies within the same two bounds of the
    float64 truth on every shape of the matrix"""
    emb, ws, xn64, l64, _ = _row(name)
    x = torch.from_numpy(emb.copy())
    xn = x / x.norm(dim=1, keepdim=True)
    logits = [None if w is None else F.conv2d(xn, torch.from_numpy(w)[:, :, None, None]) for w in ws]
    _check(f'{name} (torch float32 on the CPU)', emb.shape[1], ws, xn64, l64, xn, logits)


def _route(lib, B=1, D=16, H=8, W=8, emb=0x10000, wa=0x20000, Ca=40, la=0x30000,
           wb=None, Cb=0, lb=None, route=0):
    """the pointers are only looked at for NULL and alignment: plain integers do"""
    return lib.nmsa_dve_project_route(emb, B, D, H, W, wa, Ca, la, wb, Cb, lb, route)


def test_route_rule_class_tile_edges():
    """T = ceil(Ca / 16) + ceil(Cb / 16) over BOTH heads: up to 3 tiles <4,3> (a 64-pixel map never
    reaches <8,3>), more <4,6>, above 256 classes in one head the generic kernel"""
    from nicr_mt_scene_analysis_amd import _lib as L
    lib = L.lib()
    for C, want in ((1, R43), (16, R43), (17, R43), (48, R43), (49, R46), (96, R46), (97, R46),
                    (256, R46), (257, GENERIC)):
        assert _route(lib, Ca=C) == want, C
        assert _route(lib, wa=None, Ca=0, la=None, wb=0x20000, Cb=C, lb=0x30000) == want, C   # head b alone
    two = dict(wb=0x40000, lb=0x50000)
    for Ca, Cb, want in ((16, 16, R43), (17, 16, R43), (16, 17, R43), (32, 16, R43), (17, 17, R46),
                         (33, 16, R46), (1, 48, R46), (256, 256, R46), (256, 257, GENERIC),
                         (257, 1, GENERIC)):
        assert _route(lib, Ca=Ca, Cb=Cb, **two) == want, (Ca, Cb)


def test_route_rule_shape_alignment_and_geometry():
    from nicr_mt_scene_analysis_amd import _lib as L
    lib, cus = L.lib(), _cus()
    for D, want in ((4, R43), (20, R43), (1020, R43), (1024, R43), (1028, GENERIC), (6, GENERIC), (1, GENERIC)):
        assert _route(lib, D=D) == want, D
    assert _route(lib, H=6, W=11) == GENERIC                    # H*W % 4 != 0
    assert _route(lib, H=1, W=4) == R43
    # 16-byte alignment of every pointer of an enabled head; a disabled head's are not looked at
    assert _route(lib, emb=0x10004) == GENERIC
    assert _route(lib, wa=0x20004) == GENERIC
    assert _route(lib, la=0x30008) == GENERIC
    assert _route(lib, wb=0x40004, Cb=8, lb=0x50000) == GENERIC
    assert _route(lib, wb=0x40000, Cb=8, lb=0x5000c) == GENERIC
    assert _route(lib, wb=None, Cb=8, lb=0x50004) == R43
    assert _route(lib, route=1) == GENERIC                       # NMSA_DVE_ROUTE_GENERIC
    assert _route(lib, wa=None, Ca=0, la=None) == GENERIC        # no head: normalise only
    # <8,3> from B * ceil(HW / 128) >= 8 waves per compute unit, only with T <= 3
    for hw in (4104, 4160, 16384, 128, 4):
        tiles = -(-hw // 128)
        B = -(-8 * cus // tiles)
        assert B * tiles >= 8 * cus > (B - 1) * tiles
        assert _route(lib, B=B, D=20, H=1, W=hw) == R83, hw
        assert _route(lib, B=B, D=20, H=1, W=hw, Ca=17, wb=0x40000, Cb=16, lb=0x50000) == R83, hw
        assert _route(lib, B=B, D=20, H=1, W=hw, Ca=49) == R46, hw
        assert _route(lib, B=B, D=20, H=1, W=hw, route=1) == GENERIC, hw
        if B > 1:
            assert _route(lib, B=B - 1, D=20, H=1, W=hw) == R43, hw


def test_route_answers_the_launchs_error_codes():
    from nicr_mt_scene_analysis_amd import _lib as L
    lib = L.lib()
    assert _route(lib, emb=None) == ERR_ARG
    for bad in (dict(B=0), dict(D=0), dict(H=0), dict(W=-1), dict(Ca=0), dict(la=None), dict(route=2),
                dict(route=-1), dict(wb=0x40000, Cb=0, lb=0x50000), dict(wb=0x40000, Cb=8, lb=None)):
        assert _route(lib, **bad) == ERR_ARG, bad
    assert _route(lib, H=1 << 16, W=1 << 15) == ERR_ARG          # H*W = 2^31
    assert _route(lib, H=46340, W=46340) == R83                  # H*W just under 2^31: one image fills the device
    assert _route(lib, B=1 << 30, H=8, W=32) == ERR_ARG          # 2^32 wave tiles
    assert _route(lib, B=(1 << 31) - 1, H=1, W=257) == ERR_ARG   # generic: 2^31 + workgroups


def test_wrapper_rejects_cpu_tensors_and_dtypes():
    from nicr_mt_scene_analysis_amd import ops
    from nicr_mt_scene_analysis_amd._lib import NmsaError
    with pytest.raises(NmsaError):
        ops.dve_project_route(torch.zeros(1, 8, 4, 4))
    with pytest.raises(TypeError):
        ops.dve_project_route(torch.zeros(1, 8, 4, 4, dtype=torch.float16))


# ------------------------------------------------------------------------------------ GPU tier
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _offset_by_one_float(t):
    """the same values in a view one float into a larger allocation: 4- but not 16-byte aligned"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _run(emb, ws, want_route, **kw):
    from nicr_mt_scene_analysis_amd import ops
    assert ops.dve_project_route(emb, *ws, **kw) == want_route
    before = emb.clone()
    assert ops.dve_project_route(emb, *ws, **kw) == want_route and torch.equal(emb, before)   # launches nothing
    return ops.dve_project(emb, *ws, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(ROWS))
def test_route_and_truth(name):
    emb_np, ws_np, xn64, l64, route = _row(name)
    emb, ws = _dev(emb_np), [None if w is None else _dev(w) for w in ws_np]
    if name == 'generic_emb_4_byte_aligned':
        emb = _offset_by_one_float(emb)
    if name == 'generic_weight_4_byte_aligned':
        ws[0] = _offset_by_one_float(ws[0])
    logits = _run(emb, ws, route)
    a, n = _check(name, emb_np.shape[1], ws_np, xn64, l64, emb.cpu(),
                  [None if l is None else l.cpu() for l in logits])
    print(f'ROW {name}: B = {emb_np.shape[0]}, route {route}, error / ceiling: logits {a:.3f}, map {n:.3f}')


@pytest.mark.gpu
def test_generic_flag_on_a_production_shape():
    """the same inputs through the per-pixel kernel: the query follows the flag"""
    emb_np, ws_np, xn64, l64, _ = _row('under_threshold')
    emb, ws = _dev(emb_np), [None if w is None else _dev(w) for w in ws_np]
    logits = _run(emb, ws, GENERIC, generic=True)
    _check('under_threshold, generic', emb_np.shape[1], ws_np, xn64, l64, emb.cpu(),
           [None if l is None else l.cpu() for l in logits])


@pytest.mark.gpu
def test_replicas_under_8_3_equal_the_single_image_under_4_3():
    """one 54x76 image at B = 1 (<4,3>) and repeated until the call takes <8,3>: the wave tile a
    pixel sits in, and the half v of it, change; its results may not"""
    emb_np, ws_np, *_ = _row('prod_tails_hw4104_d20')
    w = _dev(ws_np[0])
    one = _dev(emb_np[3:4])
    many = one.repeat(_big_b(54 * 76), 1, 1, 1).contiguous()
    (l1, _), (lm, _) = _run(one, [w, None], R43), _run(many, [w, None], R83)
    assert torch.equal(lm, l1.expand_as(lm))
    assert torch.equal(many, one.expand_as(many))


@pytest.mark.gpu
def test_pixel_groups_permuted_under_8_3():
    """groups of 4 pixels (one float4 of a lane) shuffled over the whole 54x76 map: every group
    lands in another lane, half and wave tile, the 8-pixel tail included"""
    emb_np, ws_np, *_ = _row('prod_tails_hw4104_d20')
    B, D, H, W = emb_np.shape
    w = _dev(ws_np[0])
    perm = torch.from_numpy(np.random.default_rng(31).permutation(H * W // 4)).cuda()
    emb = _dev(emb_np)
    shuffled = emb.view(B, D, -1, 4)[:, :, perm].reshape(B, D, H, W).contiguous()
    (l0, _), (l1, _) = _run(emb, [w, None], R83), _run(shuffled, [w, None], R83)
    assert torch.equal(l0.view(B, -1, H * W // 4, 4)[:, :, perm].reshape(l0.shape), l1)
    assert torch.equal(emb.view(B, D, -1, 4)[:, :, perm].reshape(B, D, H, W), shuffled)


@pytest.mark.gpu
@pytest.mark.parametrize('name,route', [('tail_hw124', R43), ('prod_tails_hw4104_d20', R83)])
def test_rows_split_over_the_heads(name, route):
    """40 class rows in head a, and the same rows as 24 + 16 in heads a and b (two tiles + one):
    the second head's rows move to another tile and another head's output, the norm stays"""
    emb_np, _, *_ = _row(name)
    D = emb_np.shape[1]
    w = _dev(np.random.default_rng(32).standard_normal((40, D), dtype=np.float32) / np.float32(np.sqrt(D)))
    e1, e2 = _dev(emb_np), _dev(emb_np)
    (l, _), (la, lb) = _run(e1, [w, None], route), _run(e2, [w[:24].contiguous(), w[24:].contiguous()], route)
    assert torch.equal(torch.cat([la, lb], dim=1), l)
    assert torch.equal(e1, e2)


@pytest.mark.gpu
def test_two_passes_equal_three_calls():
    """150 rows in one call (<4,6>, T = 10: two passes over the same pixels) and 50 rows per call
    on clones of the map (T = 4, one pass)"""
    emb_np, _, *_ = _row('head_b_only_c97_hw196')
    D = emb_np.shape[1]
    w = _dev(np.random.default_rng(33).standard_normal((150, D), dtype=np.float32) / np.float32(np.sqrt(D)))
    e = _dev(emb_np)
    (l, _) = _run(e, [w, None], R46)
    for k in range(3):
        ek = _dev(emb_np)
        (lk, _) = _run(ek, [w[50 * k:50 * k + 50].contiguous(), None], R46)
        assert torch.equal(lk, l[:, 50 * k:50 * k + 50]), k
        assert torch.equal(ek, e), k


@pytest.mark.gpu
@pytest.mark.parametrize('route', [R43, R83])
def test_non_finite_pixels_on_the_tuned_routes(route):
    """an all-zero pixel and a pixel with one +inf channel next to ordinary pixels of the same
    float4 group: in a full tile and in the last, partial one (for <8,3> also in the upper half of
    a tile).  NaN for the whole zero pixel; the inf pixel: NaN logits, NaN in the inf channel,
    exact zeros in the others; every other pixel finite and within the ceilings."""
    D, C = 20, 40
    H, W = (12, 17) if route == R43 else (54, 76)      # 204 = 3 x 64 + 12, 4104 = 32 x 128 + 8
    HW = H * W
    B = 2 if route == R43 else _big_b(HW)
    emb_np, ws_np = _make(B, D, H, W, C, None, 41)
    tile = 64 if route == R43 else 128
    # (image, first pixel of the float4 group, inf channel): zero pixel at +1, inf pixel at +2
    spots = [(0, tile + 20, 5), (B - 1, HW - 4, 17), (B - 1, (HW // tile) * tile, 2)]
    if route == R83:
        spots.append((B // 2, 3 * tile + 64 + 8, 19))                      # v = 1 half
    flat = emb_np.reshape(B, D, HW)
    for b, g, d in spots:
        assert g % 4 == 0 and g + 3 < HW
        flat[b, :, g + 1] = 0.0
        flat[b, d, g + 2] = np.inf
    xn64, l64 = _truth64(emb_np, ws_np[0])
    emb = _dev(emb_np)
    (lg, _) = _run(emb, [_dev(ws_np[0]), None], route)
    xn, lg = emb.cpu(), lg.cpu()
    # every pixel against the truth: NaN exactly where it is non-finite, zeros exact, the rest bounded
    _check(f'non-finite {route}', D, ws_np, xn64, [l64, None], xn, [lg, None])
    xf, lf = xn.reshape(B, D, HW), lg.reshape(B, C, HW)
    clean = torch.ones(B, HW, dtype=torch.bool)
    for b, g, d in spots:
        assert torch.isnan(lf[b, :, g + 1]).all() and torch.isnan(xf[b, :, g + 1]).all()
        assert torch.isnan(lf[b, :, g + 2]).all() and torch.isnan(xf[b, d, g + 2])
        others = torch.arange(D) != d
        assert (xf[b, others, g + 2] == 0).all()
        clean[b, g + 1] = clean[b, g + 2] = False
    assert int((~clean).sum()) == 2 * len(spots)
    assert torch.isfinite(lf.permute(0, 2, 1)[clean]).all() and torch.isfinite(xf.permute(0, 2, 1)[clean]).all()


@pytest.mark.gpu
def test_postprocess_reaches_8_3():
    """the first <8,3> row through the public class: same logits and map as the truth allows"""
    from nicr_mt_scene_analysis_amd import ops
    from nicr_mt_scene_analysis_amd.data.preprocessing import APPLIED_PREPROCESSING_KEY
    from nicr_mt_scene_analysis_amd.model.postprocessing import get_postprocessing_class
    emb_np, ws_np, xn64, l64, route = _row('prod_tails_hw4104_d20')
    B, D, H, W = emb_np.shape
    w = _dev(ws_np[0])
    post = get_postprocessing_class('dense-visual-embedding')(with_text_embeddings_per_class=True,
                                                              text_embeddings_per_class=w)
    batch = {'semantic_fullres': torch.zeros((B, H, W), dtype=torch.uint8, device='cuda'),
             APPLIED_PREPROCESSING_KEY: [[{'type': 'Resize', 'valid_region_slice_y': slice(0, H),
                                           'valid_region_slice_x': slice(0, W)}]] * B}
    emb = _dev(emb_np)
    assert ops.dve_project_route(emb, w) == route == R83
    r = post.postprocess((emb, None), batch, is_training=False)
    logits = r['dense_visual_embedding_text_based_semantic_output']
    assert r['dense_visual_embedding_output'] is emb
    _check('postprocess, <8,3>', D, ws_np, xn64, l64, emb.cpu(), [logits.cpu(), None])
    assert torch.equal(r['dense_visual_embedding_text_based_semantic_idx'], logits.argmax(dim=1))
