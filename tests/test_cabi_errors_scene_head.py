"""CPU tier: the host checks of the three scene-head entry points (csrc/scene_head.hip), in the manner of
tests/test_cabi_errors_maxpool.py.  Every argument is checked before anything is enqueued, so a refused call
comes back with its code without a device: no call below reaches a HIP call and the made-up addresses are never
dereferenced.  The host-only route query shows that the unbroken arguments get past the checks."""
import ctypes as C

from nicr_mt_scene_analysis_amd import _lib as L

OK, ARG, UNSUPPORTED = 0, -1, -4
X, WEIGHT, BIAS, POOLED, LOGITS, G, GX, GW, GB = (0x100000 * (i + 1) for i in range(9))
GOOD = dict(x=X, dtype_x=L.NMSA_F32, B=2, C=3, H=2, W=4, weight=WEIGHT, bias=BIAS, pooled=POOLED, logits=LOGITS,
            dtype_out=L.NMSA_F32, K=5, g=G, gx=GX, gweight=GW, gbias=GB)
UNIT, VECTOR, ELEMENT = L.NMSA_SH_ROUTE_UNIT, L.NMSA_SH_ROUTE_VECTOR, L.NMSA_SH_ROUTE_ELEMENT
DTYPES = (L.NMSA_F32, L.NMSA_BF16, L.NMSA_F16)


def p(v):
    return C.c_void_p(v) if v else None


def fwd(**changes):
    a = dict(GOOD, **changes)
    return L.lib().nmsa_scene_head_fwd(p(a['x']), a['dtype_x'], a['B'], a['C'], a['H'], a['W'], p(a['weight']),
                                       p(a['bias']), p(a['pooled']), p(a['logits']), a['dtype_out'], a['K'], None)


def bwd(**changes):
    # dtype_out is the dtype of g
    a = dict(GOOD, **changes)
    return L.lib().nmsa_scene_head_bwd(p(a['g']), a['dtype_out'], p(a['pooled']), p(a['weight']), a['B'], a['C'],
                                       a['H'], a['W'], a['K'], p(a['gx']), a['dtype_x'], p(a['gweight']),
                                       p(a['gbias']), None)


def route(**changes):
    a = dict(GOOD, **changes)
    return L.lib().nmsa_scene_head_route(p(a['x']), a['dtype_x'], a['B'], a['C'], a['H'], a['W'], a['K'])


def test_route_constants_and_the_unbroken_arguments():
    assert (UNIT, VECTOR, ELEMENT) == (1, 2, 4)
    assert L.NMSA_SCENE_HEAD_MAX_CHANNELS == 2048 and L.NMSA_SCENE_MAX_CLASSES == 4096
    for dtype in DTYPES:
        assert route(dtype_x=dtype) == VECTOR                   # H W = 8


def test_null_pointers():
    for name in ('x', 'weight', 'logits'):
        assert fwd(**{name: 0}) == ARG, name
    for name in ('g', 'pooled', 'weight'):
        assert bwd(**{name: 0}) == ARG, name
    assert route(x=0) == ARG
    # every gradient of the backward call may be left out; with none wanted nothing is launched
    assert bwd(gx=0, gweight=0, gbias=0) == OK
    assert bwd(gx=0, gweight=0, gbias=0, g=0) == ARG and bwd(gx=0, gweight=0, gbias=0, K=0) == ARG


def test_dtype():
    for bad in (3, -1, 7):
        assert fwd(dtype_x=bad) == ARG and fwd(dtype_out=bad) == ARG, bad
        assert bwd(dtype_x=bad) == ARG and bwd(dtype_out=bad) == ARG, bad
        assert route(dtype_x=bad) == ARG, bad


def test_sizes_below_one():
    for name in ('B', 'C', 'H', 'W', 'K'):
        for bad in (0, -1):
            assert fwd(**{name: bad}) == ARG and bwd(**{name: bad}) == ARG and route(**{name: bad}) == ARG, name


def test_limits():
    for call in (fwd, bwd, route):
        assert call(C=L.NMSA_SCENE_HEAD_MAX_CHANNELS + 1) == UNSUPPORTED
        assert call(K=L.NMSA_SCENE_MAX_CLASSES + 1) == UNSUPPORTED
        # H W = 2^31: one element too many for 32-bit offsets inside a plane
        assert call(B=1, C=1, H=1 << 16, W=1 << 15) == UNSUPPORTED
        # 2^31 or more wave items: B C planes alone
        assert call(B=1 << 20, C=2048) == UNSUPPORTED
        # the refusals of the arguments come first
        assert call(C=L.NMSA_SCENE_HEAD_MAX_CHANNELS + 1, dtype_x=5) == ARG
        assert call(K=L.NMSA_SCENE_MAX_CLASSES + 1, H=0) == ARG
    assert route(C=L.NMSA_SCENE_HEAD_MAX_CHANNELS, K=L.NMSA_SCENE_MAX_CLASSES) == VECTOR
    assert route(B=1, C=1, H=(1 << 16) - 1, W=1 << 15) == VECTOR
    assert route(B=(1 << 20) - 2049, C=2048, K=L.NMSA_SCENE_MAX_CLASSES) == VECTOR
    # B C + 131072 + 64 items: 2^31 - 1 of them is the last accepted count (B = 2^20 - 65)
    assert route(B=(1 << 20) - 65, C=2048, K=L.NMSA_SCENE_MAX_CLASSES) == VECTOR
    assert route(B=(1 << 20) - 64, C=2048, K=L.NMSA_SCENE_MAX_CLASSES) == UNSUPPORTED


def test_misaligned_pointers():
    # off the element: refused
    for name in ('x', 'logits', 'weight', 'bias', 'pooled'):
        assert fwd(**{name: GOOD[name] + 1}) == ARG and fwd(**{name: GOOD[name] + 2}) == ARG, name
    for name in ('g', 'gx', 'weight', 'pooled', 'gweight', 'gbias'):
        assert bwd(**{name: GOOD[name] + 1}) == ARG and bwd(**{name: GOOD[name] + 2}) == ARG, name
    for name in ('x', 'logits'):
        for dtype in (L.NMSA_BF16, L.NMSA_F16):
            assert fwd(dtype_x=dtype, dtype_out=dtype, **{name: GOOD[name] + 1}) == ARG, name
    assert bwd(dtype_x=L.NMSA_F16, dtype_out=L.NMSA_BF16, g=G + 1) == ARG
    assert bwd(dtype_x=L.NMSA_F16, dtype_out=L.NMSA_BF16, gx=GX + 1) == ARG
    assert route(x=X + 1) == ARG and route(x=X + 2) == ARG and route(dtype_x=L.NMSA_BF16, x=X + 1) == ARG
    # off 16 bytes only: the element route, not an error
    assert route(x=X + 4) == route(x=X + 8) == route(x=X + 12) == ELEMENT and route(x=X + 16) == VECTOR
    for dtype in (L.NMSA_BF16, L.NMSA_F16):
        assert route(dtype_x=dtype, x=X + 2) == route(dtype_x=dtype, x=X + 8) == ELEMENT
        assert route(dtype_x=dtype, x=X + 32) == VECTOR


def test_route_follows_the_plane_size():
    for H, W, f32, half in ((1, 1, UNIT, UNIT), (2, 4, VECTOR, VECTOR), (4, 4, VECTOR, VECTOR), (2, 2, VECTOR, ELEMENT),
                            (3, 4, VECTOR, ELEMENT), (5, 8, VECTOR, VECTOR), (2, 3, ELEMENT, ELEMENT),
                            (1, 2, ELEMENT, ELEMENT), (7, 37, ELEMENT, ELEMENT), (15, 20, VECTOR, ELEMENT)):
        assert route(H=H, W=W) == f32, (H, W)
        assert route(H=H, W=W, dtype_x=L.NMSA_BF16) == half and route(H=H, W=W, dtype_x=L.NMSA_F16) == half, (H, W)
    # a plane of one element stays on the unit route wherever it starts
    assert route(H=1, W=1, x=X + 4) == UNIT and route(H=1, W=1, dtype_x=L.NMSA_F16, x=X + 2) == UNIT
    # neither the other sizes nor the class count change the route
    assert route(B=7, C=130, K=45) == VECTOR and route(B=1, C=1, K=1, H=3, W=5) == ELEMENT
