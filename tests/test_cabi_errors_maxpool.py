"""CPU tier: the host checks of the three max-pool entry points (csrc/maxpool.hip), in the manner of
tests/test_cabi_errors_upsampling.py.  Every argument is checked before anything is enqueued, so a refused
call comes back with its code without a device: no call below reaches a HIP call and the made-up addresses are
never dereferenced.  The host-only route query shows that the unbroken arguments get past the checks."""
import ctypes as C

from nicr_mt_scene_analysis_amd import _lib as L

ARG, UNSUPPORTED = -1, -4
X, Y, CODE, GY, GX = (0x100000 * (i + 1) for i in range(5))
GOOD = dict(x=X, dtype=L.NMSA_F32, B=2, C=3, H=6, W=8, y=Y, code=CODE, gy=GY, gx=GX)
VECTOR, PIXEL = L.NMSA_MP_ROUTE_VECTOR, L.NMSA_MP_ROUTE_PIXEL


def p(v):
    return C.c_void_p(v) if v else None


def fwd(**changes):
    a = dict(GOOD, **changes)
    return L.lib().nmsa_maxpool3x3s2_fwd(p(a['x']), a['dtype'], a['B'], a['C'], a['H'], a['W'], p(a['y']),
                                         p(a['code']), None)


def bwd(**changes):
    a = dict(GOOD, **changes)
    return L.lib().nmsa_maxpool3x3s2_bwd(p(a['gy']), p(a['code']), a['dtype'], a['B'], a['C'], a['H'], a['W'],
                                         p(a['gx']), None)


def route(**changes):
    a = dict(GOOD, **changes)
    return L.lib().nmsa_maxpool3x3s2_route(p(a['x']), p(a['y']), a['dtype'], a['B'], a['C'], a['H'], a['W'])


def test_route_constants_and_the_unbroken_arguments():
    assert (VECTOR, PIXEL) == (1, 2)
    for dtype in (L.NMSA_F32, L.NMSA_BF16, L.NMSA_F16):
        assert route(dtype=dtype) == VECTOR


def test_null_pointers():
    for name in ('x', 'y'):
        assert fwd(**{name: 0}) == ARG, name
        assert route(**{name: 0}) == ARG, name
    for name in ('gy', 'code', 'gx'):
        assert bwd(**{name: 0}) == ARG, name


def test_dtype():
    for bad in (3, -1, 7):
        assert fwd(dtype=bad) == ARG and bwd(dtype=bad) == ARG and route(dtype=bad) == ARG, bad


def test_sizes_below_one():
    for name in ('B', 'C', 'H', 'W'):
        for bad in (0, -1):
            assert fwd(**{name: bad}) == ARG and bwd(**{name: bad}) == ARG and route(**{name: bad}) == ARG, name


def test_a_plane_of_two_to_the_31_elements_is_refused():
    # H W = 2^31: one element too many for 32-bit offsets inside a plane; one row less is accepted
    big = dict(B=1, C=1, H=1 << 16, W=1 << 15)
    assert fwd(**big) == UNSUPPORTED and bwd(**big) == UNSUPPORTED and route(**big) == UNSUPPORTED
    assert route(**dict(big, H=(1 << 16) - 1)) == VECTOR
    many = dict(B=1 << 16, C=1 << 16)                       # B * C above 2^31 - 1
    assert fwd(**many) == UNSUPPORTED and bwd(**many) == UNSUPPORTED and route(**many) == UNSUPPORTED
    # 2^31 or more lane units: B * C * ceil(Ho / 8) * (Wo / 2) with Ho = 512, Wo = 512
    units = dict(B=1 << 10, C=1 << 7, H=1024, W=1024)
    assert route(**units) == VECTOR and fwd(**units) == UNSUPPORTED and bwd(**units) == UNSUPPORTED
    # the refusals of the arguments come first
    assert fwd(**dict(big, dtype=5)) == ARG and fwd(**dict(many, H=0)) == ARG


def test_misaligned_pointers():
    # off the element: refused.  Off 16 bytes only: the one-pixel route, not an error
    for name in ('x', 'y'):
        assert fwd(**{name: GOOD[name] + 1}) == ARG and fwd(**{name: GOOD[name] + 2}) == ARG, name
        assert route(**{name: GOOD[name] + 2}) == ARG, name
        assert fwd(dtype=L.NMSA_BF16, **{name: GOOD[name] + 1}) == ARG, name
        assert route(dtype=L.NMSA_F16, **{name: GOOD[name] + 2}) == PIXEL, name
        assert route(**{name: GOOD[name] + 4}) == PIXEL and route(**{name: GOOD[name] + 16}) == VECTOR, name
    for name in ('gy', 'gx'):
        assert bwd(**{name: GOOD[name] + 2}) == ARG and bwd(dtype=L.NMSA_F16, **{name: GOOD[name] + 1}) == ARG, name


def test_route_follows_the_width():
    for W, f32, half in ((8, VECTOR, VECTOR), (16, VECTOR, VECTOR), (4, VECTOR, PIXEL), (12, VECTOR, PIXEL),
                         (6, PIXEL, PIXEL), (9, PIXEL, PIXEL), (1, PIXEL, PIXEL), (2, PIXEL, PIXEL)):
        assert route(W=W) == f32, W
        assert route(W=W, dtype=L.NMSA_BF16) == half and route(W=W, dtype=L.NMSA_F16) == half, W
    for H in (1, 2, 7):
        assert route(H=H) == VECTOR
