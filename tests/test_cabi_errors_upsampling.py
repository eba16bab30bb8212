"""CPU tier: the host checks of the three upsampling entry points (csrc/upsampling.hip), in the
manner of tests/test_cabi_errors_scene.py.  Every argument is checked before anything is enqueued,
so a refused call comes back with its code without a device: no call below reaches a HIP call and
the made-up addresses are never dereferenced.  That the unbroken backward arguments get past the
checks is shown by a call that wants no output: NMSA_OK from behind the last check, no launch."""
import ctypes as C

from nicr_mt_scene_analysis_amd import _lib as L

ARG, WORKSPACE, UNSUPPORTED = -1, -3, -4
X, Y, W, BIAS, GX, GW, GB, WS = (0x100000 * (i + 1) for i in range(8))
GOOD = dict(x=X, dtype=L.NMSA_F32, weight=W, bias=BIAS, B=2, C=3, h=5, w=6, zeropad=0, y=Y,
            gy=Y, gx=GX, gweight=GW, gbias=GB, ws=WS, ws_bytes=1 << 20)


def p(v):
    return C.c_void_p(v) if v else None


def fwd(**changes):
    a = dict(GOOD, **changes)
    return L.lib().nmsa_upsample2x_dw3x3_fwd(p(a['x']), a['dtype'], p(a['weight']), p(a['bias']), a['B'], a['C'],
                                             a['h'], a['w'], a['zeropad'], p(a['y']), None)


def bwd(**changes):
    a = dict(GOOD, **changes)
    return L.lib().nmsa_upsample2x_dw3x3_bwd(p(a['gy']), p(a['x']), a['dtype'], p(a['weight']), a['B'], a['C'],
                                             a['h'], a['w'], a['zeropad'], p(a['gx']), p(a['gweight']),
                                             p(a['gbias']), p(a['ws']), a['ws_bytes'], None)


def route(**changes):
    a = dict(GOOD, **changes)
    return L.lib().nmsa_upsample2x_dw3x3_route(p(a['x']), p(a['y']), a['dtype'], a['B'], a['C'], a['h'], a['w'])


NOTHING = dict(gx=0, gweight=0, gbias=0)


def test_the_unbroken_backward_arguments_pass_the_checks():
    assert bwd(**NOTHING) == 0
    assert bwd(ws=0, ws_bytes=0, **NOTHING) == 0          # no workspace needed without gW / gb
    for dtype in (L.NMSA_F32, L.NMSA_BF16, L.NMSA_F16):
        assert bwd(dtype=dtype, **NOTHING) == 0 and route(dtype=dtype) > 0


def test_null_pointers():
    for name in ('x', 'weight', 'y'):
        assert fwd(**{name: 0}) == ARG, name
    for name in ('gy', 'x', 'weight'):
        assert bwd(**{name: 0}) == ARG, name
        assert bwd(**dict(NOTHING, **{name: 0})) == ARG, name    # the checks hold when nothing is wanted
    assert route(x=0) == ARG and route(y=0) == ARG


def test_dtype():
    for bad in (3, -1, 7):
        assert fwd(dtype=bad) == ARG and bwd(dtype=bad) == ARG and route(dtype=bad) == ARG, bad


def test_sizes_below_one():
    for name in ('B', 'C', 'h', 'w'):
        for bad in (0, -1):
            assert fwd(**{name: bad}) == ARG and bwd(**{name: bad}) == ARG and route(**{name: bad}) == ARG, name
            assert L.lib().nmsa_upsample2x_dw3x3_bwd_workspace_bytes(*(bad if k == name else 2 for k in 'BChw')) == 0


def test_pad_flag():
    for bad in (2, -1):
        assert fwd(zeropad=bad) == ARG and bwd(zeropad=bad) == ARG


def test_a_plane_of_two_to_the_31_elements_is_refused():
    # 4hw = 2^31: one element too many for 32-bit offsets inside a plane; one row less is accepted
    big = dict(B=1, C=1, h=1 << 14, w=1 << 15)
    assert fwd(**big) == UNSUPPORTED and bwd(**big) == UNSUPPORTED and route(**big) == UNSUPPORTED
    assert bwd(**dict(big, h=(1 << 14) - 1, **NOTHING)) == 0
    assert fwd(B=1 << 16, C=1 << 16) == UNSUPPORTED         # B * C above 2^31 - 1


def test_misaligned_pointers():
    # off the element: refused.  Off 16 bytes only: the one-pixel route, not an error
    for name in ('x', 'y', 'weight', 'bias'):
        assert fwd(**{name: GOOD[name] + 1}) == ARG, name
    for name in ('gy', 'x', 'gx', 'weight', 'gweight', 'gbias'):
        assert bwd(**{name: GOOD[name] + 2}) == ARG, name
    assert fwd(dtype=L.NMSA_BF16, x=X + 1) == ARG and bwd(dtype=L.NMSA_F16, gy=Y + 1) == ARG
    assert bwd(dtype=L.NMSA_BF16, gy=Y + 2, **NOTHING) == 0
    assert route(x=X + 2) == ARG and route(dtype=L.NMSA_BF16, x=X + 2) == L.NMSA_UP_ROUTE_PIXEL
    assert bwd(ws=WS + 4) == ARG and bwd(ws=WS + 8, gx=0) == ARG


def test_workspace():
    need = L.lib().nmsa_upsample2x_dw3x3_bwd_workspace_bytes(2, 3, 5, 6)
    assert need > 0
    for want in (dict(gx=0, gbias=0), dict(gx=0, gweight=0), dict()):
        assert bwd(ws_bytes=0, **want) == WORKSPACE and bwd(ws=0, **want) == ARG
    # the one-pixel route (an odd width) needs the whole of the query's answer
    odd = dict(w=7, gx=0)
    need = L.lib().nmsa_upsample2x_dw3x3_bwd_workspace_bytes(2, 3, 5, 7)
    assert bwd(ws_bytes=need - 1, **odd) == WORKSPACE
    assert bwd(ws_bytes=need - 1, gweight=0, gbias=0, **odd) == 0     # nothing wanted, none needed
