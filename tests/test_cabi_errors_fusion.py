"""CPU tier: the host checks of the four LayerNorm-transpose entry points (csrc/ln_transpose.hip), in
the manner of tests/test_cabi_errors_upsampling.py.  Every argument is checked before anything is
enqueued, so a refused call comes back with its code without a device: no call below reaches a HIP
call and the made-up addresses are never dereferenced.  That the unbroken backward arguments get
past the checks is shown by a call that wants no output: NMSA_OK from behind the last check, no
launch.  (The forward call has no such form; its unbroken arguments are run by the GPU tier.)"""
import ctypes as C
import math

from nicr_mt_scene_analysis_amd import _lib as L

ARG, WORKSPACE, UNSUPPORTED = -1, -3, -4
VECTOR, ELEMENT = L.NMSA_LNT_ROUTE_VECTOR, L.NMSA_LNT_ROUTE_ELEMENT
X, Y, GAMMA, BETA, ADD, MEAN, RSTD, GX, GG, GB, WS = (0x100000 * (i + 1) for i in range(11))
F32, BF16, F16 = L.NMSA_F32, L.NMSA_BF16, L.NMSA_F16
GOOD = dict(x=X, dtype_x=F32, gamma=GAMMA, beta=BETA, eps=1e-5, add=ADD, B=2, P=8, C=8, y=Y, dtype_y=F32,
            mean=MEAN, rstd=RSTD, gy=Y, gx=GX, ggamma=GG, gbeta=GB, ws=WS, ws_bytes=1 << 20)
PAIRS = ((F32, F32), (BF16, BF16), (BF16, F32), (F16, F16), (F16, F32))


def p(v):
    return C.c_void_p(v) if v else None


def fwd(**changes):
    a = dict(GOOD, **changes)
    return L.lib().nmsa_ln_nhwc_nchw_fwd(p(a['x']), a['dtype_x'], p(a['gamma']), p(a['beta']), a['eps'], p(a['add']),
                                         a['B'], a['P'], a['C'], p(a['y']), a['dtype_y'], p(a['mean']),
                                         p(a['rstd']), None)


def bwd(**changes):
    a = dict(GOOD, **changes)
    return L.lib().nmsa_ln_nhwc_nchw_bwd(p(a['gy']), a['dtype_y'], p(a['x']), a['dtype_x'], p(a['gamma']),
                                         p(a['mean']), p(a['rstd']), a['B'], a['P'], a['C'], p(a['gx']),
                                         p(a['ggamma']), p(a['gbeta']), p(a['ws']), a['ws_bytes'], None)


def route(**changes):
    a = dict(GOOD, **changes)
    return L.lib().nmsa_ln_nhwc_nchw_route(p(a['x']), p(a['y']), a['dtype_x'], a['dtype_y'], a['B'], a['P'], a['C'])


def ws_bytes(B, P, C):
    return L.lib().nmsa_ln_nhwc_nchw_bwd_workspace_bytes(B, P, C)


NOTHING = dict(gx=0, ggamma=0, gbeta=0)


def test_the_unbroken_backward_arguments_pass_the_checks():
    assert bwd(**NOTHING) == 0
    assert bwd(ws=0, ws_bytes=0, **NOTHING) == 0          # no workspace needed without ggamma / gbeta
    for dx, dy in PAIRS:
        assert bwd(dtype_x=dx, dtype_y=dy, **NOTHING) == 0 and route(dtype_x=dx, dtype_y=dy) == VECTOR


def test_null_pointers():
    for name in ('x', 'y', 'gamma', 'beta'):
        assert fwd(**{name: 0}) == ARG, name
    for name in ('gy', 'x', 'gamma', 'mean', 'rstd'):
        assert bwd(**{name: 0}) == ARG, name
        assert bwd(**dict(NOTHING, **{name: 0})) == ARG, name    # the checks hold when nothing is wanted
    assert route(x=0) == ARG and route(y=0) == ARG
    # exactly one of mean / rstd
    assert fwd(mean=0) == ARG and fwd(rstd=0) == ARG


def test_dtypes():
    for bad in (3, -1, 7):
        assert fwd(dtype_x=bad) == ARG and bwd(dtype_x=bad) == ARG and route(dtype_x=bad) == ARG, bad
        assert fwd(dtype_y=bad) == ARG and bwd(dtype_y=bad) == ARG and route(dtype_y=bad) == ARG, bad
    # dtype_y is dtype_x or float32
    for dx, dy in ((F32, BF16), (F32, F16), (BF16, F16), (F16, BF16)):
        assert fwd(dtype_x=dx, dtype_y=dy) == ARG and bwd(dtype_x=dx, dtype_y=dy) == ARG
        assert route(dtype_x=dx, dtype_y=dy) == ARG


def test_sizes_below_one():
    for name in ('B', 'P', 'C'):
        for bad in (0, -1):
            assert fwd(**{name: bad}) == ARG and bwd(**{name: bad}) == ARG and route(**{name: bad}) == ARG, name
            assert ws_bytes(*(bad if k == name else 2 for k in 'BPC')) == 0


def test_eps():
    for bad in (-1e-5, -0.0 - 1.0, math.inf, -math.inf, math.nan):
        assert fwd(eps=bad) == ARG, bad


def test_unsupported_limits():
    wide = dict(C=L.NMSA_LNT_MAX_CHANNELS + 1, P=8, B=1)
    assert fwd(**wide) == UNSUPPORTED and bwd(**wide) == UNSUPPORTED and route(**wide) == UNSUPPORTED
    assert bwd(**dict(wide, C=L.NMSA_LNT_MAX_CHANNELS, **NOTHING)) == 0
    # B*P*C = 2^31: one element too many; one pixel less is accepted
    big = dict(B=1 << 10, P=1 << 10, C=1 << 11)
    assert fwd(**big) == UNSUPPORTED and bwd(**big) == UNSUPPORTED and route(**big) == UNSUPPORTED
    assert ws_bytes(1 << 10, 1 << 10, 1 << 11) == 0
    assert bwd(**dict(big, B=1, P=(1 << 20) - 1, **NOTHING)) == 0
    assert route(B=1, P=(1 << 20) - 8, C=1 << 11) == VECTOR


def test_misaligned_pointers():
    # off the element: refused.  Off 16 bytes only: the element route, not an error
    for name in ('x', 'y', 'add', 'gamma', 'beta', 'mean', 'rstd'):
        assert fwd(**{name: GOOD[name] + 1}) == ARG, name
        assert fwd(**{name: GOOD[name] + 2}) == ARG, name
    for name in ('gy', 'x', 'gx', 'gamma', 'mean', 'rstd', 'ggamma', 'gbeta'):
        assert bwd(**{name: GOOD[name] + 2}) == ARG, name
    half = dict(dtype_x=BF16, dtype_y=BF16)
    assert fwd(x=X + 1, **half) == ARG and fwd(y=Y + 1, **half) == ARG and fwd(add=ADD + 1, **half) == ARG
    assert bwd(gy=Y + 1, **half) == ARG and bwd(gx=GX + 1, **half) == ARG
    assert bwd(gy=Y + 2, **dict(half, **NOTHING)) == 0
    assert bwd(dtype_x=F16, dtype_y=F32, gy=Y + 2, **NOTHING) == ARG       # a float32 gy off its element
    assert route(x=X + 2) == ARG and route(x=X + 2, **half) == ELEMENT
    assert bwd(ws=WS + 4) == ARG and bwd(ws=WS + 8, gx=0) == ARG


def test_workspace():
    need = ws_bytes(2, 8, 8)
    assert need > 0
    for want in (dict(gx=0, gbeta=0), dict(gx=0, ggamma=0), dict()):
        assert bwd(ws_bytes=0, **want) == WORKSPACE and bwd(ws=0, **want) == ARG
        assert bwd(ws_bytes=need - 1, **want) == WORKSPACE
    assert bwd(ws_bytes=need - 1, **NOTHING) == 0                       # nothing wanted, none needed
    # a line [2][C] per workgroup: grows with the tiles until the grid is full, and with C
    assert ws_bytes(2, 8, 16) == 2 * need and ws_bytes(4, 8, 8) == 2 * need
    assert ws_bytes(2, 32, 8) == need and ws_bytes(2, 33, 8) == 2 * need
    sizes = [ws_bytes(16, n, 96) for n in (1, 32, 33, 1000, 19200, 100000)]
    assert sizes == sorted(sizes) and sizes[-1] == sizes[-2] > sizes[0]


def test_route_answers():
    # vector: C a multiple of 4 (float32 x) / 8 (half x), P of 4 (float32 y) / 8 (half y), both on 16 bytes
    for dx, dy in PAIRS:
        vx, vy = (4 if dx == F32 else 8), (4 if dy == F32 else 8)
        for Cn in range(1, 33):
            for Pn in (1, 2, 3, 4, 8, 12, 16, 31, 32, 33, 40):
                want = VECTOR if (Cn % vx == 0 and Pn % vy == 0) else ELEMENT
                assert route(dtype_x=dx, dtype_y=dy, C=Cn, P=Pn) == want, (dx, dy, Cn, Pn)
        ex, ey = (4 if dx == F32 else 2), (4 if dy == F32 else 2)
        for off in range(ex, 16, ex):
            assert route(dtype_x=dx, dtype_y=dy, x=X + off) == ELEMENT
        for off in range(ey, 16, ey):
            assert route(dtype_x=dx, dtype_y=dy, y=Y + off) == ELEMENT
        assert route(dtype_x=dx, dtype_y=dy, x=X + 16, y=Y + 48) == VECTOR
