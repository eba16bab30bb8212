"""CPU tier: the host checks of the six batch-norm-tail entry points (csrc/block_tail.hip), in the manner of
tests/test_cabi_errors_encoder_fusion.py.  Every argument is checked before anything is enqueued, so a
refused call comes back with its code without a device: no call below reaches a HIP call and the made-up
addresses are never dereferenced.  That unbroken arguments get past the checks is shown by the forms
without a launch: nmsa_bntail_bwd_apply with nothing wanted answers NMSA_OK from behind the last check,
nmsa_bntail_route answers a route and nmsa_bntail_workspace_bytes a size.  (The other entry points share
their checks' code with these; the GPU tier runs them.)"""
import ctypes as C

from nicr_mt_scene_analysis_amd import _lib as L

ARG = -1
VECTOR, ELEMENT = L.NMSA_BNTAIL_ROUTE_VECTOR, L.NMSA_BNTAIL_ROUTE_ELEMENT
F32, BF16, F16 = L.NMSA_F32, L.NMSA_BF16, L.NMSA_F16
RELU, SILU = L.NMSA_BNTAIL_ACT_RELU, L.NMSA_BNTAIL_ACT_SILU
X, ID, Y, GY, GX, GID = (0x1000000 * (i + 1) for i in range(6))                # the maps
SCALE, GAMMA, BETA, RM, RV, MEAN, INVSTD, PART, DG, DB = (0x8000000 + 0x100000 * i for i in range(10))
GOOD = dict(x=X, identity=ID, y=Y, gy=GY, gx=GX, gid=GID, aux=Y, scale=SCALE, gamma=GAMMA, beta=BETA, rm=RM, rv=RV,
            mean=MEAN, invstd=INVSTD, part=PART, nbytes=1 << 20, dgamma=DG, dbeta=DB, save_mean=MEAN,
            save_invstd=INVSTD, dtype=F32, B=2, C=5, H=8, W=16, act=RELU)
MAPS = {'stats': ('x',), 'apply': ('x', 'identity', 'y'), 'bwd_reduce': ('gy', 'x', 'aux'),
        'bwd_apply': ('gy', 'x', 'aux', 'gx', 'gid')}
VECS = {'stats': ('part',), 'apply': ('gamma', 'beta', 'part', 'rm', 'rv', 'save_mean', 'save_invstd'),
        'bwd_reduce': ('gamma', 'beta', 'mean', 'invstd', 'part', 'dgamma', 'dbeta'),
        'bwd_apply': ('gamma', 'beta', 'mean', 'invstd', 'part', 'dgamma', 'dbeta')}
# the pointers that may not be NULL, per entry point (RELU; under SILU beta takes the place of aux)
NEEDED = {'stats': ('x', 'part'), 'apply': ('x', 'y', 'gamma', 'beta', 'rm', 'rv'),
          'bwd_reduce': ('gy', 'x', 'aux', 'gamma', 'mean', 'invstd', 'part'),
          'bwd_apply': ('gy', 'x', 'aux', 'gamma', 'mean', 'invstd')}
NOTHING = dict(gx=0, gid=0, dgamma=0, dbeta=0)                                 # bwd_apply: nothing wanted
ALL = tuple(MAPS)


def vp(v):
    return C.c_void_p(v) if v else None


def call(fn, **changes):
    a = dict(GOOD, **changes)
    lib = L.lib()
    shape = (a['dtype'], a['B'], a['C'], a['H'], a['W'])
    if fn == 'stats':
        return lib.nmsa_bntail_stats(vp(a['x']), *shape, vp(a['part']), a['nbytes'], None)
    if fn == 'apply':
        return lib.nmsa_bntail_apply(vp(a['x']), vp(a['identity']), vp(a['scale']), *shape, vp(a['gamma']), vp(a['beta']),
                                     vp(a['part']), a['nbytes'], vp(a['rm']), vp(a['rv']), 1e-5, 0.1, a['act'],
                                     vp(a['save_mean']), vp(a['save_invstd']), vp(a['y']), None)
    head = (vp(a['gy']), vp(a['x']), vp(a['aux']), vp(a['scale']), *shape, vp(a['gamma']), vp(a['beta']), vp(a['mean']),
            vp(a['invstd']), a['act'], vp(a['part']), a['nbytes'])
    if fn == 'bwd_reduce':
        return lib.nmsa_bntail_bwd_reduce(*head, vp(a['dgamma']), vp(a['dbeta']), None)
    if fn == 'bwd_apply':
        return lib.nmsa_bntail_bwd_apply(*head, vp(a['gx']), vp(a['gid']), vp(a['dgamma']), vp(a['dbeta']), None)
    raise KeyError(fn)


def route(t=(X, ID, Y, 0, 0), dtype=F32, H=8, W=16, want_segments=True):
    seg = C.c_int(-1)
    rc = L.lib().nmsa_bntail_route(*(vp(p) for p in t), dtype, H, W, C.byref(seg) if want_segments else None)
    return (rc, seg.value) if want_segments else rc


def refused(fn, **changes):
    """ARG, and for bwd_apply also in the form that launches nothing"""
    ok = call(fn, **changes) == ARG
    if fn == 'bwd_apply' and not set(changes) & set(NOTHING):
        ok = ok and call(fn, **dict(NOTHING, **changes)) == ARG
    return ok


def test_the_unbroken_arguments_pass_the_checks():
    assert call('bwd_apply', **NOTHING) == 0
    for dtype in (F32, BF16, F16):
        assert call('bwd_apply', dtype=dtype, **NOTHING) == 0
    assert call('bwd_apply', act=SILU, aux=0, **NOTHING) == 0 and call('bwd_apply', beta=0, **NOTHING) == 0
    assert call('bwd_apply', part=0, scale=0, **NOTHING) == 0
    assert call('bwd_apply', B=1, C=1, H=1, W=1, **NOTHING) == 0
    assert call('bwd_apply', B=8, C=64, H=2048, W=2047, nbytes=1 << 30, **NOTHING) == 0
    assert route() == (VECTOR, 1)
    assert L.lib().nmsa_bntail_workspace_bytes(2, 5, 8, 16) == 5 * 2 * 2 * 4
    assert L.lib().nmsa_bntail_workspace_bytes(3, 7, 3, 683) == 7 * 6 * 2 * 4


def test_null_pointers():
    for fn, names in NEEDED.items():
        for name in names:
            assert refused(fn, **{name: 0}), (fn, name)
    # SiLU recomputes z: beta is needed, the identity (aux) is not
    for fn in ('bwd_reduce', 'bwd_apply'):
        assert refused(fn, act=SILU, beta=0), fn
    # pairs: both or neither
    assert call('apply', save_mean=0) == ARG and call('apply', save_invstd=0) == ARG
    for fn in ('bwd_reduce', 'bwd_apply'):
        assert call(fn, dgamma=0) == ARG and call(fn, dbeta=0) == ARG, fn
    # the sums of bwd_apply come from the partials
    assert call('bwd_apply', part=0) == ARG and call('bwd_apply', part=0, dgamma=0, dbeta=0, gx=0, gid=0) == 0
    assert route(t=(0, ID, Y, 0, 0)) == (ARG, -1) and route(t=(X, 0, 0, 0, 0)) == (VECTOR, 1)
    assert route(want_segments=False) == VECTOR


def test_dtypes_and_activations():
    for bad in (3, -1, 7):
        for fn in ALL:
            assert refused(fn, dtype=bad), (fn, bad)
        assert route(dtype=bad)[0] == ARG
    for bad in (2, -1):
        for fn in ('apply', 'bwd_reduce', 'bwd_apply'):
            assert refused(fn, act=bad), (fn, bad)


def test_sizes():
    for fn in ALL:
        for name in ('B', 'C', 'H', 'W'):
            for bad in (0, -1):
                assert refused(fn, **{name: bad}), (fn, name, bad)
        # B*C*H*W stays below 2^31 (32-bit offsets)
        assert refused(fn, B=8, C=64, H=2048, W=2048, nbytes=1 << 30), fn
    for bad in (0, -8):
        assert route(H=bad)[0] == ARG and route(W=bad)[0] == ARG
    assert route(H=65536, W=65536)[0] == ARG
    assert L.lib().nmsa_bntail_workspace_bytes(0, 5, 8, 16) == 0 and L.lib().nmsa_bntail_workspace_bytes(8, 64, 2048, 2048) == 0
    # one value per channel has no unbiased variance: training only
    assert call('apply', B=1, H=1, W=1) == ARG


def test_workspace_too_small():
    need = L.lib().nmsa_bntail_workspace_bytes(2, 5, 8, 16)
    for fn in ALL:
        assert refused(fn, nbytes=need - 4), fn
    assert call('bwd_apply', nbytes=need, **NOTHING) == 0
    assert call('bwd_apply', nbytes=0, part=0, **NOTHING) == 0                  # no partials, no size


def test_misaligned_pointers():
    for fn, names in MAPS.items():
        for name in names:
            for off in (1, 2, 3):
                assert refused(fn, **{name: GOOD[name] + off}), (fn, name, off)
            for half in (BF16, F16):
                assert refused(fn, dtype=half, **{name: GOOD[name] + 1}), (fn, name)
    for fn in ('apply', 'bwd_reduce', 'bwd_apply'):
        assert refused(fn, scale=SCALE + 1) and refused(fn, scale=SCALE + 1, dtype=BF16), fn
    assert call('bwd_apply', gy=GY + 4, **NOTHING) == 0 and call('bwd_apply', gy=GY + 2, dtype=BF16, **NOTHING) == 0
    for fn, names in VECS.items():
        for name in names:
            for off in (1, 2, 3):
                assert refused(fn, **{name: GOOD[name] + off}), (fn, name, off)
    for k in range(5):
        for off in (1, 2, 3):
            t = [X, ID, Y, GX, GID]
            t[k] += off
            assert route(t=tuple(t))[0] == ARG, (k, off)
    assert route(t=(X + 1, 0, 0, 0, 0), dtype=BF16)[0] == ARG and route(t=(X + 2, 0, 0, 0, 0), dtype=BF16) == (ELEMENT, 1)


def test_route_answers():
    # VECTOR: H*W on the vector width (4 float32, 8 half elements) and every map on 16 bytes
    for dtype in (F32, BF16, F16):
        assert route(dtype=dtype) == (VECTOR, 1)
    assert route(H=15, W=20) == (VECTOR, 1)                                       # 300 = 4 * 75
    assert route(H=15, W=20, dtype=BF16) == (ELEMENT, 1) and route(H=15, W=20, dtype=F16) == (ELEMENT, 1)
    assert route(H=3, W=5) == (ELEMENT, 1) and route(H=1, W=1) == (ELEMENT, 1)
    assert route(H=1, W=4) == (VECTOR, 1) and route(H=1, W=4, dtype=F16) == (ELEMENT, 1)
    assert route(H=2, W=4, dtype=F16) == (VECTOR, 1)
    for k in range(5):
        t = [X, ID, Y, GX, GID]
        t[k] += 4
        assert route(t=tuple(t)) == (ELEMENT, 1), k
        t[k] += 4
        assert route(t=tuple(t), dtype=BF16) == (ELEMENT, 1), k
        t[k] += 8
        assert route(t=tuple(t)) == (VECTOR, 1), k
    # maps that are not part of the call are not looked at
    assert route(t=(X + 4, 0, 0, 0, 0)) == (ELEMENT, 1)
    # the units of a plane: segments of NMSA_BNTAIL_SEGMENT elements
    n = L.NMSA_BNTAIL_SEGMENT
    assert route(H=1, W=n) == (VECTOR, 1) and route(H=1, W=n + 1) == (ELEMENT, 2) and route(H=2, W=n) == (VECTOR, 2)
    assert route(H=120, W=160, dtype=BF16) == (VECTOR, 10) and route(H=3, W=683) == (ELEMENT, 2)
