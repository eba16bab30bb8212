"""CPU tier: the host checks of the seven encoder-fusion entry points (csrc/encoder_fusion.hip), in the
manner of tests/test_cabi_errors_mlp_decoder.py.  Every argument is checked before anything is
enqueued, so a refused call comes back with its code without a device: no call below reaches a HIP
call and the made-up addresses are never dereferenced.  That unbroken arguments get past the checks
is shown by the forms without a launch: weight_grad with no map, excite_bwd with no modality and
apply_bwd with no gradient wanted answer NMSA_OK from behind the last check, and nmsa_sefuse_route
answers a route.  (squeeze, excite and scale_add have no such form; the GPU tier runs them.)"""
import ctypes as C

from nicr_mt_scene_analysis_amd import _lib as L

ARG, UNSUPPORTED = -1, -4
VECTOR, ELEMENT = L.NMSA_SEFUSE_ROUTE_VECTOR, L.NMSA_SEFUSE_ROUTE_ELEMENT
WAVE, BLOCK = L.NMSA_SEFUSE_ROUTE_WAVE, L.NMSA_SEFUSE_ROUTE_BLOCK
F32, BF16, F16 = L.NMSA_F32, L.NMSA_BF16, L.NMSA_F16
RELU, SILU = L.NMSA_SEFUSE_ACT_RELU, L.NMSA_SEFUSE_ACT_SILU
XR, XD, Y, GY = 0x1000000, 0x2000000, 0x3000000, 0x4000000            # the maps
S, W, Z1, GW, GZ2, GZ1, GS, H = (0x5000000 + 0x100000 * i for i in range(8))     # the float32 vectors
PARAMS = tuple(0x6000000 + 0x100000 * i for i in range(8))
GOOD = dict(xr=XR, xd=XD, y=Y, gy=GY, dtype=F32, B=2, C=48, H=8, W=16, act=RELU, s=S, w=W, z1=Z1, gw=GW, gz2=GZ2,
            gz1=GZ1, gs=GS, h=H, params=PARAMS, weights=(PARAMS[0], PARAMS[2], PARAMS[4], PARAMS[6]))


def vp(v):
    return C.c_void_p(v) if v else None


def ptrs(values):
    return None if values is None else (C.c_void_p * len(values))(*(v or None for v in values))


def call(fn, **changes):
    a = dict(GOOD, **changes)
    lib = L.lib()
    if fn == 'squeeze':
        return lib.nmsa_sefuse_squeeze(vp(a['xr']), vp(a['xd']), a['dtype'], a['B'], a['C'], a['H'], a['W'], vp(a['s']), None)
    if fn == 'excite':
        return lib.nmsa_sefuse_excite(vp(a['s']), ptrs(a['params']), a['act'], a['B'], a['C'], vp(a['w']), vp(a['z1']), None)
    if fn == 'scale_add':
        return lib.nmsa_sefuse_scale_add(vp(a['xr']), vp(a['xd']), a['dtype'], vp(a['w']), a['B'], a['C'], a['H'],
                                         a['W'], vp(a['y']), None)
    if fn == 'weight_grad':
        return lib.nmsa_sefuse_weight_grad(vp(a['gy']), vp(a['xr']), vp(a['xd']), a['dtype'], a['B'], a['C'], a['H'],
                                           a['W'], vp(a['gw']), None)
    if fn == 'excite_bwd':
        return lib.nmsa_sefuse_excite_bwd(vp(a['gw']), vp(a['w']), vp(a['z1']), ptrs(a['weights']), a['act'], a['B'],
                                          a['C'], vp(a['gz2']), vp(a['gz1']), vp(a['gs']), vp(a['h']), None)
    if fn == 'apply_bwd':
        return lib.nmsa_sefuse_apply_bwd(vp(a['gy']), a['dtype'], vp(a['w']), vp(a['gs']), a['B'], a['C'], a['H'],
                                         a['W'], vp(a['xr']), vp(a['xd']), None)
    raise KeyError(fn)


def route(t0=XR, t1=XD, t2=Y, dtype=F32, H=8, W=16):
    return L.lib().nmsa_sefuse_route(vp(t0), vp(t1), vp(t2), dtype, H, W)


MAPS = ('squeeze', 'scale_add', 'weight_grad', 'apply_bwd')
VECS = ('excite', 'excite_bwd')
ALL = MAPS + VECS
# the forms that pass every check and launch nothing
NOTHING = {'weight_grad': dict(xr=0, xd=0), 'apply_bwd': dict(xr=0, xd=0), 'excite_bwd': dict(weights=(0, 0, 0, 0))}
# the pointers that may not be NULL, per entry point
NEEDED = {'squeeze': ('xr', 'xd', 's'), 'excite': ('s', 'params', 'w'), 'scale_add': ('xr', 'xd', 'w', 'y'),
          'weight_grad': ('gy', 'gw'), 'excite_bwd': ('gw', 'w', 'z1', 'weights', 'gz2', 'gz1', 'gs', 'h'),
          'apply_bwd': ('gy', 'w', 'gs')}


def test_the_unbroken_arguments_pass_the_checks():
    for fn, nothing in NOTHING.items():
        assert call(fn, **nothing) == 0, fn
        for dtype in (F32, BF16, F16):
            for act in (RELU, SILU):
                assert call(fn, dtype=dtype, act=act, **nothing) == 0, fn
        assert call(fn, C=16, **nothing) == 0 and call(fn, C=2048, B=1, H=1, W=1, **nothing) == 0, fn
    assert route() == VECTOR | WAVE


def test_null_pointers():
    for fn, names in NEEDED.items():
        for name in names:
            changes = {name: None if name in ('params', 'weights') else 0}
            assert call(fn, **changes) == ARG, (fn, name)
            if fn in NOTHING and name not in NOTHING[fn]:
                assert call(fn, **dict(NOTHING[fn], **changes)) == ARG, (fn, name)
    for k in range(8):
        assert call('excite', params=tuple(0 if i == k else p for i, p in enumerate(PARAMS))) == ARG, k
    # z1 of excite is optional; a modality of excite_bwd is given with both matrices or with neither
    for holes in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (0, 1, 0, 1)):
        weights = tuple(p if keep else 0 for p, keep in zip(GOOD['weights'], holes))
        assert call('excite_bwd', weights=weights) == ARG, holes
    assert route(t0=0) == ARG and route(t1=0, t2=0) == VECTOR | WAVE


def test_dtypes_and_activations():
    for bad in (3, -1, 7):
        for fn in MAPS:
            assert call(fn, dtype=bad) == ARG and call(fn, dtype=bad, **NOTHING.get(fn, {})) == ARG, (fn, bad)
        assert route(dtype=bad) == ARG
    for bad in (2, -1):
        for fn in VECS:
            assert call(fn, act=bad) == ARG and call(fn, act=bad, **NOTHING.get(fn, {})) == ARG, (fn, bad)


def test_sizes():
    for fn in ALL:
        names = ('B', 'C') if fn in VECS else ('B', 'C', 'H', 'W')
        for name in names:
            for bad in (0, -1):
                assert call(fn, **{name: bad}) == ARG, (fn, name, bad)
                assert call(fn, **dict(NOTHING.get(fn, {}), **{name: bad})) == ARG, (fn, name, bad)
        # the squeeze-and-excitation needs C // 16 >= 1
        for bad in (1, 8, 15):
            assert call(fn, C=bad) == ARG and call(fn, **dict(NOTHING.get(fn, {}), C=bad)) == ARG, (fn, bad)
    for bad in (0, -8):
        assert route(H=bad) == ARG and route(W=bad) == ARG


def test_unsupported_limits():
    # B*C*H*W stays below 2^31 (32-bit offsets)
    edge = dict(B=8, C=64, H=2048, W=2048)
    for fn in MAPS:
        assert call(fn, **edge) == UNSUPPORTED and call(fn, **dict(NOTHING.get(fn, {}), **edge)) == UNSUPPORTED, fn
        assert call(fn, **dict(edge, dtype=9)) == ARG and call(fn, **dict(edge, gy=0, xr=0, s=0)) == ARG, fn
    for fn in ('weight_grad', 'apply_bwd'):
        assert call(fn, **dict(NOTHING[fn], B=8, C=64, H=2048, W=2047)) == 0, fn
    # the excite kernels keep a channel vector in LDS
    for fn in VECS:
        assert call(fn, C=L.NMSA_SEFUSE_MAX_CHANNELS + 1) == UNSUPPORTED, fn
        assert call(fn, C=L.NMSA_SEFUSE_MAX_CHANNELS + 1, act=5) == ARG and call(fn, C=4096, w=0) == ARG, fn
    assert call('excite_bwd', C=L.NMSA_SEFUSE_MAX_CHANNELS, **NOTHING['excite_bwd']) == 0
    assert route(H=65536, W=65536) == UNSUPPORTED and route(H=65536, W=65536, dtype=4) == ARG


def test_misaligned_pointers():
    maps = {'squeeze': ('xr', 'xd'), 'scale_add': ('xr', 'xd', 'y'), 'weight_grad': ('gy', 'xr', 'xd'),
            'apply_bwd': ('gy', 'xr', 'xd')}
    for fn, names in maps.items():
        for name in names:
            for off in (1, 2, 3):
                assert call(fn, **{name: GOOD[name] + off}) == ARG, (fn, name, off)
            for half in (BF16, F16):
                assert call(fn, dtype=half, **{name: GOOD[name] + 1}) == ARG, (fn, name)
    assert call('weight_grad', gy=GY + 4, **NOTHING['weight_grad']) == 0
    assert call('weight_grad', gy=GY + 2, dtype=BF16, **NOTHING['weight_grad']) == 0
    vectors = {'squeeze': ('s',), 'excite': ('s', 'w', 'z1'), 'scale_add': ('w',), 'weight_grad': ('gw',),
               'excite_bwd': ('gw', 'w', 'z1', 'gz2', 'gz1', 'gs', 'h'), 'apply_bwd': ('w', 'gs')}
    for fn, names in vectors.items():
        for name in names:
            for off in (1, 2, 3):
                assert call(fn, **{name: GOOD[name] + off}) == ARG, (fn, name, off)
    for k in range(8):
        assert call('excite', params=tuple(p + 2 if i == k else p for i, p in enumerate(PARAMS))) == ARG, k
    for k in range(4):
        assert call('excite_bwd', weights=tuple(p + 2 if i == k else p for i, p in enumerate(GOOD['weights']))) == ARG
    for off in (1, 2, 3):
        assert route(t0=XR + off) == ARG and route(t1=XD + off) == ARG and route(t2=Y + off) == ARG
    assert route(t0=XR + 1, dtype=BF16) == ARG and route(t0=XR + 2, dtype=BF16) == ELEMENT | WAVE


def test_route_answers():
    # VECTOR: H*W on the vector width (4 float32, 8 half elements) and every tensor on 16 bytes
    for dtype in (F32, BF16, F16):
        assert route(dtype=dtype) == VECTOR | WAVE
    assert route(H=15, W=20) == VECTOR | WAVE                                   # 300 = 4 * 75
    assert route(H=15, W=20, dtype=BF16) == ELEMENT | WAVE and route(H=15, W=20, dtype=F16) == ELEMENT | WAVE
    assert route(H=3, W=5) == ELEMENT | WAVE and route(H=1, W=1) == ELEMENT | WAVE
    assert route(H=1, W=4) == VECTOR | WAVE and route(H=1, W=4, dtype=F16) == ELEMENT | WAVE
    assert route(H=2, W=4, dtype=F16) == VECTOR | WAVE
    for k in range(3):
        moved = [XR, XD, Y]
        moved[k] += 4
        assert route(*moved) == ELEMENT | WAVE, k
        moved[k] += 4
        assert route(*moved, dtype=BF16) == ELEMENT | WAVE, k
        moved[k] += 8
        assert route(*moved) == VECTOR | WAVE, k
    # tensors that are not part of the call are not looked at
    assert route(t1=0, t2=0) == VECTOR | WAVE and route(t0=XR + 4, t1=0, t2=0) == ELEMENT | WAVE
    # one wave up to NMSA_SEFUSE_WAVE_PLANE_MAX elements of a plane, one workgroup above
    n = L.NMSA_SEFUSE_WAVE_PLANE_MAX
    assert route(H=1, W=n) == VECTOR | WAVE and route(H=1, W=n + 1) == ELEMENT | BLOCK
    assert route(H=2, W=n // 2 + 2) == VECTOR | BLOCK and route(H=240, W=320, dtype=BF16) == VECTOR | BLOCK
