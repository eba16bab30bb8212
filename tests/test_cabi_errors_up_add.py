"""CPU tier: the host checks of the two entry points of csrc/up_add.hip, in the manner of
tests/test_cabi_errors_upsampling.py.  Every argument is checked before anything is enqueued, so a refused call
comes back with its code without a device: no call below reaches a HIP call and the made-up addresses are never
dereferenced.  That the unbroken arguments get past the checks is shown by the route query, which runs the same
checks and launches nothing."""
import ctypes as C

from nicr_mt_scene_analysis_amd import _lib as L

ARG, UNSUPPORTED = -1, -4
X, SKIP, Y, W, BIAS = (0x10000000 * (i + 1) for i in range(5))
GOOD = dict(x=X, dtype=L.NMSA_F32, mode=L.NMSA_UPADD_LEARNED, weight=W, bias=BIAS, skip=SKIP, B=2, C=3, h=5, w=6,
            y=Y)
VECTOR, PIXEL = L.NMSA_UPADD_ROUTE_VECTOR, L.NMSA_UPADD_ROUTE_PIXEL
MODES = (L.NMSA_UPADD_NEAREST, L.NMSA_UPADD_BILINEAR, L.NMSA_UPADD_LEARNED, L.NMSA_UPADD_LEARNED_ZEROPAD)
DTYPES = (L.NMSA_F32, L.NMSA_BF16, L.NMSA_F16)


def p(v):
    return C.c_void_p(v) if v else None


def fwd(**changes):
    a = dict(GOOD, **changes)
    return L.lib().nmsa_up2x_add_fwd(p(a['x']), a['dtype'], a['mode'], p(a['weight']), p(a['bias']), p(a['skip']),
                                     a['B'], a['C'], a['h'], a['w'], p(a['y']), None)


def route(**changes):
    a = dict(GOOD, **changes)
    return L.lib().nmsa_up2x_add_route(p(a['x']), p(a['skip']), p(a['y']), a['dtype'], a['B'], a['C'], a['h'],
                                       a['w'])


def test_constants():
    assert MODES == (0, 1, 2, 3) and (VECTOR, PIXEL) == (1, 2)
    for name in ('nmsa_up2x_add_route', 'nmsa_up2x_add_fwd'):
        assert name in L.declared_symbols() and name in L._SIGNATURES
    assert len(L._SIGNATURES['nmsa_up2x_add_route'][1]) == 8 and len(L._SIGNATURES['nmsa_up2x_add_fwd'][1]) == 12


def test_the_unbroken_arguments_pass_the_checks():
    for dtype in DTYPES:
        assert route(dtype=dtype) > 0


def test_null_pointers():
    for name in ('x', 'skip', 'y'):
        assert route(**{name: 0}) == ARG, name
        for mode in MODES:
            assert fwd(mode=mode, **{name: 0}) == ARG, (name, mode)
    # the weight is needed in the learned modes; a NULL bias is no bias, so it cannot be told apart without a device
    assert fwd(mode=L.NMSA_UPADD_LEARNED, weight=0) == ARG
    assert fwd(mode=L.NMSA_UPADD_LEARNED_ZEROPAD, weight=0) == ARG


def test_dtype_and_mode():
    for bad in (3, -1, 7):
        assert fwd(dtype=bad) == ARG and route(dtype=bad) == ARG, bad
    for bad in (4, -1, 9):
        assert fwd(mode=bad) == ARG, bad


def test_sizes_below_one():
    for name in ('B', 'C', 'h', 'w'):
        for bad in (0, -1):
            assert fwd(**{name: bad}) == ARG and route(**{name: bad}) == ARG, name


def test_misaligned_pointers():
    # off the element: refused.  Off 16 bytes only: the one-pixel route, not an error
    for name in ('x', 'skip', 'y'):
        assert fwd(**{name: GOOD[name] + 1}) == ARG and route(**{name: GOOD[name] + 2}) == ARG, name
        assert fwd(dtype=L.NMSA_BF16, **{name: GOOD[name] + 1}) == ARG, name
        assert route(dtype=L.NMSA_F16, **{name: GOOD[name] + 1}) == ARG, name
    for name in ('weight', 'bias'):
        assert fwd(**{name: GOOD[name] + 2}) == ARG, name


def test_an_output_that_overlaps_an_input_is_refused():
    e = 4
    n_in, n_out = 2 * 3 * 5 * 6 * e, 2 * 3 * 10 * 12 * e
    for name, n_other in (('x', n_in), ('skip', n_out)):
        other = GOOD[name]
        assert route(y=other) == ARG and fwd(y=other) == ARG, name                          # the same start
        assert route(y=other + n_other - e) == ARG and fwd(y=other + n_other - e) == ARG      # the last element
        assert route(y=other - n_out + e) == ARG and fwd(y=other - n_out + e) == ARG          # y's last on its first
        assert route(y=other + n_other) > 0 and route(y=other - n_out) > 0, name              # touching is fine
    assert route(dtype=L.NMSA_BF16, y=X + n_in // 2 - 2) == ARG and route(dtype=L.NMSA_BF16, y=X + n_in // 2) > 0
    assert route(x=SKIP) > 0            # the inputs may overlap each other


def test_what_is_too_large_is_unsupported():
    # 4hw = 2^31: one element too many for 32-bit offsets inside a plane; one row less passes
    big = dict(B=1, C=1, h=1 << 14, w=1 << 15, x=1 << 40, skip=1 << 44, y=1 << 48)
    assert fwd(**big) == UNSUPPORTED and route(**big) == UNSUPPORTED
    assert route(**dict(big, h=(1 << 14) - 1)) == VECTOR
    far = dict(x=1 << 40, skip=1 << 50, y=1 << 60)
    assert fwd(B=1 << 16, C=1 << 16, **far) == UNSUPPORTED and route(B=1 << 16, C=1 << 16, **far) == UNSUPPORTED
    # 2^31 work items: 2^31 - 1 planes of one chunk pass, of two chunks do not (the one-pixel route: two row tiles x 129
    # pixels are 258 lane units)
    assert route(B=(1 << 31) - 1, C=1, h=1, w=2, **far) == VECTOR
    assert route(B=(1 << 31) - 1, C=1, h=9, w=127, dtype=L.NMSA_BF16, **far) == PIXEL
    assert route(B=(1 << 31) - 1, C=1, h=9, w=129, dtype=L.NMSA_BF16, **far) == UNSUPPORTED
    assert fwd(B=(1 << 31) - 1, C=1, h=9, w=129, dtype=L.NMSA_BF16, **far) == UNSUPPORTED


def test_route_answers():
    for dtype, run in ((L.NMSA_F32, 2), (L.NMSA_BF16, 4), (L.NMSA_F16, 4)):
        e = 4 if dtype == L.NMSA_F32 else 2
        for w in range(1, 10):
            assert route(dtype=dtype, w=w) == (VECTOR if w % run == 0 else PIXEL), (dtype, w)
        for name in ('x', 'skip', 'y'):
            for shift in (e, 2 * e, 8):
                assert route(dtype=dtype, w=8, **{name: GOOD[name] + shift}) == PIXEL, (dtype, name, shift)
            assert route(dtype=dtype, w=8, **{name: GOOD[name] + 16}) == VECTOR, (dtype, name)
