"""CPU tier: the host checks of the three MLP-decoder entry points (csrc/mlp_decoder.hip), in the
manner of tests/test_cabi_errors_context_module.py.  Every argument is checked before anything is
enqueued, so a refused call comes back with its code without a device: no call below reaches a HIP
call and the made-up addresses are never dereferenced.  That unbroken arguments get past the checks
is shown by the calls that have a form without a launch: nmsa_mlpdec_upcat_bwd with no gradient
wanted answers NMSA_OK from behind the last check, and nmsa_mlpdec_route answers a route.  (The
forward has no such form; its unbroken arguments are run by the GPU tier.)"""
import ctypes as C

from nicr_mt_scene_analysis_amd import _lib as L

ARG, UNSUPPORTED = -1, -4
VECTOR, ELEMENT = L.NMSA_MLPDEC_ROUTE_VECTOR, L.NMSA_MLPDEC_ROUTE_ELEMENT
OUT = 0x200000
P = tuple(0x1000000 * (i + 1) for i in range(4))            # the per-branch tensors
F32, BF16, F16 = L.NMSA_F32, L.NMSA_BF16, L.NMSA_F16
GOOD = dict(out=OUT, dtype=F32, B=2, H=8, W=16, n=3, c=(3, 2, 4), s=(3, 1, 0), p=P[:3], mode=L.NMSA_MLPDEC_BILINEAR)
MAX_DIM = 32768


def vp(v):
    return C.c_void_p(v) if v else None


def ints(values):
    return None if values is None else (C.c_int * max(len(values), 1))(*values)


def ptrs(values):
    return None if values is None else (C.c_void_p * max(len(values), 1))(*(v or None for v in values))


def args(changes):
    return dict(GOOD, **changes)


def fwd(**changes):
    a = args(changes)
    return L.lib().nmsa_mlpdec_upcat_fwd(ptrs(a['p']), a['dtype'], a['B'], a['H'], a['W'], a['n'], ints(a['c']),
                                         ints(a['s']), a['mode'], vp(a['out']), None)


def bwd(**changes):
    a = args(changes)
    return L.lib().nmsa_mlpdec_upcat_bwd(vp(a['out']), a['dtype'], a['B'], a['H'], a['W'], a['n'], ints(a['c']),
                                         ints(a['s']), a['mode'], ptrs(a['p']), None)


def route(**changes):
    a = args(changes)
    return L.lib().nmsa_mlpdec_route(ptrs(a['p']), vp(a['out']), a['dtype'], a['H'], a['W'], a['n'], ints(a['s']))


BOTH = (fwd, bwd)
NOTHING = dict(p=(0, 0, 0))


def test_the_unbroken_arguments_pass_the_checks():
    assert bwd(**NOTHING) == 0
    for dtype in (F32, BF16, F16):
        for mode in (L.NMSA_MLPDEC_NEAREST, L.NMSA_MLPDEC_BILINEAR):
            assert bwd(dtype=dtype, mode=mode, **NOTHING) == 0
    assert bwd(n=1, c=(1,), s=(0,), p=(0,)) == 0
    assert bwd(n=4, H=16, W=32, c=(6, 5, 4, 3), s=(4, 2, 1, 0), p=(0, 0, 0, 0)) == 0
    assert route() == VECTOR


def test_null_pointers():
    assert fwd(out=0) == ARG and bwd(out=0) == ARG and bwd(out=0, **NOTHING) == ARG and route(out=0) == ARG
    for fn in BOTH:
        assert fn(p=None) == ARG and fn(c=None) == ARG and fn(s=None) == ARG, fn.__name__
    assert route(p=None) == ARG and route(s=None) == ARG
    # every branch map is needed forward; a NULL gradient is "not wanted"
    for k in range(3):
        holed = tuple(0 if i == k else P[i] for i in range(3))
        assert fwd(p=holed) == ARG and route(p=holed) == ARG, k


def test_dtypes_and_modes():
    for bad in (3, -1, 7):
        assert fwd(dtype=bad) == ARG and bwd(dtype=bad) == ARG and bwd(dtype=bad, **NOTHING) == ARG
        assert route(dtype=bad) == ARG
    for bad in (2, -1):
        assert fwd(mode=bad) == ARG and bwd(mode=bad) == ARG and bwd(mode=bad, **NOTHING) == ARG


def test_sizes_below_one():
    for name in ('B', 'H', 'W'):
        for bad in (0, -1):
            for fn in BOTH:
                assert fn(**{name: bad}) == ARG, (fn.__name__, name, bad)
            assert bwd(**dict(NOTHING, **{name: bad})) == ARG
    for bad in (0, -16):
        assert route(H=bad) == ARG and route(W=bad) == ARG
    for k in range(3):
        for bad in (0, -1):
            c = tuple(bad if i == k else GOOD['c'][i] for i in range(3))
            assert fwd(c=c) == ARG and bwd(c=c) == ARG and bwd(c=c, **NOTHING) == ARG, (k, bad)


def test_branch_count():
    five = dict(n=5, c=(1,) * 5, s=(0,) * 5, p=(P[0],) * 5)
    for fn in BOTH:
        assert fn(**five) == ARG and fn(n=0) == ARG and fn(n=-1) == ARG, fn.__name__
    assert route(**five) == ARG and route(n=0) == ARG
    assert L.NMSA_MLPDEC_MAX_BRANCHES == 4
    assert bwd(n=4, c=(1,) * 4, s=(0,) * 4, p=(0,) * 4) == 0


def test_shifts():
    for k in range(3):
        for bad in (-1, 5, 31):
            s = tuple(bad if i == k else GOOD['s'][i] for i in range(3))
            assert fwd(s=s, H=64, W=64) == ARG and bwd(s=s, H=64, W=64) == ARG and route(s=s, H=64, W=64) == ARG
    assert bwd(H=16, W=16, s=(4, 4, 4), **NOTHING) == 0
    # H and W are multiples of 1 << s_i for every branch
    for name, bad in (('H', 12), ('W', 20), ('H', 4), ('W', 7)):
        assert fwd(**{name: bad}) == ARG and bwd(**{name: bad}) == ARG and route(**{name: bad}) == ARG, (name, bad)
        assert bwd(**dict(NOTHING, **{name: bad})) == ARG
    assert bwd(H=12, W=20, s=(2, 1, 0), **NOTHING) == 0
    # branches beyond n are not looked at
    assert bwd(n=2, H=2, W=2, c=(1, 1, 0), s=(1, 0, 9), **NOTHING) == 0


def test_unsupported_limits():
    flat = dict(s=(0, 0, 0))
    for name in ('H', 'W'):
        for fn in BOTH:
            assert fn(**dict(flat, **{name: MAX_DIM + 1})) == UNSUPPORTED, (fn.__name__, name)
        assert route(**dict(flat, **{name: MAX_DIM + 1})) == UNSUPPORTED
        assert bwd(**dict(NOTHING, **{name: MAX_DIM})) == 0 and route(**{name: MAX_DIM}) == VECTOR
        # the argument checks come first
        assert fwd(**dict(flat, mode=2, **{name: MAX_DIM + 1})) == ARG
        assert fwd(**dict(flat, out=0, **{name: MAX_DIM + 1})) == ARG
    # B * sum(c) stays below 2^31
    edge = dict(B=1 << 16, c=(1 << 14, 1 << 13, 1 << 13))
    assert fwd(**edge) == UNSUPPORTED and bwd(**edge) == UNSUPPORTED and bwd(**dict(edge, **NOTHING)) == UNSUPPORTED
    assert bwd(**dict(edge, c=(1 << 14, 1 << 13, (1 << 13) - 1), **NOTHING)) == 0
    # 2^31 or more work items: 2^21 planes of 2^20 pixels are 2^31 forward items of 1024 pixels and
    # 2^33 backward items of 256 source pixels
    many = dict(B=1 << 10, n=1, c=(1 << 11,), s=(0,), H=1024, W=1024)
    assert fwd(p=(P[0],), **many) == UNSUPPORTED and bwd(p=(P[0],), **many) == UNSUPPORTED
    assert bwd(p=(0,), **many) == 0


def test_misaligned_pointers():
    for off in (1, 2, 3):
        assert fwd(out=OUT + off) == ARG and bwd(out=OUT + off) == ARG and route(out=OUT + off) == ARG
        for k in range(3):
            moved = tuple(P[i] + off if i == k else P[i] for i in range(3))
            assert fwd(p=moved) == ARG and bwd(p=moved) == ARG and route(p=moved) == ARG, (k, off)
    for half in (BF16, F16):
        assert fwd(out=OUT + 1, dtype=half) == ARG and bwd(out=OUT + 1, dtype=half) == ARG
        assert bwd(p=(P[0] + 1, 0, 0), dtype=half) == ARG
        assert bwd(out=OUT + 2, dtype=half, **NOTHING) == 0
    assert bwd(out=OUT + 4, **NOTHING) == 0


def test_route_answers():
    # VECTOR: W on the vector width (4 float32, 8 half pixels) and every tensor on 16 bytes
    assert route() == VECTOR and route(dtype=BF16) == VECTOR and route(dtype=F16) == VECTOR
    assert route(W=8, s=(3, 1, 0)) == VECTOR and route(W=8, s=(3, 1, 0), dtype=BF16) == VECTOR
    assert route(W=4, s=(2, 1, 0)) == VECTOR and route(W=4, s=(2, 1, 0), dtype=F16) == ELEMENT
    assert route(W=6, s=(1, 1, 0)) == ELEMENT and route(W=5, s=(0, 0, 0)) == ELEMENT
    assert route(out=OUT + 4) == ELEMENT and route(out=OUT + 2, dtype=BF16) == ELEMENT
    for k in range(3):
        moved = tuple(P[i] + 8 if i == k else P[i] for i in range(3))
        assert route(p=moved) == ELEMENT, k
    # branches beyond n are not looked at
    assert route(n=2, p=(P[0], P[1], P[2] + 4)) == VECTOR
