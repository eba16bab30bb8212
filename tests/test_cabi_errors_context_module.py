"""CPU tier: the host checks of the five context-module entry points (csrc/context_module.hip), in
the manner of tests/test_cabi_errors_fusion.py.  Every argument is checked before anything is
enqueued, so a refused call comes back with its code without a device: no call below reaches a HIP
call and the made-up addresses are never dereferenced.  That unbroken arguments get past the checks
is shown by the one call that has a form without a launch: nmsa_ppm_upcat_bwd with no gradient
wanted answers NMSA_OK from behind the last check.  (The other three have no such form; their
unbroken arguments are run by the GPU tier.)"""
import ctypes as C

from nicr_mt_scene_analysis_amd import _lib as L

ARG, UNSUPPORTED = -1, -4
LDS, GLOBAL = L.NMSA_PPM_ROUTE_LDS, L.NMSA_PPM_ROUTE_GLOBAL
X, OUT, GX = 0x100000, 0x200000, 0x300000
P = tuple(0x1000000 * (i + 1) for i in range(4))            # the per-branch tensors
F32, BF16, F16 = L.NMSA_F32, L.NMSA_BF16, L.NMSA_F16
GOOD = dict(x=X, out=OUT, gx=GX, dtype=F32, B=2, C=8, H=7, W=9, n=3, ph=(1, 2, 5), pw=(1, 3, 5), cr=(2, 2, 3),
            p=P[:3], mode=L.NMSA_PPM_BILINEAR)
MAX_DIM = 32768


def vp(v):
    return C.c_void_p(v) if v else None


def ints(values):
    return None if values is None else (C.c_int * max(len(values), 1))(*values)


def ptrs(values):
    return None if values is None else (C.c_void_p * max(len(values), 1))(*(v or None for v in values))


def args(changes):
    return dict(GOOD, **changes)


def pool_fwd(**changes):
    a = args(changes)
    return L.lib().nmsa_ppm_pool_fwd(vp(a['x']), a['dtype'], a['B'], a['C'], a['H'], a['W'], a['n'], ints(a['ph']),
                                     ints(a['pw']), ptrs(a['p']), None)


def pool_bwd(**changes):
    a = args(changes)
    return L.lib().nmsa_ppm_pool_bwd(ptrs(a['p']), a['dtype'], a['B'], a['C'], a['H'], a['W'], a['n'], ints(a['ph']),
                                     ints(a['pw']), vp(a['gx']), None)


def upcat_fwd(**changes):
    a = args(changes)
    return L.lib().nmsa_ppm_upcat_fwd(vp(a['x']), ptrs(a['p']), a['dtype'], a['B'], a['C'], a['H'], a['W'], a['n'],
                                      ints(a['cr']), ints(a['ph']), ints(a['pw']), a['mode'], vp(a['out']), None)


def upcat_bwd(**changes):
    a = args(changes)
    return L.lib().nmsa_ppm_upcat_bwd(vp(a['out']), a['dtype'], a['B'], a['C'], a['H'], a['W'], a['n'], ints(a['cr']),
                                      ints(a['ph']), ints(a['pw']), a['mode'], ptrs(a['p']), None)


def route(**changes):
    a = args(changes)
    return L.lib().nmsa_ppm_route(a['H'], a['W'], a['n'], ints(a['ph']), ints(a['pw']))


ALL = (pool_fwd, pool_bwd, upcat_fwd, upcat_bwd)
NOTHING = dict(p=(0, 0, 0))


def test_the_unbroken_arguments_pass_the_checks():
    assert upcat_bwd(**NOTHING) == 0
    for dtype in (F32, BF16, F16):
        for mode in (L.NMSA_PPM_NEAREST, L.NMSA_PPM_BILINEAR):
            assert upcat_bwd(dtype=dtype, mode=mode, **NOTHING) == 0
    assert upcat_bwd(n=1, ph=(9,), pw=(11,), cr=(1,), p=(0,)) == 0           # ph > H
    assert upcat_bwd(n=4, ph=(1, 2, 3, 6), pw=(1, 2, 3, 6), cr=(2, 2, 2, 2), p=(0, 0, 0, 0)) == 0
    assert route() == LDS


def test_null_pointers():
    assert pool_fwd(x=0) == ARG and upcat_fwd(x=0) == ARG
    assert pool_bwd(gx=0) == ARG
    assert upcat_fwd(out=0) == ARG and upcat_bwd(out=0) == ARG and upcat_bwd(out=0, **NOTHING) == ARG
    for fn in ALL:
        assert fn(p=None) == ARG and fn(ph=None) == ARG and fn(pw=None) == ARG, fn.__name__
    assert upcat_fwd(cr=None) == ARG and upcat_bwd(cr=None) == ARG
    assert route(ph=None) == ARG and route(pw=None) == ARG
    # every pooled map and every branch output is needed; a NULL gradient is "not used" / "not wanted"
    for k in range(3):
        holed = tuple(0 if i == k else P[i] for i in range(3))
        assert pool_fwd(p=holed) == ARG and upcat_fwd(p=holed) == ARG, k


def test_dtypes_and_modes():
    for bad in (3, -1, 7):
        for fn in ALL:
            assert fn(dtype=bad) == ARG, (fn.__name__, bad)
        assert upcat_bwd(dtype=bad, **NOTHING) == ARG
    for bad in (2, -1):
        assert upcat_fwd(mode=bad) == ARG and upcat_bwd(mode=bad) == ARG and upcat_bwd(mode=bad, **NOTHING) == ARG


def test_sizes_below_one():
    for name in ('B', 'C', 'H', 'W'):
        for bad in (0, -1):
            for fn in ALL:
                assert fn(**{name: bad}) == ARG, (fn.__name__, name, bad)
    for bad in (0, -3):
        assert route(H=bad) == ARG and route(W=bad) == ARG
    for name in ('ph', 'pw'):
        for k in range(3):
            for bad in (0, -1):
                sizes = tuple(bad if i == k else GOOD[name][i] for i in range(3))
                for fn in ALL:
                    assert fn(**{name: sizes}) == ARG, (fn.__name__, name, k, bad)
                assert route(**{name: sizes}) == ARG
    for k in range(3):
        for bad in (0, -1):
            cr = tuple(bad if i == k else GOOD['cr'][i] for i in range(3))
            assert upcat_fwd(cr=cr) == ARG and upcat_bwd(cr=cr) == ARG and upcat_bwd(cr=cr, **NOTHING) == ARG


def test_branch_count():
    five = dict(n=5, ph=(1,) * 5, pw=(1,) * 5, cr=(1,) * 5, p=(P[0],) * 5)
    for fn in ALL:
        assert fn(**five) == ARG and fn(n=0) == ARG and fn(n=-1) == ARG, fn.__name__
    assert route(**five) == ARG and route(n=0) == ARG
    assert L.NMSA_PPM_MAX_BINS == 4
    assert upcat_bwd(n=4, ph=(1,) * 4, pw=(1,) * 4, cr=(1,) * 4, p=(0,) * 4) == 0


def test_unsupported_limits():
    for name in ('H', 'W'):
        for fn in ALL:
            assert fn(**{name: MAX_DIM + 1}) == UNSUPPORTED, (fn.__name__, name)
        assert route(**{name: MAX_DIM + 1}) == UNSUPPORTED
        assert upcat_bwd(**dict(NOTHING, **{name: MAX_DIM})) == 0 and route(**{name: MAX_DIM}) == GLOBAL
    for name in ('ph', 'pw'):
        big = (1, MAX_DIM + 1, 5)
        for fn in ALL:
            assert fn(**{name: big}) == UNSUPPORTED, (fn.__name__, name)
        assert route(**{name: big}) == UNSUPPORTED
        assert upcat_bwd(**dict(NOTHING, **{name: (1, MAX_DIM, 5)})) == 0
    # B * C, and B * (C + sum cr), stay below 2^31
    for fn in ALL:
        assert fn(B=1 << 16, C=1 << 15) == UNSUPPORTED, fn.__name__
    edge = dict(B=1 << 16, C=(1 << 15) - 7)                     # B * C below 2^31, B * (C + 7) = 2^31
    assert upcat_fwd(**edge) == UNSUPPORTED and upcat_bwd(**edge) == UNSUPPORTED
    assert upcat_bwd(**dict(edge, C=(1 << 15) - 8, **NOTHING)) == 0


def test_misaligned_pointers():
    # off the element: refused (there is no other alignment rule: every access is element-wise)
    for off in (1, 2, 3):
        assert pool_fwd(x=X + off) == ARG and upcat_fwd(x=X + off) == ARG and upcat_fwd(out=OUT + off) == ARG
        assert pool_bwd(gx=GX + off) == ARG and upcat_bwd(out=OUT + off) == ARG
        for k in range(3):
            moved = tuple(P[i] + off if i == k else P[i] for i in range(3))
            for fn in ALL:
                assert fn(p=moved) == ARG, (fn.__name__, k, off)
    for half in (BF16, F16):
        assert pool_fwd(x=X + 1, dtype=half) == ARG and upcat_fwd(out=OUT + 1, dtype=half) == ARG
        assert pool_bwd(gx=GX + 1, dtype=half) == ARG and upcat_bwd(out=OUT + 1, dtype=half) == ARG
        assert upcat_bwd(p=(P[0] + 1, 0, 0), dtype=half) == ARG
        assert upcat_bwd(out=OUT + 2, dtype=half, **NOTHING) == 0
    assert upcat_bwd(out=OUT + 4, **NOTHING) == 0


def test_route_answers():
    # LDS: the plane has at most 2048 elements and H * pw_i at most 512 for every branch
    for H, W, want in ((32, 64, LDS), (64, 32, LDS), (1, 2048, LDS), (2048, 1, GLOBAL), (1, 2049, GLOBAL),
                       (3, 683, GLOBAL), (33, 62, LDS), (33, 63, GLOBAL), (1, 1, LDS)):
        assert route(H=H, W=W, n=1, ph=(1,), pw=(1,)) == want, (H, W)
    for H, pw, want in ((64, 8, LDS), (64, 9, GLOBAL), (32, 16, LDS), (32, 17, GLOBAL), (3, 170, LDS), (3, 171, GLOBAL),
                        (1, 512, LDS), (1, 513, GLOBAL)):
        for k in range(4):
            pws = tuple(pw if i == k else 1 for i in range(4))
            assert route(H=H, W=2048 // H, n=4, ph=(1, 1, 1, 1), pw=pws) == want, (H, pw, k)
    # ph does not matter, and branches beyond n_bins are not looked at
    assert route(H=8, W=8, n=2, ph=(MAX_DIM, 1), pw=(1, 1)) == LDS
    assert route(H=64, W=8, n=1, ph=(1, 1), pw=(8, 9)) == LDS
