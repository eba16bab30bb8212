"""GPU tier of the context module (csrc/context_module.hip, ops.ppm_*, model.context_module).

Oracle: the four operations written out in float64 on the CPU from the same, already dtype-rounded
inputs (`testing.context_ref.reference64`), the error bounds of `testing.context_ref.bounds`
(tests/test_context_module_host.py holds torch's own float32 to them and three defective
restatements out of them), and the recorded results of the reference's modules in
tests/golden/context_module.npz.

Launch geometry the shapes are picked from (csrc/context_module.hip): pool_fwd and upcat_bwd give a
plane to a wave, four planes to a workgroup (LDS route up to 2048 elements per plane and 512 row
sums per branch, GLOBAL route beyond); pool_bwd gives a lane a column and packs floor(64 / W) planes
into a wave; upcat_fwd walks the output in items of 1024 pixels of one plane.  So: B = 2 (a plane must
not run into the next image), C in {3, 8, 64} (not a multiple of four planes, one group per image,
several), maps from 1x1 to 30x40 (W = 9, 20, 40: lanes left over; 16, 32: none; 30x40: two items per
plane), bins with ph > H, overlapping windows (H % ph != 0) and equal ones.
"""
import pytest
import torch

from nicr_mt_scene_analysis_amd import _lib as L
from nicr_mt_scene_analysis_amd import ops
from nicr_mt_scene_analysis_amd.model import context_module as cm
from nicr_mt_scene_analysis_amd.model.context_module import ppm as ppm_mod
from nicr_mt_scene_analysis_amd.testing import context_cases as cc
from nicr_mt_scene_analysis_amd.testing import context_ref as R

import _golden

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = (F32, BF16, F16)
MODES = ('nearest', 'bilinear')
LDS, GLOBAL = L.NMSA_PPM_ROUTE_LDS, L.NMSA_PPM_ROUTE_GLOBAL
CR = 3                                      # channels of a branch: B * n * CR is no multiple of four planes
POISON = 12288.0                            # exact in bfloat16 and float16
APPM_SIZES = tuple((2 * b, 2 * b) for b in cc.APPM_BINS)


# ------------------------------------------------------------------------------ helpers
def dev(tensors):
    return tuple(None if t is None else t.to(DEV) for t in tensors)


def off_by_one(t):
    """the same values on the device, one element into a larger buffer: off 16 bytes, on the element"""
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=DEV)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def run_ops(x, ys, g_out, gps, sizes, mode, shift=False):
    """the four kernels on the device -> dict like reference64's"""
    place = (lambda t: off_by_one(t.to(DEV))) if shift else (lambda t: t.to(DEV))
    xd, g_outd = place(x), place(g_out)
    ysd, gpsd = tuple(place(y) for y in ys), tuple(place(g) for g in gps)
    return {'pooled': ops.ppm_pool(xd, sizes),
            'cat': ops.ppm_upsample_concat(xd, ysd, mode),
            'gys': ops.ppm_upsample_concat_backward(g_outd, x.shape[1], [tuple(y.shape) for y in ys], mode),
            'gx_pool': ops.ppm_pool_backward(gpsd, tuple(x.shape), sizes)}


def pairs(got, ref):
    """(key, got tensor, reference / bound tensor) over the four results"""
    for i, (g, r) in enumerate(zip(got['pooled'], ref['pooled'])):
        yield f'pooled{i}', g, r
    yield 'cat', got['cat'], ref['cat']
    for i, (g, r) in enumerate(zip(got['gys'], ref['gys'])):
        yield f'gys{i}', g, r
    yield 'gx_pool', got['gx_pool'], ref['gx_pool']


def check_exact(C, hw, dtype, mode, seed=0):
    sizes = cc.sizes_of(cc.EXACT_BINS)
    x, ys, g_out, gps = R.make_inputs(2, C, CR, hw, sizes, seed, dtype=dtype, integer=True)
    ref = R.reference64(x, sizes, ys, mode, g_out, gps)
    got = run_ops(x, ys, g_out, gps, sizes, mode)
    for key, g, r in pairs(got, ref):
        assert g.dtype == dtype and g.is_contiguous(), key
        assert torch.equal(g.cpu(), r.to(dtype)), (key, C, hw, dtype, mode)        # the exact value, cast once


def check_bounds(C, hw, sizes, dtype, mode, seed, shift=False):
    x, ys, g_out, gps = R.make_inputs(2, C, CR, hw, sizes, seed, dtype=dtype)
    ref = R.reference64(x, sizes, ys, mode, g_out, gps)
    bd = R.bounds(x, sizes, ys, mode, g_out, gps, dtype=dtype)
    got = run_ops(x, ys, g_out, gps, sizes, mode, shift)
    worst = {}
    for (key, g, r), (_, _, b) in zip(pairs(got, ref), pairs(got, bd)):
        assert g.dtype == dtype and tuple(g.shape) == tuple(r.shape), key
        worst[key] = R.worst_ratio(g, r, b)
    print('bounds', C, hw, sizes, dtype, mode, {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, (C, hw, sizes, dtype, mode, worst)
    assert torch.equal(got['cat'][:, :C].cpu(), x), 'the copy of x inside the concatenation'
    return got


# ------------------------------------------------------------------------------ exact tier
@pytest.mark.parametrize('C', cc.GPU_CHANNELS)
@pytest.mark.parametrize('hw', cc.EXACT_HW)
def test_exact_on_power_of_two_geometries(C, hw):
    """integer inputs in -8..8, bins (1, 2, 4, 8) over 8x16 and 16x32: every window area and resize
    weight is a power of two and every sum is exact in float32 in any order (held on the CPU by
    tests/test_context_module_host.py), so all four kernels must give the float64 value, cast once"""
    for dtype in DTYPES:
        for mode in MODES:
            check_exact(C, hw, dtype, mode)


# ------------------------------------------------------------------------------ bounds tier
@pytest.mark.parametrize('C', cc.GPU_CHANNELS)
@pytest.mark.parametrize('hw', cc.GPU_HW)
def test_bounds_on_normal_inputs(C, hw):
    for k, bins in enumerate(cc.GPU_BINS):
        for dtype in DTYPES:
            for mode in MODES:
                check_bounds(C, hw, cc.sizes_of(bins), dtype, mode, seed=100 + k)


@pytest.mark.parametrize('C', (3, 8))
def test_bounds_on_the_appm_geometry(C):
    """a 32x64 map for input_size (16, 32): pools (2, 4, 8, 16) squared, the largest plane of the LDS route"""
    assert ops.ppm_route(cc.APPM_HW, APPM_SIZES) == LDS
    for dtype in DTYPES:
        for mode in MODES:
            check_bounds(C, cc.APPM_HW, APPM_SIZES, dtype, mode, seed=7)


@pytest.mark.parametrize('hw,sizes,lds', cc.ROUTE_CASES)
def test_bounds_on_both_sides_of_the_route_limits(hw, sizes, lds):
    assert ops.ppm_route(hw, sizes) == (LDS if lds else GLOBAL)
    for dtype in DTYPES:
        for mode in MODES:
            check_bounds(5, hw, sizes, dtype, mode, seed=11)


def test_non_square_pools_and_pointers_off_16_bytes():
    """(ph, pw) pairs with ph > H and pw < W, and every tensor one element into a larger buffer: there is
    no alignment rule beyond the element, and the results are the bits of the aligned call"""
    sizes = ((5, 2), (1, 7), (4, 3))
    for dtype in DTYPES:
        for mode in MODES:
            a = check_bounds(3, (3, 9), sizes, dtype, mode, seed=5)
            b = check_bounds(3, (3, 9), sizes, dtype, mode, seed=5, shift=True)
            for (key, ta, _), (_, tb, _) in zip(pairs(a, a), pairs(b, b)):
                assert torch.equal(ta, tb), key


def test_unused_and_unwanted_branches():
    sizes = cc.sizes_of((1, 2, 3))
    x, ys, g_out, gps = R.make_inputs(2, 3, CR, (7, 9), sizes, 3)
    shapes = [tuple(y.shape) for y in ys]
    full = ops.ppm_upsample_concat_backward(g_out.to(DEV), 3, shapes, 'bilinear')
    part = ops.ppm_upsample_concat_backward(g_out.to(DEV), 3, shapes, 'bilinear', need=(True, False, True))
    assert part[1] is None and torch.equal(part[0], full[0]) and torch.equal(part[2], full[2])
    assert ops.ppm_upsample_concat_backward(g_out.to(DEV), 3, shapes, 'bilinear', need=(False,) * 3) == (None,) * 3
    gx = ops.ppm_pool_backward((gps[0].to(DEV), None, gps[2].to(DEV)), tuple(x.shape), sizes)
    ref = R.pool_backward64((gps[0], None, gps[2]), tuple(x.shape), sizes)
    bd = R.bounds(x, sizes, ys, 'nearest', None, (gps[0], None, gps[2]))['gx_pool']
    assert R.worst_ratio(gx, ref, bd) <= 1.0


# ------------------------------------------------------------------------------ the fixture
@pytest.fixture(scope='module')
def golden():
    return _golden.load('context_module')


KERNEL_CASES = [k for k, c in cc.CONTEXT_CASES.items() if c[0] != 'none']


def build(case):
    name, n_in, n_out, _, input_size, upsampling, _ = cc.CONTEXT_CASES[case] if isinstance(case, str) else case
    module = cm.get_context_module(name, n_in, n_out, input_size, upsampling=upsampling)
    inp = cc.make_context_inputs(case)
    module.load_state_dict({k: torch.from_numpy(v) for k, v in inp['state'].items()}, strict=False)
    return module.eval().to(DEV), inp


@pytest.mark.parametrize('case', KERNEL_CASES)
def test_kernels_against_the_recorded_intermediates(golden, case):
    """float32 kernels on the recorded inputs of every step: within TWICE the bounds of the recorded
    float32 intermediates (both sides are float32 evaluations within one bound of the truth)"""
    p = _golden.jload(golden[f'{case}__params'])
    inp = cc.make_context_inputs(case)
    n, mode = p['n_features'], p['upsampling']
    sizes = tuple(tuple(s) for s in p['sizes'])
    x = torch.from_numpy(inp['x'])
    C = x.shape[1]
    ys = tuple(torch.from_numpy(golden[f'{case}__feat{i}']) for i in range(n))
    gps = tuple(torch.from_numpy(golden[f'{case}__gpool{i}']) for i in range(n))
    g_cat = torch.from_numpy(golden[f'{case}__gcat'])
    got = run_ops(x, ys, g_cat, gps, sizes, mode)
    bd = R.bounds(x, sizes, ys, mode, g_cat, gps)
    worst = {}
    for i in range(n):
        worst[f'pool{i}'] = R.worst_ratio(got['pooled'][i], torch.from_numpy(golden[f'{case}__pool{i}']).double(),
                                          2 * bd['pooled'][i])
        worst[f'gfeat{i}'] = R.worst_ratio(got['gys'][i], torch.from_numpy(golden[f'{case}__gfeat{i}']).double(),
                                           2 * bd['gys'][i])
    worst['cat'] = R.worst_ratio(got['cat'], torch.from_numpy(golden[f'{case}__cat']).double(), 2 * bd['cat'])
    # gx = the x channels of g_cat plus the pools' gradient: n more float32 additions on either side,
    # each within u of the magnitudes it adds
    gx = g_cat[:, :C].to(DEV) + got['gx_pool']
    mag = g_cat[:, :C].double().abs() + R.pool_backward64([g.abs() for g in gps], tuple(x.shape), sizes)
    worst['gx'] = R.worst_ratio(gx, torch.from_numpy(golden[f'{case}__gx']).double(),
                                2 * bd['gx_pool'] + 2 * R.gamma(n + 1) * mag)
    print('fixture', case, {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, (case, worst)


def torch_twin(module, x, sizes, mode):
    """the module's parameters with adaptive_avg_pool2d / interpolate / cat"""
    feats = tuple(f[1](p) for f, p in zip(module.features, R.torch_pool(x, sizes)))
    return module.final_conv(R.torch_upcat(x, feats, mode)), feats


@pytest.mark.parametrize('case', KERNEL_CASES)
def test_module_against_the_fixture_end_to_end(golden, case):
    """eval mode, float32: the module's worst error against the recorded output must not exceed twice
    that of a torch-ops twin with the same parameters on the same device (two float32 evaluations of
    one formula in different summation orders)"""
    p = _golden.jload(golden[f'{case}__params'])
    module, inp = build(case)
    sizes = tuple(tuple(s) for s in p['sizes'])
    want = {'out': torch.from_numpy(golden[f'{case}__out']), 'gx': torch.from_numpy(golden[f'{case}__gx'])}
    errs = {}
    for who in ('module', 'twin'):
        x = torch.from_numpy(inp['x']).to(DEV).requires_grad_(True)
        out, feats = module(x) if who == 'module' else torch_twin(module, x, sizes, p['upsampling'])
        out.backward(torch.from_numpy(inp['gy']).to(DEV))
        assert len(feats) == p['n_features'] and tuple(out.shape) == tuple(want['out'].shape)
        for i, f in enumerate(feats):
            assert tuple(f.shape) == golden[f'{case}__feat{i}'].shape
        errs[who] = {'out': float((out.detach().cpu() - want['out']).abs().max()),
                     'gx': float((x.grad.cpu() - want['gx']).abs().max())}
    print('end-to-end', case, errs)
    for key in ('out', 'gx'):
        assert errs['module'][key] <= 2 * errs['twin'][key], (case, key, errs)


def test_train_mode_runs_and_matches_the_recorded_shapes(golden):
    train = _golden.jload(golden['train'])
    module, inp = build(cc.CONTEXT_TRAIN_CASE)
    module.train()
    x = torch.from_numpy(inp['x']).to(DEV).requires_grad_(True)
    out, feats = module(x)
    out.backward(torch.from_numpy(inp['gy']).to(DEV))
    assert list(out.shape) == train['out'] and [list(f.shape) for f in feats] == train['features']
    assert x.grad.shape == x.shape and bool(torch.isfinite(x.grad).all())
    assert all(q.grad is not None for q in module.parameters())


# ------------------------------------------------------------------------------ determinism
def test_same_bits_on_every_call_stream_and_graph_replay():
    sizes = cc.sizes_of((1, 2, 3, 6))
    for dtype in (F32, BF16):
        x, ys, g_out, gps = R.make_inputs(2, 8, CR, (15, 20), sizes, 9, dtype=dtype)
        xd, g_outd = x.to(DEV), g_out.to(DEV)
        ysd, gpsd = dev(ys), dev(gps)
        shapes = [tuple(y.shape) for y in ys]

        def call():
            return (ops.ppm_pool(xd, sizes) + (ops.ppm_upsample_concat(xd, ysd, 'bilinear'),) +
                    ops.ppm_upsample_concat_backward(g_outd, 8, shapes, 'bilinear') +
                    (ops.ppm_pool_backward(gpsd, tuple(x.shape), sizes),))

        first = call()
        torch.cuda.synchronize()
        for a, b in zip(first, call()):
            assert torch.equal(a, b)
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            on_side = call()
        side.synchronize()
        for a, b in zip(first, on_side):
            assert torch.equal(a, b)
        graph = torch.cuda.CUDAGraph()
        warm = torch.cuda.Stream(DEV)
        warm.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(warm):
            call()
        torch.cuda.current_stream(DEV).wait_stream(warm)
        with torch.cuda.graph(graph):
            captured = call()
        for t in captured:
            t.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(first, captured):
            assert torch.equal(a, b)


def test_out_is_written_in_place_and_the_guard_band_stays():
    sizes = cc.sizes_of((1, 5))
    for dtype in DTYPES:
        x, ys, _, _ = R.make_inputs(2, 3, CR, (7, 9), sizes, 4, dtype=dtype)
        xd, ysd = x.to(DEV), dev(ys)
        want = ops.ppm_upsample_concat(xd, ysd, 'bilinear')
        n, guard = want.numel(), 64
        buf = torch.full((n + 2 * guard,), POISON, dtype=dtype, device=DEV)
        out = buf[guard:guard + n].view(want.shape)
        back = ops.ppm_upsample_concat(xd, ysd, 'bilinear', out=out)
        assert back is out and torch.equal(out, want)
        assert bool((buf[:guard] == POISON).all()) and bool((buf[guard + n:] == POISON).all())
        with pytest.raises(TypeError):
            ops.ppm_upsample_concat(xd, ysd, 'bilinear', out=out[:, :-1])
        with pytest.raises(TypeError):
            ops.ppm_upsample_concat(xd, ysd, 'bilinear', out=out.float() if dtype != F32 else out.half())


def test_argument_checks_on_the_device():
    x = torch.zeros(2, 4, 5, 6, device=DEV)
    y = torch.zeros(2, 2, 1, 1, device=DEV)
    with pytest.raises(TypeError):
        ops.ppm_pool(x.double(), (1,))
    with pytest.raises(TypeError):
        ops.ppm_pool(x[0], (1,))
    with pytest.raises(ValueError):
        ops.ppm_pool(x, ())
    with pytest.raises(ValueError):
        ops.ppm_pool(x, (1, 2, 3, 4, 5))
    with pytest.raises(TypeError):
        ops.ppm_upsample_concat(x, (y.half(),), 'nearest')          # one dtype per call
    with pytest.raises(TypeError):
        ops.ppm_upsample_concat(x, (y[:1],), 'nearest')
    with pytest.raises(ValueError):
        ops.ppm_upsample_concat(x, (y,), 'bicubic')
    with pytest.raises(TypeError):
        ops.ppm_upsample_concat_backward(torch.zeros(2, 7, 5, 6, device=DEV), 4, ((2, 2, 1, 1),), 'nearest')
    with pytest.raises(TypeError):
        ops.ppm_pool_backward((torch.zeros(2, 4, 2, 2, device=DEV),), (2, 4, 5, 6), (1,))
    with pytest.raises(TypeError):
        ops.ppm_pool_backward((None,), (2, 4, 5, 6), (1,))
    # non-contiguous inputs are made contiguous: channels-last x, a permuted branch
    xs, ys, _, _ = R.make_inputs(2, 4, 2, (5, 6), ((2, 3),), 1)
    xs, ys = xs.to(DEV), dev(ys)
    cl = xs.to(memory_format=torch.channels_last)
    assert not cl.is_contiguous()
    assert torch.equal(ops.ppm_pool(cl, ((2, 3),))[0], ops.ppm_pool(xs, ((2, 3),))[0])
    yt = ys[0].permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not yt.is_contiguous()
    assert torch.equal(ops.ppm_upsample_concat(cl, (yt,), 'bilinear'), ops.ppm_upsample_concat(xs, ys, 'bilinear'))


# ------------------------------------------------------------------------------ wiring
def composition(module, x, sizes, mode, cast=None):
    """the module's forward and backward written with the ops' forward and backward functions"""
    x = x.detach()
    pooled = ops.ppm_pool(x, sizes)
    leaves = [p.detach().requires_grad_(True) for p in pooled]
    with torch.autocast('cuda', dtype=cast, enabled=cast is not None):
        feats = [f[1](p) for f, p in zip(module.features, leaves)]
    dtype = x.dtype
    for f in feats:
        dtype = torch.promote_types(dtype, f.dtype)
    ys = [f.detach().to(dtype) for f in feats]
    cat = ops.ppm_upsample_concat(x.to(dtype), ys, mode).requires_grad_(True)
    with torch.autocast('cuda', dtype=cast, enabled=cast is not None):
        out = module.final_conv(cat)
    return out, feats, leaves, cat, ys, dtype


@pytest.mark.parametrize('name,hw,input_size,mode', (('ppm-1-5-10', (15, 20), (15, 20), 'bilinear'),
                                                    ('ppm-1-2-4-8', (7, 9), (7, 9), 'nearest'),
                                                    ('appm-1-2-4-8', (16, 32), (8, 16), 'bilinear')))
def test_module_wiring_is_the_composition_of_the_ops(name, hw, input_size, mode):
    torch.manual_seed(0)
    module = cm.get_context_module(name, 16, 8, input_size, upsampling=mode).to(DEV).train()
    sizes = module.pool_sizes(*hw) if name.startswith('appm') else ops._ppm_sizes(module._bins)
    x = torch.randn(2, 16, *hw, device=DEV)
    gy = torch.randn(2, 8, *hw, device=DEV)
    params = list(module.parameters())

    def twin():
        """forward and backward of the composition -> (out, feats, the tensors that flow into and out of
        the kernels, the parameter gradients, gx); in train mode a forward changes the running
        statistics, not the result"""
        module.zero_grad(set_to_none=True)
        out2, feats2, leaves, cat, ys, _ = composition(module, x, sizes, mode)
        out2.backward(gy)
        g_cat = cat.grad
        gys = ops.ppm_upsample_concat_backward(g_cat, 16, [tuple(y.shape) for y in ys], mode)
        torch.autograd.backward(feats2, gys)
        gps = [p.grad for p in leaves]
        gx2 = g_cat[:, :16] + ops.ppm_pool_backward(gps, tuple(x.shape), sizes)
        flows = [g_cat] + list(gys) + gps
        return out2, feats2, flows, [q.grad.clone() for q in params], gx2

    out2, feats2, flows2, want, gx2 = twin()
    # torch's own convolution backward may pick another algorithm on another call: the parameter
    # gradients are compared where torch repeats its own bits, the tensors torch receives always
    torch_repeats = all(torch.equal(a, b) for a, b in zip(want, twin()[3]))
    module.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(True)
    flows = {}
    def tap(key):
        """a forward pre-hook that records the gradient of the module's input under `key`"""
        def pre_hook(_, args):
            args[0].register_hook(lambda g: flows.__setitem__(key, g))
        return pre_hook

    pre = [f[1].register_forward_pre_hook(tap(f'gp{i}')) for i, f in enumerate(module.features)]
    pre.append(module.final_conv.register_forward_pre_hook(tap('g_cat')))
    out, feats = module(xr)
    for i, f in enumerate(feats):
        f.register_hook(lambda g, i=i: flows.__setitem__(f'gy{i}', g) or None)
    for h in pre:
        h.remove()
    assert isinstance(feats, tuple) and len(feats) == len(sizes)
    assert torch.equal(out, out2)
    for a, b in zip(feats, feats2):
        assert torch.equal(a, b)
    out.backward(gy)
    n = len(sizes)
    got = [flows['g_cat']] + [flows[f'gy{i}'] for i in range(n)] + [flows[f'gp{i}'] for i in range(n)]
    for a, b in zip(got, flows2):
        assert torch.equal(a, b)
    assert torch.equal(xr.grad, gx2)
    print('wiring', name, 'torch repeats its parameter gradients:', torch_repeats)
    if torch_repeats:
        for q, w in zip(params, want):
            assert torch.equal(q.grad, w)
    # an input that needs no gradient: the same parameter gradients (the pools' backward is not asked)
    first = [q.grad.clone() for q in params]
    module.zero_grad(set_to_none=True)
    module(x)[0].backward(gy)
    if torch_repeats:
        for q, w in zip(params, first):
            assert torch.equal(q.grad, w)


@pytest.mark.parametrize('cast', (BF16, F16))
def test_autocast_is_the_explicit_cast_composition(cast):
    torch.manual_seed(1)
    module = cm.get_context_module('ppm-1-5', 16, 8, (7, 9)).to(DEV).eval()
    sizes = ops._ppm_sizes(module._bins)
    for x in (torch.randn(2, 16, 7, 9, device=DEV), torch.randn(2, 16, 7, 9, device=DEV).to(cast)):
        with torch.autocast('cuda', dtype=cast):
            out, feats = module(x)
        out2, feats2, _, cat, _, dtype = composition(module, x, sizes, 'bilinear', cast=cast)
        # float32 x with half branch outputs: the concatenation is float32 (torch.cat's promotion)
        assert cat.dtype == dtype == torch.promote_types(x.dtype, cast) and all(f.dtype == cast for f in feats)
        assert out.dtype == out2.dtype == cast and torch.equal(out, out2)
        for a, b in zip(feats, feats2):
            assert torch.equal(a, b)
    # the other way round: half x, float32 branches (no autocast, half input into float32 modules is
    # not a torch configuration; the functions are called directly)
    xh = torch.randn(2, 4, 7, 9, device=DEV).to(cast)
    y32 = torch.randn(2, 2, 5, 5, device=DEV)
    got = ppm_mod.UpsampleConcatFunction.apply('bilinear', xh.float(), y32)
    assert got.dtype == F32 and torch.equal(got[:, :4], xh.float())
