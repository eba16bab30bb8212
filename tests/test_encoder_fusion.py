"""GPU tier of the encoder RGB-D fusion: the six `ops.sefuse_*` kernels one by one and the whole module
through autograd, against the float64 restatement and the derived bounds of
testing/encoder_fusion_ref.py (exact equality on constructed inputs), the recorded reference module,
both routes and off-16-byte tensors, determinism, gradient subsets, the fallbacks and autocast."""
import os

import pytest
import torch

from nicr_mt_scene_analysis_amd import _lib as L
from nicr_mt_scene_analysis_amd import model
from nicr_mt_scene_analysis_amd import ops
from nicr_mt_scene_analysis_amd.model.activation import get_activation_class
from nicr_mt_scene_analysis_amd.testing import encoder_fusion_cases as EC
from nicr_mt_scene_analysis_amd.testing import encoder_fusion_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = (F32, BF16, F16)
VECTOR, ELEMENT = L.NMSA_SEFUSE_ROUTE_VECTOR, L.NMSA_SEFUSE_ROUTE_ELEMENT
WAVE, BLOCK = L.NMSA_SEFUSE_ROUTE_WAVE, L.NMSA_SEFUSE_ROUTE_BLOCK
B = EC.B
POISON = -1024.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'encoder_fusion.npz')
MODULE_KEYS = ('y', 'gx_rgb', 'gx_depth') + R.PARAM_GRADS


def dev(t):
    return t.to(DEV)


def dev_params(params, dtype=F32):
    return tuple(tuple(p.to(DEV, dtype) for p in group) for group in params)


class Moved:
    """a tensor one element into a larger buffer (off 16 bytes), poison around it"""

    def __init__(self, like, fill=None):
        n = like.numel()
        self.buf = torch.full((n + 16,), POISON, dtype=like.dtype, device=DEV)
        self.t = self.buf[1:1 + n].view(like.shape)
        if fill is not None:
            self.t.copy_(fill)
        assert self.t.data_ptr() % 16 != 0 and self.t.is_contiguous()

    def untouched(self):
        n = self.t.numel()
        return bool((self.buf[:1] == POISON).all()) and bool((self.buf[1 + n:] == POISON).all())


def build(name, C, act, layout='nchw'):
    return model.get_encoder_fusion_class(name)(n_channels_in=C, input_memory_layout=layout,
                                                activation=get_activation_class(act))


def module_params(module):
    """(params_rgb, params_depth) of a module in the order of the reference restatement"""
    return tuple((se.layers[0].weight, se.layers[0].bias, se.layers[2].weight, se.layers[2].bias)
                 for se in (module.weighting_rgb, module.weighting_depth))


def load_params(module, params):
    with torch.no_grad():
        for group, mine in zip(params, module_params(module)):
            for src, dst in zip(group, mine):
                dst.copy_(src.reshape(dst.shape))
    return module


def run_module(module, x_rgb, x_depth, gy, need_maps=(True, True)):
    """-> dict y, gx_rgb, gx_depth, gW1 .. gb2 ([2, ...], None where a parameter got no gradient)"""
    xr = x_rgb.clone().requires_grad_(need_maps[0])
    xd = x_depth.clone().requires_grad_(need_maps[1])
    module.zero_grad(set_to_none=True)
    y = module({'rgb': xr, 'depth': xd})['rgb']
    if y.requires_grad:
        y.backward(gy)
    out = {'y': y.detach(), 'gx_rgb': xr.grad, 'gx_depth': xd.grad}
    groups = module_params(module)
    for i, key in enumerate(R.PARAM_GRADS):
        grads = [g[i].grad for g in groups]
        out[key] = None if any(g is None for g in grads) else torch.stack([g.reshape(g.shape[:2]) if g.ndim == 4 else g
                                                                           for g in grads])
    return out


_CASES = {}


def case(C, hw, dtype, act):
    """inputs (rounded to dtype), parameters, reference64 and chained bounds of a shape, computed once"""
    key = (C, hw, dtype, act)
    if key not in _CASES:
        i = EC.SHAPES.index((C, hw))
        x_rgb, x_depth, gy = R.make_inputs(B, C, hw, 300 + i, dtype)
        params = R.make_params(C, 400 + i)
        _CASES[key] = dict(x_rgb=x_rgb, x_depth=x_depth, gy=gy, params=params,
                           ref=R.reference64(x_rgb, x_depth, params, act, gy),
                           bounds=R.bounds(x_rgb, x_depth, params, act, gy, dtype))
    return _CASES[key]


def check(got, ref, bound, what, worst):
    r = R.worst_ratio(got, ref, bound)
    worst[what] = max(worst.get(what, 0.0), r)
    assert r <= 1.0, (what, r)


# ------------------------------------------------------------------------------ routes
@pytest.mark.parametrize('dtype', DTYPES)
def test_routes_of_the_tier_shapes(dtype):
    for hw in EC.PLANES:
        x = torch.zeros((B, 16) + hw, dtype=dtype, device=DEV)
        assert ops.sefuse_route(x, x, x) == EC.expected_route(dtype, hw), hw
        moved = Moved(x)
        assert ops.sefuse_route(x, moved.t) == EC.expected_route(dtype, hw, aligned=False), hw
    n = EC.WAVE_MAX
    assert ops.sefuse_route(torch.zeros((1, 16, 1, n), dtype=dtype, device=DEV)) & WAVE
    assert ops.sefuse_route(torch.zeros((1, 16, 1, n + 1), dtype=dtype, device=DEV)) & BLOCK
    assert EC.expected_route(dtype, EC.BLOCK_HW) & BLOCK and EC.expected_route(dtype, (30, 40)) & WAVE
    assert EC.expected_route(BF16, (15, 20)) & ELEMENT and EC.expected_route(F32, (15, 20)) & VECTOR


# ------------------------------------------------------------------------------ exact tier
def exact_inputs(C, dtype, seed):
    """integers in -8..8 on 8x16 planes; weights and gs / (H*W) from {0.25, 0.5, 1, 2}: every product, sum
    and mean is exact in float32 in any order and every map result is a multiple of 0.25 below 64, which
    bfloat16 and float16 hold"""
    gen = torch.Generator().manual_seed(seed)
    x_rgb, x_depth, gy = R.make_inputs(B, C, EC.EXACT_HW, seed, dtype, integer=True)
    pick = torch.tensor([0.25, 0.5, 1.0, 2.0])
    w = pick[torch.randint(0, 4, (2, B, C), generator=gen)]
    gs = pick[torch.randint(0, 4, (2, B, C), generator=gen)] * (EC.EXACT_HW[0] * EC.EXACT_HW[1])
    return x_rgb, x_depth, gy, w, gs


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C', EC.CHANNELS)
@pytest.mark.parametrize('moved', (False, True))
def test_exact_on_integer_inputs(dtype, C, moved):
    x_rgb, x_depth, gy, w, gs = exact_inputs(C, dtype, 11 + C)
    place = (lambda t: Moved(t, dev(t)).t) if moved else dev
    xr, xd, g = place(x_rgb), place(x_depth), place(gy)
    route = ops.sefuse_route(xr, xd, g)
    assert route == EC.expected_route(dtype, EC.EXACT_HW, aligned=not moved)
    assert torch.equal(ops.sefuse_squeeze(xr, xd).cpu(), R.squeeze64(x_rgb, x_depth).float())
    assert torch.equal(ops.sefuse_weight_grad(g, xr, xd).cpu(), R.weight_grad64(gy, x_rgb, x_depth).float())
    y_out = Moved(xr) if moved else None
    y = ops.sefuse_scale_add(xr, xd, dev(w), out=None if y_out is None else y_out.t)
    y64 = R.scale_add64(x_rgb, x_depth, w)
    assert torch.equal(y64.to(dtype).double(), y64), 'the exact tier must be representable'
    assert torch.equal(y.cpu(), y64.to(dtype))
    outs = (Moved(xr), Moved(xr)) if moved else (None, None)
    gxr, gxd = ops.sefuse_apply_backward(g, dev(w), dev(gs), out_rgb=outs[0] and outs[0].t, out_depth=outs[1] and outs[1].t)
    for got, want in zip((gxr, gxd), R.apply64(gy, w, gs)):
        assert torch.equal(want.to(dtype).double(), want), 'the exact tier must be representable'
        assert torch.equal(got.cpu(), want.to(dtype))
    if moved:
        assert y_out.untouched() and outs[0].untouched() and outs[1].untouched()


# ------------------------------------------------------------------------------ bounds tier
@pytest.mark.parametrize('C,hw', EC.SHAPES)
@pytest.mark.parametrize('dtype', DTYPES)
def test_each_kernel_within_its_bound(C, hw, dtype):
    worst = {}
    for act in EC.ACTS:
        c = case(C, hw, dtype, act)
        x_rgb, x_depth, gy, params = c['x_rgb'], c['x_depth'], c['gy'], c['params']
        xr, xd, g, P = dev(x_rgb), dev(x_depth), dev(gy), dev_params(params)
        assert ops.sefuse_route(xr, xd, g) == EC.expected_route(dtype, hw)
        s = ops.sefuse_squeeze(xr, xd)
        check(s, R.squeeze64(x_rgb, x_depth), R.squeeze_bound(x_rgb, x_depth), 's', worst)
        # every later kernel takes its inputs from the device and is held to the float64 restatement
        # of exactly these inputs
        w, z1 = ops.sefuse_excite(s, P[0], P[1], act, save_z1=True)
        assert torch.equal(ops.sefuse_excite(s, P[0], P[1], act), w)
        ex, eb = R.excite64(s, params, act), R.excite_bound(s, params, act)
        check(z1, ex['z1'], eb['z1'], 'z1', worst)
        check(w, ex['w'], eb['w'], 'w', worst)
        y = ops.sefuse_scale_add(xr, xd, w)
        check(y, R.scale_add64(x_rgb, x_depth, w), R.scale_add_bound(x_rgb, x_depth, w, dtype=dtype), 'y', worst)
        gw = ops.sefuse_weight_grad(g, xr, xd)
        check(gw, R.weight_grad64(gy, x_rgb, x_depth), R.weight_grad_bound(gy, x_rgb, x_depth), 'gw', worst)
        got = dict(zip(('gz2', 'gz1', 'gs', 'h'),
                       ops.sefuse_excite_backward(gw, w, z1, (P[0][0], P[0][2]), (P[1][0], P[1][2]), act)))
        xb, bb = R.excite_backward64(gw, w, z1, params, act), R.excite_backward_bound(gw, w, z1, params, act)
        for key in got:
            check(got[key], xb[key], bb[key], key, worst)
        gxs = ops.sefuse_apply_backward(g, w, got['gs'])
        for m, got_m, want, bnd in zip(('gx_rgb', 'gx_depth'), gxs, R.apply64(gy, w, got['gs']),
                                       R.apply_bound(gy, w, got['gs'], dtype=dtype)):
            check(got_m, want, bnd, m, worst)
    print(f'C {C} {hw} {dtype}: ' + ' '.join(f'{k} {v:.3f}' for k, v in worst.items()))


@pytest.mark.parametrize('C,hw', EC.SHAPES)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('act', EC.ACTS)
def test_module_forward_and_backward_within_bounds(C, hw, dtype, act):
    c = case(C, hw, dtype, act)
    module = load_params(build('se-add', C, act), c['params']).to(DEV)
    got = run_module(module, dev(c['x_rgb']), dev(c['x_depth']), dev(c['gy']))
    worst = {}
    for key in MODULE_KEYS:
        assert got[key] is not None, key
        check(got[key], c['ref'][key], c['bounds'][key], key, worst)
    assert got['y'].dtype == dtype and got['gx_rgb'].dtype == dtype and got['gW1'].dtype == F32
    print(f'C {C} {hw} {dtype} {act}: ' + ' '.join(f'{k} {v:.3f}' for k, v in worst.items()))


def test_half_parameters_are_cast_for_the_kernels():
    c = case(48, (15, 20), F16, 'relu')
    module = load_params(build('se-add', 48, 'relu'), c['params']).to(DEV).half()
    params = tuple(tuple(p.detach().cpu() for p in group) for group in module_params(module))     # float16-rounded
    x_rgb, x_depth, gy = c['x_rgb'], c['x_depth'], c['gy']
    got = run_module(module, dev(x_rgb), dev(x_depth), dev(gy))
    ref = R.reference64(x_rgb, x_depth, params, 'relu', gy)
    bnd = R.bounds(x_rgb, x_depth, params, 'relu', gy, F16)
    for key in ('y', 'gx_rgb', 'gx_depth'):
        assert R.worst_ratio(got[key], ref[key], bnd[key]) <= 1.0, key
    assert got['gW1'].dtype == F16 and got['gb2'].dtype == F16


# ------------------------------------------------------------------------------ golden tier
@pytest.fixture(scope='module')
def golden():
    return EC.GoldenFile(GOLDEN)


@pytest.mark.parametrize('name,act,k', EC.golden_records())
def test_module_against_the_recorded_reference(golden, name, act, k):
    rec = golden.record(EC.record_name(name, act, k))
    C = EC.GOLDEN_SHAPES[k][1]
    se, dest = EC.EXPECTED[name]
    module = build(name, C, act)
    module.load_state_dict(golden.state_dict(rec), strict=True)
    module.to(DEV)
    x = {m: dev(rec[f'x_{m}']).requires_grad_(True) for m in ('rgb', 'depth')}
    y = module(x)
    for m in ('rgb', 'depth'):
        assert (y[m] is x[m]) == (m not in dest), m
    assert (y['rgb'] is y['depth']) == (len(dest) == 2)
    ((y['rgb'] * dev(rec['gy_rgb'])).sum() + (y['depth'] * dev(rec['gy_depth'])).sum()).backward()
    if not se:
        for m in ('rgb', 'depth'):
            assert torch.equal(y[m].detach().cpu(), rec[f'y_{m}']) and torch.equal(x[m].grad.cpu(), rec[f'gx_{m}']), m
        return
    # the upstream gradient of the fused map: that of every key that holds it
    gy = sum(rec[f'gy_{m}'] for m in dest)
    params = tuple(tuple(rec[f'state/weighting_{m}.layers.{i}.{p}'] for i, p in ((0, 'weight'), (0, 'bias'),
                                                                                (2, 'weight'), (2, 'bias')))
                   for m in ('rgb', 'depth'))
    bnd = R.bounds(rec['x_rgb'], rec['x_depth'], params, act, gy)
    worst = {}
    for m in dest:
        check(y[m].detach(), rec[f'y_{m}'].double(), bnd['y'], 'y', worst)
    for m in ('rgb', 'depth'):
        # one more rounding where autograd adds the handed-through gradient
        extra = R.U * rec[f'gx_{m}'].double().abs() * (m not in dest)
        check(x[m].grad, rec[f'gx_{m}'].double(), bnd[f'gx_{m}'] + extra, f'gx_{m}', worst)
    for i, m in enumerate(('rgb', 'depth')):
        for key, layer, p in (('gW1', 0, 'weight'), ('gb1', 0, 'bias'), ('gW2', 2, 'weight'), ('gb2', 2, 'bias')):
            got = getattr(getattr(module, f'weighting_{m}').layers[layer], p).grad
            want = rec[f'grad/weighting_{m}.layers.{layer}.{p}'].double()
            check(got, want.reshape(bnd[key][i].shape), bnd[key][i], key, worst)
    print(f'{name} {act} {k}: ' + ' '.join(f'{key} {v:.3f}' for key, v in worst.items()))


# ------------------------------------------------------------------------------ routes and alignment
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('hw', ((8, 16), (15, 20), EC.BLOCK_HW))
def test_off_16_byte_tensors_give_the_same_bits_and_touch_nothing_else(dtype, hw):
    C = 48
    c = case(C, hw, dtype, 'silu')
    xr, xd, g = dev(c['x_rgb']), dev(c['x_depth']), dev(c['gy'])
    P = dev_params(c['params'])
    s = ops.sefuse_squeeze(xr, xd)
    w = ops.sefuse_excite(s, P[0], P[1], 'silu')
    gs = dev(c['ref']['gs'].float())
    base = (s, ops.sefuse_scale_add(xr, xd, w), ops.sefuse_weight_grad(g, xr, xd)) + ops.sefuse_apply_backward(g, w, gs)
    mxr, mxd, mg = Moved(xr, xr), Moved(xd, xd), Moved(g, g)
    assert ops.sefuse_route(mxr.t, mxd.t, mg.t) & ELEMENT
    outs = [Moved(s), Moved(xr), Moved(s), Moved(xr), Moved(xr)]
    ops.sefuse_squeeze(mxr.t, mxd.t, out=outs[0].t)
    ops.sefuse_scale_add(mxr.t, mxd.t, w, out=outs[1].t)
    ops.sefuse_weight_grad(mg.t, mxr.t, mxd.t, out=outs[2].t)
    ops.sefuse_apply_backward(mg.t, w, gs, out_rgb=outs[3].t, out_depth=outs[4].t)
    for i, (a, b) in enumerate(zip(base, outs)):
        assert torch.equal(a, b.t), i
        assert b.untouched(), i
    # one tensor off 16 bytes is enough for the element route, and the inputs are left as they were
    assert torch.equal(ops.sefuse_scale_add(xr, mxd.t, w), base[1]) and torch.equal(ops.sefuse_squeeze(mxr.t, xd), s)
    assert mxr.untouched() and mxd.untouched() and mg.untouched() and torch.equal(mxr.t, xr)


# ------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize('dtype', (F32, BF16))
@pytest.mark.parametrize('hw', ((15, 20), EC.BLOCK_HW))
def test_same_bits_on_every_call_stream_and_graph_replay(dtype, hw):
    c = case(48, hw, dtype, 'relu')
    xr, xd, g = dev(c['x_rgb']), dev(c['x_depth']), dev(c['gy'])
    P = dev_params(c['params'])

    def call():
        s = ops.sefuse_squeeze(xr, xd)
        w, z1 = ops.sefuse_excite(s, P[0], P[1], 'relu', save_z1=True)
        y = ops.sefuse_scale_add(xr, xd, w)
        gw = ops.sefuse_weight_grad(g, xr, xd)
        back = ops.sefuse_excite_backward(gw, w, z1, (P[0][0], P[0][2]), (P[1][0], P[1][2]), 'relu')
        return (s, w, z1, y, gw) + back + ops.sefuse_apply_backward(g, w, back[2])

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
    graph = torch.cuda.CUDAGraph()              # one chain: every call is enqueued on the capturing stream
    warm = torch.cuda.Stream(DEV)
    warm.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(warm):
        call()
    torch.cuda.current_stream(DEV).wait_stream(warm)
    with torch.cuda.graph(graph):
        captured = call()
    for _ in range(3):
        for t in captured:
            t.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(first, captured):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------ gradient subsets
def test_gradient_subsets_skip_the_rest_and_keep_the_bits(monkeypatch):
    c = case(48, (15, 20), BF16, 'silu')
    module = load_params(build('se-add', 48, 'silu'), c['params']).to(DEV)
    xr, xd, g = dev(c['x_rgb']), dev(c['x_depth']), dev(c['gy'])
    full = run_module(module, xr, xd, g)
    calls = []
    for name in ('sefuse_weight_grad', 'sefuse_excite_backward', 'sefuse_apply_backward'):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _r=real, **k: calls.append((_n, a, k)) or _r(*a, **k))

    def same(got, keys):
        for key in MODULE_KEYS[1:]:
            if key in keys:
                assert torch.equal(got[key], full[key]), key
            else:
                assert got[key] is None, key
        assert torch.equal(got['y'], full['y'])

    # the maps alone (frozen parameters)
    module.requires_grad_(False)
    same(run_module(module, xr, xd, g), ('gx_rgb', 'gx_depth'))
    # the parameters alone (a frozen encoder): no map pass
    module.requires_grad_(True)
    calls.clear()
    same(run_module(module, xr, xd, g, need_maps=(False, False)), R.PARAM_GRADS)
    assert [n for n, a, k in calls] == ['sefuse_weight_grad', 'sefuse_excite_backward', 'sefuse_apply_backward']
    assert calls[2][1][3:5] == (False, False)
    # one modality: the other is left out of all three kernels
    module.requires_grad_(False)
    calls.clear()
    got = run_module(module, xr, xd, g, need_maps=(False, True))
    same(got, ('gx_depth',))
    (_, wg, _), (_, eb, _), (_, ap, _) = calls
    assert wg[1] is None and wg[2] is not None and eb[3] is None and eb[4] is not None and ap[3:5] == (False, True)
    module.weighting_rgb.requires_grad_(True)
    calls.clear()
    got = run_module(module, xr, xd, g, need_maps=(False, False))
    for key in R.PARAM_GRADS:
        assert got[key] is None                         # run_module reports a gradient only with both halves
    for i, p in enumerate(module_params(module)[0]):
        assert torch.equal(p.grad.reshape(full[R.PARAM_GRADS[i]][0].shape), full[R.PARAM_GRADS[i]][0]), i
    assert all(p.grad is None for p in module_params(module)[1])
    (_, wg, _), (_, eb, _), (_, ap, _) = calls
    assert wg[1] is not None and wg[2] is None and eb[3] is not None and eb[4] is None and ap[3:5] == (False, False)


def test_nothing_is_saved_when_nothing_needs_a_gradient(monkeypatch):
    c = case(48, (3, 5), F32, 'relu')
    module = load_params(build('se-add', 48, 'relu'), c['params']).to(DEV)
    seen = []
    real = ops.sefuse_excite
    monkeypatch.setattr(ops, 'sefuse_excite', lambda *a, **k: seen.append(k.get('save_z1', False)) or real(*a, **k))
    x = {'rgb': dev(c['x_rgb']), 'depth': dev(c['x_depth'])}
    with torch.no_grad():
        y = module(x)['rgb']
    assert y.grad_fn is None and seen == [False]
    module.requires_grad_(False)
    y2 = module(x)['rgb']
    assert y2.grad_fn is None and seen == [False, False] and torch.equal(y, y2)
    module.requires_grad_(True)
    y3 = module(x)['rgb']
    assert y3.grad_fn is not None and seen == [False, False, True] and torch.equal(y, y3)


# ------------------------------------------------------------------------------ fallbacks
def forbid_the_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError('the library must not be called on this path')
    for name in ('sefuse_squeeze', 'sefuse_excite', 'sefuse_scale_add', 'sefuse_weight_grad',
                 'sefuse_excite_backward', 'sefuse_apply_backward'):
        monkeypatch.setattr(ops, name, refuse)


@pytest.mark.parametrize('act', EC.ACTS)
def test_fallbacks_on_the_device_are_the_torch_formulation(monkeypatch, act):
    C, hw = 48, (15, 20)
    c = case(C, hw, F32, act)
    xr, xd = dev(c['x_rgb']), dev(c['x_depth'])
    P = dev_params(c['params'])
    fused = load_params(build('se-add', C, act), c['params']).to(DEV)({'rgb': xr, 'depth': xd})['rgb']
    assert R.worst_ratio(fused, c['ref']['y'], c['bounds']['y']) <= 1.0
    forbid_the_library(monkeypatch)
    # NHWC (the Swin encoders): the formulation on the permuted views the module makes
    nhwc = load_params(build('se-add', C, act, 'nhwc'), c['params']).to(DEV)
    hr, hd = xr.permute(0, 2, 3, 1).contiguous(), xd.permute(0, 2, 3, 1).contiguous()
    y = nhwc({'rgb': hr, 'depth': hd})['rgb']
    assert y.shape == (B,) + hw + (C,)
    assert torch.equal(y.permute(0, 3, 1, 2), R.torch_formulation(hr.permute(0, 3, 1, 2), hd.permute(0, 3, 1, 2), P, act))
    # a non-dense view
    module = load_params(build('se-add', C, act), c['params']).to(DEV)
    wide = torch.zeros((B, C, hw[0], hw[1] + 3), device=DEV)
    wide[..., :hw[1]] = xr
    view = wide[..., :hw[1]]
    assert not view.is_contiguous()
    assert torch.equal(module({'rgb': view, 'depth': xd})['rgb'], R.torch_formulation(view, xd, P, act))
    # mixed dtypes: the depth branch in float16
    module.weighting_depth.half()
    P16 = (P[0], tuple(p.half() for p in P[1]))
    y = module({'rgb': xr, 'depth': xd.half()})['rgb']
    assert y.dtype == F32 and torch.equal(y, R.torch_formulation(xr, xd.half(), P16, act))
    # another activation module
    other = model.get_encoder_fusion_class('se-add')(n_channels_in=C, input_memory_layout='nchw', activation=torch.nn.GELU)
    other.to(DEV)({'rgb': xr, 'depth': xd})


def test_plain_add_names_never_touch_the_library(monkeypatch):
    forbid_the_library(monkeypatch)
    monkeypatch.setattr(L, 'lib', lambda: (_ for _ in ()).throw(AssertionError('the library must not be loaded')))
    x = {'rgb': torch.randn((B, 32, 4, 5), device=DEV), 'depth': torch.randn((B, 32, 4, 5), device=DEV)}
    for name in ('add', 'add-uni-rgb', 'add-uni-depth', 'none'):
        y = build(name, 32, 'relu').to(DEV)(x)
        for m in ('rgb', 'depth'):
            assert torch.equal(y[m], x['rgb'] + x['depth'] if m in EC.EXPECTED[name][1] else x[m]), (name, m)
    enc_dec = model.get_encoder_decoder_fusion_class('add-rgb')(n_channels_encoder=32, n_channels_decoder=32)
    assert torch.equal(enc_dec(x, x['depth']), x['rgb'] + x['depth'])


# ------------------------------------------------------------------------------ autocast
@pytest.mark.parametrize('dtype,cast', ((F32, F16), (F32, BF16), (F16, F16), (BF16, BF16)))
def test_autocast_keeps_the_dtype_of_the_torch_formulation(monkeypatch, dtype, cast):
    C, hw = 48, (15, 20)
    c = case(C, hw, dtype, 'relu')
    xr, xd, g = dev(c['x_rgb']), dev(c['x_depth']), dev(c['gy'])
    module = load_params(build('se-add', C, 'relu'), c['params']).to(DEV)
    calls = []
    real = ops.sefuse_scale_add
    monkeypatch.setattr(ops, 'sefuse_scale_add', lambda *a, **k: calls.append(1) or real(*a, **k))
    with torch.autocast('cuda', dtype=cast):
        want = R.torch_formulation(xr, xd, dev_params(c['params']), 'relu')
        got = run_module(module, xr, xd, g)
    assert want.dtype == dtype and got['y'].dtype == want.dtype and len(calls) == 1
    for key in MODULE_KEYS:
        assert R.worst_ratio(got[key], c['ref'][key], c['bounds'][key]) <= 1.0, key
    # a half input that the torch formulation would promote takes the torch formulation
    if dtype == BF16:
        calls.clear()
        with torch.autocast('cuda', dtype=F16):
            want = R.torch_formulation(xr, xd, dev_params(c['params']), 'relu')
            y = module({'rgb': xr, 'depth': xd})['rgb']
        assert want.dtype == F32 and y.dtype == F32 and not calls and torch.equal(y, want)
