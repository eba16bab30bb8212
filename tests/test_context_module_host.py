"""CPU tier of the context module: the names, bins and the factory, the state dicts, `NoContextModule`
and the APPM pool sizes against the reference's recorded results, a `load_state_dict` round trip, the
refusal of CPU tensors, the fixture's input digests, and the two conditions the error bounds of
`testing.context_ref` must meet: torch's own float32 CPU result stays inside them on every input the
GPU tier uses, and three defective restatements (window ends by floor, bilinear without the
half-pixel offset, nearest by rounding) do not."""
import numpy as np
import pytest
import torch

from nicr_mt_scene_analysis_amd import _lib as L
from nicr_mt_scene_analysis_amd import model
from nicr_mt_scene_analysis_amd import ops
from nicr_mt_scene_analysis_amd import types as T
from nicr_mt_scene_analysis_amd.model import context_module as cm
from nicr_mt_scene_analysis_amd.testing import context_cases as cc
from nicr_mt_scene_analysis_amd.testing import context_ref as R

import _golden

NAMES = ('ppm', 'ppm-1-5', 'ppm-1-5-10', 'ppm-1-2-4-8', 'appm', 'appm-1-5', 'appm-1-5-10', 'appm-1-2-4-8', 'none')


@pytest.fixture(scope='module')
def golden():
    return _golden.load('context_module')


def build(case):
    """the module of a case with the case's state, in eval mode, and its inputs"""
    name, n_in, n_out, _, input_size, upsampling, _ = cc.CONTEXT_CASES[case] if isinstance(case, str) else case
    module = cm.get_context_module(name, n_in, n_out, input_size, upsampling=upsampling)
    inp = cc.make_context_inputs(case)
    missing, unexpected = module.load_state_dict({k: torch.from_numpy(v) for k, v in inp['state'].items()},
                                                 strict=False)
    assert not unexpected and all(k.endswith('num_batches_tracked') for k in missing)
    return module.eval(), inp


def test_names_bins_factory_and_exports(golden):
    assert len(NAMES) == 9 and cm.KNOWN_CONTEXT_MODULES == NAMES
    assert _golden.jload(golden['known']) == list(NAMES)
    for attr in ('KNOWN_CONTEXT_MODULES', 'PyramidPoolingModule', 'AdaptivePyramidPoolingModule', 'NoContextModule',
                 'ContextModuleType', 'get_context_module'):
        assert getattr(model, attr) is getattr(cm, attr), attr
    for attr in ('ContextModuleInputType', 'ContextModuleContextFeaturesType', 'ContextModuleOutputType'):
        assert hasattr(T, attr), attr
    bins = _golden.jload(golden['bins'])
    for name in NAMES:
        m = cm.get_context_module(name.upper(), 8, 6, (15, 20))
        want = (cm.NoContextModule if name == 'none' else
                cm.AdaptivePyramidPoolingModule if name.startswith('appm') else cm.PyramidPoolingModule)
        assert type(m) is want, name
        assert list(cc.NAME_BINS[name]) == bins[name], name
        if name != 'none':
            assert list(m._bins) == bins[name] and m.n_channels_reduction == 8 // len(bins[name])
            first = [type(f[0]) for f in m.features]
            assert first == [torch.nn.Identity if name.startswith('appm') else torch.nn.AdaptiveAvgPool2d] * len(first)
            if not name.startswith('appm'):
                assert [f[0].output_size for f in m.features] == bins[name]
    assert cm.get_context_module('none', 8, 6, (1, 1)).n_channels_reduction == 6
    for bad in ('ppm-1', 'ppm-1-2-3-6', 'pyramid', ''):
        with pytest.raises(ValueError):
            cm.get_context_module(bad, 8, 6, (15, 20))
    # the classes' own defaults, as in the reference
    for m in (cm.PyramidPoolingModule(8, 6), cm.AdaptivePyramidPoolingModule(8, 6, (15, 20))):
        assert m._bins == (1, 2, 3, 6) and m._upsampling == 'bilinear' and m.n_channels_reduction == 2
    with pytest.raises(ValueError):
        cm.PyramidPoolingModule(10, 6, bins=(1, 2, 3, 4, 5))            # more than NMSA_PPM_MAX_BINS


@pytest.mark.parametrize('name', NAMES)
def test_state_dict_keys_and_shapes(golden, name):
    recorded = _golden.jload(golden['state'])[name]
    n_in, n_out, input_size = cc.CONTEXT_STATE_PROBE
    m = cm.get_context_module(name, n_in, n_out, input_size)
    got = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert got == recorded and list(got) == list(recorded)
    mine = [k for k in got if not k.endswith('num_batches_tracked')]
    assert mine == list(cc.context_param_shapes(name, n_in, n_out))


@pytest.mark.parametrize('name', ('ppm-1-5-10', 'appm-1-2-4-8', 'none'))
def test_load_state_dict_round_trip(name):
    a = cm.get_context_module(name, 8, 6, (15, 20))
    b = cm.get_context_module(name, 8, 6, (15, 20))
    with torch.no_grad():
        for p in a.parameters():
            p.normal_()
    b.load_state_dict(a.state_dict())                       # strict
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)
    # PPM and APPM checkpoints are interchangeable (index 0 of a branch has no parameters)
    if name != 'none':
        other = cm.get_context_module(name[1:] if name.startswith('appm') else 'a' + name, 8, 6, (15, 20))
        other.load_state_dict(a.state_dict())


def test_no_context_module_against_the_fixture(golden):
    module, inp = build('none_4_6')
    x = torch.from_numpy(inp['x']).requires_grad_(True)
    y, feats = module(x)
    assert feats == ()
    y.backward(torch.from_numpy(inp['gy']))
    # the same torch ops on the same machine class: a few ulps of slack for another BLAS / thread count
    np.testing.assert_allclose(y.detach().numpy(), golden['none_4_6__out'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(x.grad.numpy(), golden['none_4_6__gx'], rtol=1e-5, atol=1e-6)
    same = cm.get_context_module('none', 4, 4, (3, 4))
    assert isinstance(same.layer, torch.nn.Identity) and same(x)[0] is x


def test_appm_pool_sizes_against_the_fixture(golden):
    m = cm.get_context_module('appm-1-5', 4, 4, (15, 20))
    for h, w, sizes in _golden.jload(golden['appm']):
        assert [list(s) for s in m.pool_sizes(h, w)] == sizes, (h, w)
    for case, (name, *_rest) in cc.CONTEXT_CASES.items():
        if name == 'none':
            continue
        p = _golden.jload(golden[f'{case}__params'])
        module, _ = build(case)
        H, W = p['shape'][1:]
        sizes = module.pool_sizes(H, W) if name.startswith('appm') else ops._ppm_sizes(module._bins)
        assert [list(s) for s in sizes] == p['sizes'], case


def test_cpu_tensors_are_refused():
    for name in ('ppm', 'appm-1-2-4-8'):
        m = cm.get_context_module(name, 8, 6, (3, 4))
        with pytest.raises(L.NmsaError):
            m(torch.zeros(2, 8, 3, 4))
    x = torch.zeros(1, 2, 3, 4)
    with pytest.raises(L.NmsaError):
        ops.ppm_pool(x, (1, 2))
    with pytest.raises(L.NmsaError):
        ops.ppm_pool_backward((torch.zeros(1, 2, 1, 1),), (1, 2, 3, 4), (1,))
    with pytest.raises(L.NmsaError):
        ops.ppm_upsample_concat(x, (torch.zeros(1, 1, 2, 2),), 'nearest')
    with pytest.raises(L.NmsaError):
        ops.ppm_upsample_concat_backward(torch.zeros(1, 3, 3, 4), 2, ((1, 1, 2, 2),), 'nearest')
    assert ops.ppm_route((32, 64), (1, 2, (16, 16))) == L.NMSA_PPM_ROUTE_LDS          # host only
    assert ops.ppm_route((33, 64), (1,)) == L.NMSA_PPM_ROUTE_GLOBAL
    for (hw, sizes, lds) in cc.ROUTE_CASES:
        assert ops.ppm_route(hw, sizes) == (L.NMSA_PPM_ROUTE_LDS if lds else L.NMSA_PPM_ROUTE_GLOBAL), (hw, sizes)
    with pytest.raises(ValueError):
        ops.ppm_route((8, 8), (1, 2, 3, 4, 5))
    with pytest.raises(ValueError):
        ops.ppm_route((8, 8), (0,))


def test_fixture_digests_match_the_regenerated_cases(golden):
    assert _golden.jload(golden['names']) == list(cc.CONTEXT_CASES)
    for case, (name, n_in, n_out, shape, input_size, upsampling, _) in cc.CONTEXT_CASES.items():
        p = _golden.jload(golden[f'{case}__params'])
        inp = cc.make_context_inputs(case)
        assert p['digest'] == cc.context_input_digest(inp), case
        assert (p['name'], p['n_in'], p['n_out'], tuple(p['shape']), tuple(p['input_size']), p['upsampling']) == \
            (name, n_in, n_out, shape, input_size, upsampling)
        assert golden[f'{case}__out'].shape == (shape[0], n_out) + tuple(shape[1:])
        assert golden[f'{case}__out'].dtype == np.float32
        assert p['n_features'] == len(cc.NAME_BINS[name])
    train = _golden.jload(golden['train'])
    name, n_in, n_out, (B, H, W), *_ = cc.CONTEXT_TRAIN_CASE
    assert train['out'] == [B, n_out, H, W]
    assert train['features'] == [[B, n_in // 2, b, b] for b in cc.NAME_BINS[name]]


def test_reference64_agrees_with_torch_float64():
    x, ys, g_out, gps = R.make_inputs(2, 3, 2, (7, 9), ((1, 1), (5, 5), (9, 11)), seed=3)
    for mode in ('nearest', 'bilinear'):
        x64 = x.double().requires_grad_(True)
        pooled = R.torch_pool(x64, ((1, 1), (5, 5), (9, 11)))
        torch.autograd.backward(pooled, [g.double() for g in gps])
        y64 = [y.double().requires_grad_(True) for y in ys]
        cat = R.torch_upcat(x.double(), y64, mode)
        cat.backward(g_out.double())
        ref = R.reference64(x, ((1, 1), (5, 5), (9, 11)), ys, mode, g_out, gps)
        # torch's float64 resize takes float64 weights, the reference ATen's float32 ones: a source
        # coordinate below 11 is off by at most 2^-21, times the difference of two N(0, 1) neighbours
        tol = dict(rtol=0, atol=1e-5)
        for got, want in zip(pooled, ref['pooled']):
            np.testing.assert_allclose(got.detach().numpy(), want.numpy(), rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(x64.grad.numpy(), ref['gx_pool'].numpy(), rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(cat.detach().numpy(), ref['cat'].numpy(), **tol)
        for y, want in zip(y64, ref['gys']):
            np.testing.assert_allclose(y.grad.numpy(), want.numpy(), **tol)


def gpu_tier_geometries():
    """every (hw, sizes) of the GPU tier's bound and exact tests"""
    for hw in cc.GPU_HW:
        for bins in cc.GPU_BINS:
            yield hw, cc.sizes_of(bins)
    yield cc.APPM_HW, tuple((2 * b, 2 * b) for b in cc.APPM_BINS)
    for hw, sizes, _ in cc.ROUTE_CASES:
        yield hw, sizes


GEOMETRIES = list(gpu_tier_geometries())


def test_torch_float32_meets_the_bounds_and_the_defects_do_not():
    """(a) torch's float32 CPU pools, resizes and their autograd stay inside `bounds` on every geometry of
    the GPU tier (C = 3, the tier's seeds); (b) each of the three defective restatements, evaluated in
    float64 (so that nothing but the defect is wrong), leaves them on at least one of those inputs"""
    missed = {'floor': 0.0, 'no_half_pixel': 0.0, 'round': 0.0}
    for k, (hw, sizes) in enumerate(GEOMETRIES):
        x, ys, g_out, gps = R.make_inputs(2, 3, 2, hw, sizes, seed=k)
        for mode in ('nearest', 'bilinear'):
            ref, bd = R.reference64(x, sizes, ys, mode, g_out, gps), R.bounds(x, sizes, ys, mode, g_out, gps)
            xr = x.clone().requires_grad_(True)
            pooled = R.torch_pool(xr, sizes)
            torch.autograd.backward(pooled, gps)
            yr = [y.clone().requires_grad_(True) for y in ys]
            cat = R.torch_upcat(x, yr, mode)
            cat.backward(g_out)
            tag = (hw, sizes, mode)
            for i in range(len(sizes)):
                assert R.worst_ratio(pooled[i], ref['pooled'][i], bd['pooled'][i]) <= 1.0, tag
                assert R.worst_ratio(yr[i].grad, ref['gys'][i], bd['gys'][i]) <= 1.0, tag
            assert R.worst_ratio(cat, ref['cat'], bd['cat']) <= 1.0, tag
            assert R.worst_ratio(xr.grad, ref['gx_pool'], bd['gx_pool']) <= 1.0, tag
            assert torch.equal(cat[:, :3], x)
            defect = 'round' if mode == 'nearest' else 'no_half_pixel'
            missed[defect] = max(missed[defect], R.worst_ratio(R.upcat64(x, ys, mode, defect), ref['cat'], bd['cat']))
        for got, want, b in zip(R.pool64(x, sizes, end='floor'), ref['pooled'], bd['pooled']):
            missed['floor'] = max(missed['floor'], R.worst_ratio(got, want, b))
    for defect, worst in missed.items():
        assert worst > 1000.0, (defect, worst)          # not a rounding matter: another pixel was read


def test_the_exact_tier_is_exact_in_float32_on_the_cpu():
    """integer inputs in -8..8 on power-of-two geometries: torch's float32 equals the float64 reference"""
    sizes = cc.sizes_of(cc.EXACT_BINS)
    for hw in cc.EXACT_HW:
        assert R.is_power_of_two_geometry(hw, sizes)
        for mode in ('nearest', 'bilinear'):
            x, ys, g_out, gps = R.make_inputs(2, 3, 2, hw, sizes, seed=7, integer=True)
            ref = R.reference64(x, sizes, ys, mode, g_out, gps)
            xr = x.clone().requires_grad_(True)
            pooled = R.torch_pool(xr, sizes)
            torch.autograd.backward(pooled, gps)
            yr = [y.clone().requires_grad_(True) for y in ys]
            cat = R.torch_upcat(x, yr, mode)
            cat.backward(g_out)
            assert all(torch.equal(p.double(), r) for p, r in zip(pooled, ref['pooled']))
            assert torch.equal(cat.double(), ref['cat']) and torch.equal(xr.grad.double(), ref['gx_pool'])
            assert all(torch.equal(y.grad.double(), r) for y, r in zip(yr, ref['gys']))
    assert not R.is_power_of_two_geometry((15, 20), cc.sizes_of((1, 5)))


# ------------------------------------------------------------------------------ non-finite values
from nicr_mt_scene_analysis_amd.testing import nonfinite as NF      # noqa: E402


@pytest.mark.parametrize('case', NF.ppm_cases(), ids=repr)
def test_nonfinite_cases_show_the_poison_and_contain_it_in_the_composition(case):
    """the condition that keeps tests/test_nonfinite_model.py honest, on the composition alone: in every poisoned
    run an output element is touched and one is not, and a NaN and a +inf leave a non-finite output"""
    for dtype in NF.DTYPES:
        assert NF.run(case, dtype) > 0
