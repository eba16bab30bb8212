"""CPU tier of the learned upsampling: the bound symbols, the route rule and the workspace query
without a device (made-up addresses, never dereferenced), the module's construction and its plain
`interpolate` modes, and the fixture's input digest."""
import ctypes
import itertools

import numpy as np
import pytest
import torch
from torch.nn.functional import interpolate

from nicr_mt_scene_analysis_amd import _lib as L
from nicr_mt_scene_analysis_amd import model
from nicr_mt_scene_analysis_amd.model import upsampling as up
from nicr_mt_scene_analysis_amd.testing import synthetic as syn

import _golden

SYMBOLS = ('nmsa_upsample2x_dw3x3_fwd', 'nmsa_upsample2x_dw3x3_bwd_workspace_bytes',
           'nmsa_upsample2x_dw3x3_bwd', 'nmsa_upsample2x_dw3x3_route')
VECTOR, PIXEL, ARG = L.NMSA_UP_ROUTE_VECTOR, L.NMSA_UP_ROUTE_PIXEL, -1
X, Y = 0x100000, 0x200000


def route(x=X, y=Y, dtype=L.NMSA_F32, B=2, C=3, h=5, w=8):
    return L.lib().nmsa_upsample2x_dw3x3_route(ctypes.c_void_p(x) if x else None, ctypes.c_void_p(y) if y else None,
                                               dtype, B, C, h, w)


def test_symbols_are_declared_and_bound():
    handle = ctypes.CDLL(L.LIB_PATH)
    for s in SYMBOLS:
        assert s in L.declared_symbols() and s in L._SIGNATURES and hasattr(handle, s), s
    assert [len(L._SIGNATURES[s][1]) for s in SYMBOLS] == [11, 4, 15, 7]


def test_route_by_width_and_dtype():
    # f32: a lane run of 2 pixels; half: of 4
    for w in range(1, 18):
        assert route(w=w) == (VECTOR if w % 2 == 0 else PIXEL), w
        for half in (L.NMSA_BF16, L.NMSA_F16):
            assert route(w=w, dtype=half) == (VECTOR if w % 4 == 0 else PIXEL), w


def test_route_by_alignment():
    for dtype, e in ((L.NMSA_F32, 4), (L.NMSA_BF16, 2), (L.NMSA_F16, 2)):
        for off in range(e, 16, e):                       # element-aligned, off 16 bytes
            assert route(dtype=dtype, y=Y + off) == PIXEL and route(dtype=dtype, x=X + off) == PIXEL
        assert route(dtype=dtype, x=X + 16, y=Y + 32) == VECTOR


def test_route_refuses_bad_arguments():
    assert route(x=0) == ARG and route(y=0) == ARG and route(dtype=3) == ARG and route(dtype=-1) == ARG
    for name in ('B', 'C', 'h', 'w'):
        assert route(**{name: 0}) == ARG and route(**{name: -2}) == ARG
    assert route(x=X + 1) == ARG and route(y=Y + 2) == ARG and route(dtype=L.NMSA_F16, y=Y + 1) == ARG


def test_workspace_bytes_is_positive_and_monotone():
    q = L.lib().nmsa_upsample2x_dw3x3_bwd_workspace_bytes
    base = (2, 3, 5, 6)
    assert q(*base) > 0 and q(1, 1, 1, 1) > 0
    for axis, factor in itertools.product(range(4), (2, 7, 64)):
        grown = tuple(n * factor if i == axis else n for i, n in enumerate(base))
        assert q(*grown) >= q(*base), (axis, factor)
    sizes = [q(1, 1, n, n) for n in (1, 8, 9, 64, 65, 512, 513)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert q(32, 40, 240, 320) > q(32, 40, 120, 160) > q(1, 40, 120, 160)


@pytest.mark.parametrize('mode', ('learned-3x3', 'learned-3x3-zeropad'))
@pytest.mark.parametrize('use_bias', (True, False))
def test_learned_module_construction(mode, use_bias):
    m = up.Upsampling(mode, n_channels=5, use_bias=use_bias)
    sd = m.state_dict()
    assert list(sd) == (['conv.weight', 'conv.bias'] if use_bias else ['conv.weight'])
    assert tuple(sd['conv.weight'].shape) == (5, 1, 3, 3) and sd['conv.weight'].dtype == torch.float32
    assert isinstance(m.conv, torch.nn.Conv2d) and m.conv.groups == 5
    stencil = torch.tensor([[1., 2., 1.], [2., 4., 2.], [1., 2., 1.]]) / 16.
    assert torch.equal(sd['conv.weight'], stencil.expand(5, 1, 3, 3))             # bit-equal: exact in f32
    if use_bias:
        assert tuple(sd['conv.bias'].shape) == (5,) and torch.equal(sd['conv.bias'], torch.zeros(5))
    assert all(p.requires_grad for p in m.parameters())
    recorded = _golden.jload(_golden.load('upsampling')['state'])[mode]
    assert {k: list(v.shape) for k, v in up.Upsampling(mode, n_channels=4).state_dict().items()} == recorded


def test_scale_factor_check():
    for mode in ('learned-3x3', 'learned-3x3-zeropad'):
        for bad in (3., 1., (2., 3.), 4):
            with pytest.raises(ValueError):
                up.Upsampling(mode, n_channels=2, scale_factor=bad)
        up.Upsampling(mode, n_channels=2, scale_factor=(2., 2.))
        up.Upsampling(mode, n_channels=2, scale_factor=2)
    up.Upsampling('bilinear', n_channels=2, scale_factor=3.)                      # the plain modes take any


def test_factory_and_exports():
    assert model.Upsampling is up.Upsampling and model.UpsamplingType is up.Upsampling
    assert model.get_upsampling_class is up.get_upsampling_class
    assert model.KNOWN_UPSAMPLING_METHODS == ('nearest', 'bilinear', 'learned-3x3', 'learned-3x3-zeropad')
    m = up.get_upsampling_class(None)(n_channels=3)
    assert isinstance(m, up.Upsampling) and m._mode == 'bilinear' and not list(m.parameters())
    assert up.get_upsampling_class('Learned-3x3', use_bias=False)(n_channels=3).conv.bias is None
    with pytest.raises(ValueError):
        up.get_upsampling_class('bicubic')
    with pytest.raises(ValueError):
        up.Upsampling('bicubic', n_channels=3)


def test_plain_modes_equal_interpolate_on_cpu():
    x = torch.randn(2, 3, 5, 7, generator=torch.Generator().manual_seed(3))
    assert torch.equal(up.Upsampling('nearest', 3)(x), interpolate(x, scale_factor=2., mode='nearest'))
    assert torch.equal(up.Upsampling('bilinear', 3)(x),
                       interpolate(x, scale_factor=2., mode='bilinear', align_corners=False))
    assert torch.equal(up.Upsampling('nearest', 3, scale_factor=3.)(x), interpolate(x, scale_factor=3., mode='nearest'))
    shapes = _golden.jload(_golden.load('upsampling')['shapes'])
    probe = torch.zeros(syn.UPSAMPLING_SHAPE_INPUT)
    for mode in ('nearest', 'bilinear'):
        assert list(up.Upsampling(mode, probe.shape[1])(probe).shape) == shapes[mode]
    for mode in ('learned-3x3', 'learned-3x3-zeropad'):                            # x2 of the probe
        assert shapes[mode] == [probe.shape[0], probe.shape[1], 2 * probe.shape[2], 2 * probe.shape[3]]


@pytest.mark.parametrize('mode', ('learned-3x3', 'learned-3x3-zeropad'))
def test_learned_mode_on_a_cpu_tensor_raises(mode):
    with pytest.raises(L.NmsaError):
        up.Upsampling(mode, n_channels=3)(torch.zeros(1, 3, 4, 4))


@pytest.mark.parametrize('zeropad', (False, True))
def test_the_two_float64_formulations_of_the_oracle_agree(zeropad):
    """the GPU tier's oracle is the reference's ops (interpolate, pad, depthwise conv2d) in float64;
    at 70001 channels it uses the unfold form of the same sum: equal on integer-grid inputs, where
    every order of summation is exact"""
    from nicr_mt_scene_analysis_amd.testing import upsampling_ref as R
    gen = torch.Generator().manual_seed(11)
    for B, C, h, w in ((2, 3, 1, 1), (1, 2, 1, 2), (2, 3, 3, 5), (1, 4, 9, 2)):
        x = torch.randint(-8, 9, (B, C, h, w), generator=gen).float()
        wt = torch.randint(-8, 9, (C, 1, 3, 3), generator=gen).float() / 16
        b = torch.randint(-8, 9, (C,), generator=gen).float() / 16
        gy = torch.randint(-8, 9, (B, C, 2 * h, 2 * w), generator=gen).float()
        for bias in (b, None):
            got = R.reference64(x, wt, bias, gy, zeropad, R.unfold_formulation)
            want = R.reference64(x, wt, bias, gy, zeropad)
            for a, e in zip(got, want):
                assert (a is None and e is None) or torch.equal(a, e)


def test_fixture_digests_match_the_regenerated_cases():
    g = _golden.load('upsampling')
    assert _golden.jload(g['names']) == list(syn.UPSAMPLING_CASES)
    for name, (mode, use_bias, trained, shape, _) in syn.UPSAMPLING_CASES.items():
        p = _golden.jload(g[f'{name}__params'])
        inp = syn.make_upsampling_inputs(name)
        assert p['digest'] == syn.upsampling_input_digest(inp), name
        assert (p['mode'], p['use_bias'], p['trained'], tuple(p['shape'])) == (mode, use_bias, trained, shape)
        B, C, h, w = shape
        assert g[f'{name}__y'].shape == (B, C, 2 * h, 2 * w) and g[f'{name}__gx'].shape == shape
        assert g[f'{name}__gw'].shape == (C, 1, 3, 3) and ((f'{name}__gb' in g.files) == use_bias)
        assert g[f'{name}__y'].dtype == np.float32


# ------------------------------------------------------------------------------ non-finite values
from nicr_mt_scene_analysis_amd.testing import nonfinite as NF      # noqa: E402


@pytest.mark.parametrize('case', NF.up_cases(), ids=repr)
def test_nonfinite_cases_show_the_poison_and_contain_it_in_the_composition(case):
    """the condition that keeps tests/test_nonfinite_model.py honest, on the composition alone: in every poisoned
    run an output element is touched and one is not, and a NaN and a +inf leave a non-finite output"""
    for dtype in NF.DTYPES:
        assert NF.run(case, dtype) > 0
