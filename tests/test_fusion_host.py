"""CPU tier of the encoder-decoder fusion: the names and the factory, the state dicts and the
pure-torch names against the reference's recorded results, the refusal of CPU tensors by the
`swin-ln-*` names, the fixture's input digests, and the two conditions the error bounds of
`testing.fusion_ref` must meet: torch's own float32 CPU result stays inside them on every input the
GPU tier uses, and a float32 evaluation with the one-pass variance E[x^2] - mean^2 does not."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nicr_mt_scene_analysis_amd import _lib as L
from nicr_mt_scene_analysis_amd import model
from nicr_mt_scene_analysis_amd.model import encoder_decoder_fusion as edf
from nicr_mt_scene_analysis_amd.testing import fusion_cases as fc
from nicr_mt_scene_analysis_amd.testing import fusion_ref as R

import _golden

NAMES = ('add', 'add-rgb', 'add-depth', 'select', 'select-rgb', 'select-depth',
         'swin-ln-add', 'swin-ln-add-rgb', 'swin-ln-add-depth',
         'swin-ln-select', 'swin-ln-select-rgb', 'swin-ln-select-depth',
         'swin-add', 'swin-add-rgb', 'swin-add-depth', 'swin-select', 'swin-select-rgb', 'swin-select-depth',
         'none')
TORCH_CASES = [n for n, c in fc.FUSION_CASES.items() if not c[0].startswith('swin-ln')]


@pytest.fixture(scope='module')
def golden():
    return _golden.load('encoder_decoder_fusion')


def build(name):
    """the module of a fixture case with the case's parameters, and its inputs as tensors"""
    fusion, n_enc, n_dec, _, _ = fc.FUSION_CASES[name]
    inp = fc.make_fusion_inputs(name)
    module = edf.get_encoder_decoder_fusion_class(fusion)(n_channels_encoder=n_enc, n_channels_decoder=n_dec)
    params = dict(module.named_parameters())
    assert list(params) == list(inp['params'])
    with torch.no_grad():
        for key, value in inp['params'].items():
            params[key].copy_(torch.from_numpy(value))
    return module, inp


def test_names_default_and_exports(golden):
    assert len(NAMES) == 19 and edf.KNOWN_ENCODER_DECODER_FUSIONS == NAMES
    assert _golden.jload(golden['known']) == list(NAMES)
    assert model.KNOWN_ENCODER_DECODER_FUSIONS is edf.KNOWN_ENCODER_DECODER_FUSIONS
    assert model.EncoderDecoderFusion is edf.EncoderDecoderFusion
    assert model.EncoderDecoderFusionSwin is edf.EncoderDecoderFusionSwin
    assert model.EncoderDecoderFusionType is edf.EncoderDecoderFusionType
    assert model.get_encoder_decoder_fusion_class is edf.get_encoder_decoder_fusion_class
    default = edf.get_encoder_decoder_fusion_class()(n_channels_encoder=4, n_channels_decoder=4)
    assert isinstance(default, edf.EncoderDecoderFusion) and not isinstance(default, edf.EncoderDecoderFusionSwin)
    assert default._fuse_features_from == 'rgb'
    assert default._fuse_operation is torch.add
    upper = edf.get_encoder_decoder_fusion_class('SWIN-LN-Select-Depth')(n_channels_encoder=4, n_channels_decoder=4)
    assert isinstance(upper, edf.EncoderDecoderFusionSwin) and upper._fuse_features_from == 'depth'
    assert isinstance(upper.ln, torch.nn.LayerNorm) and isinstance(upper.layer, torch.nn.Identity)
    assert isinstance(edf.get_encoder_decoder_fusion_class('swin-add')(4, 4).ln, torch.nn.Identity)
    for bad in ('mul', 'swin-ln', 'add-ir', ''):
        with pytest.raises(ValueError):
            edf.get_encoder_decoder_fusion_class(bad)


def test_lazy_key_and_none():
    x_dec = torch.ones(1, 4, 2, 3)
    m = edf.get_encoder_decoder_fusion_class('add')(n_channels_encoder=4, n_channels_decoder=4)
    assert m._fuse_features_from is None
    assert torch.equal(m({'anything': 2 * x_dec}, x_dec), 3 * x_dec) and m._fuse_features_from == 'anything'
    with pytest.raises(AssertionError):
        edf.get_encoder_decoder_fusion_class('select')(4, 4)({'a': x_dec, 'b': x_dec}, x_dec)
    s = edf.get_encoder_decoder_fusion_class('swin-select')(n_channels_encoder=4, n_channels_decoder=4)
    nhwc = torch.arange(24.).reshape(1, 2, 3, 4)
    assert torch.equal(s({'only': nhwc}, None), nhwc.permute(0, 3, 1, 2)) and s._fuse_features_from == 'only'
    none = edf.get_encoder_decoder_fusion_class('none')(n_channels_encoder=4, n_channels_decoder=6)
    assert none({'rgb': nhwc}, x_dec) is x_dec and none({}, None) is None
    assert not list(none.state_dict()) and not hasattr(none, 'layer')


@pytest.mark.parametrize('name', NAMES)
def test_state_dict_keys_and_shapes(golden, name):
    recorded = _golden.jload(golden['state'])[name]
    for n_enc, n_dec in fc.FUSION_STATE_CHANNELS:
        m = edf.get_encoder_decoder_fusion_class(name)(n_channels_encoder=n_enc, n_channels_decoder=n_dec)
        got = {k: list(v.shape) for k, v in m.state_dict().items()}
        assert got == recorded[f'{n_enc}_{n_dec}'] and list(got) == list(recorded[f'{n_enc}_{n_dec}'])
        assert list(dict(m.named_parameters())) == list(fc.fusion_param_shapes(name, n_enc, n_dec))


@pytest.mark.parametrize('name', TORCH_CASES)
def test_pure_torch_names_against_the_fixture_on_cpu(golden, name):
    module, inp = build(name)
    p = _golden.jload(golden[f'{name}__params'])
    x_enc = torch.from_numpy(inp['x_enc']).requires_grad_(True)
    x_dec = torch.from_numpy(inp['x_dec']).requires_grad_(True)
    y = module({p['key']: x_enc}, x_dec)
    y.backward(torch.from_numpy(inp['gy']))
    # the same torch ops on the same machine class: a few ulps of slack for another BLAS / thread count
    tol = dict(rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(y.detach().numpy(), golden[f'{name}__y'], **tol)
    for key, t in (('gx_enc', x_enc), ('gx_dec', x_dec)):
        assert (t.grad is not None) == (key in p['grads']), key
        if t.grad is not None:
            np.testing.assert_allclose(t.grad.numpy(), golden[f'{name}__{key}'], **tol)
    for key, param in module.named_parameters():
        np.testing.assert_allclose(param.grad.numpy(), golden[f'{name}__g__{key}'], **tol)


def test_output_shapes(golden):
    shapes = _golden.jload(golden['shapes'])
    B, H, W = fc.FUSION_SHAPE_INPUT
    for name in NAMES:
        assert shapes[name] == [B, 8, H, W], name
        if name.startswith('swin-ln'):
            continue                                # these need the device: tests/test_fusion.py
        m = edf.get_encoder_decoder_fusion_class(name)(n_channels_encoder=8, n_channels_decoder=8)
        x_enc = torch.zeros((B, H, W, 8) if name.startswith('swin') else (B, 8, H, W))
        assert list(m({fc.fusion_key(name): x_enc}, torch.zeros(B, 8, H, W)).shape) == shapes[name]


@pytest.mark.parametrize('name', ('swin-ln-add', 'swin-ln-select-rgb'))
@pytest.mark.parametrize('n_dec', (8, 12))
def test_swin_ln_on_a_cpu_tensor_raises(name, n_dec):
    m = edf.get_encoder_decoder_fusion_class(name)(n_channels_encoder=8, n_channels_decoder=n_dec)
    with pytest.raises(L.NmsaError):
        m({fc.fusion_key(name): torch.zeros(1, 2, 3, 8)}, torch.zeros(1, n_dec, 2, 3))


def test_fixture_digests_match_the_regenerated_cases(golden):
    assert _golden.jload(golden['names']) == list(fc.FUSION_CASES)
    for name, (fusion, n_enc, n_dec, shape, _) in fc.FUSION_CASES.items():
        p = _golden.jload(golden[f'{name}__params'])
        inp = fc.make_fusion_inputs(name)
        assert p['digest'] == fc.fusion_input_digest(inp), name
        assert (p['fusion'], p['n_enc'], p['n_dec'], tuple(p['shape'])) == (fusion, n_enc, n_dec, shape)
        assert golden[f'{name}__y'].shape == (shape[0], n_dec) + tuple(shape[1:])
        assert golden[f'{name}__y'].dtype == np.float32


def test_reference64_is_the_float64_autograd_of_the_formulation():
    x, gamma, beta, gy, add = R.make_inputs('offset_pos', 2, 5, 7, seed=3)
    x4 = x.reshape(2, 5, 1, 7).double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = R.torch_formulation(x4, g64, b64, 1e-5, add.double().reshape(2, 7, 5, 1))
    y.backward(gy.double().reshape(2, 7, 5, 1))
    ref = R.reference64(x, gamma, beta, 1e-5, add, gy)
    for got, key in ((y.detach(), 'y'), (x4.grad, 'gx'), (g64.grad, 'ggamma'), (b64.grad, 'gbeta')):
        np.testing.assert_allclose(got.reshape(ref[key].shape).numpy(), ref[key].numpy(), rtol=1e-12, atol=1e-13)


# every C of the GPU tier's bound tests (tests/test_fusion.py), with the row counts it uses
BOUND_CS = (2, 3, 7, 63, 64, 65, 96, 97, 192, 384, 768, 1536, 2047, 2048)


@pytest.mark.parametrize('C', BOUND_CS)
def test_torch_float32_meets_the_bounds_and_the_one_pass_variance_does_not(C):
    """(a) torch's float32 CPU layer_norm and autograd stay inside `bounds` on the four input classes
    (forward also on 1000 + N(0,1)), 74 rows, five seeds; (b) over the same five seeds the
    one-pass-variance control misses the y bound by more than 100x on 1000 + N(0,1) and the gx bound
    by more than 9x on -50 + 5 N(0,1): the figures the bounds were specified with"""
    eps = 1e-5
    for kind in R.INPUT_CLASSES:
        for seed in range(5):
            x, gamma, beta, gy, add = R.make_inputs(kind, 2, 37, C, seed)
            xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
            y = F.layer_norm(xr, (C,), gr, br, eps).permute(0, 2, 1) + add
            y.backward(gy)
            ref, bd = R.reference64(x, gamma, beta, eps, add, gy), R.bounds(x, gamma, beta, eps, add, gy)
            assert R.worst_ratio(y, ref['y'], bd['y']) <= 1.0, (kind, seed)
            if kind in R.FORWARD_ONLY_CLASSES:
                continue
            for got, key in ((xr.grad, 'gx'), (gr.grad, 'ggamma'), (br.grad, 'gbeta')):
                assert R.worst_ratio(got, ref[key], bd[key]) <= 1.0, (kind, seed, key)
    for kind, key, factor in (('offset_1000', 'y', 100.0), ('offset_neg', 'gx', 9.0)):
        worst = 0.0
        for seed in range(5):
            x, gamma, beta, gy, _ = R.make_inputs(kind, 2, 37, C, seed)
            y1, gx1 = R.one_pass_variance_f32(x, gamma, beta, eps, gy)
            ref, bd = R.reference64(x, gamma, beta, eps, None, gy), R.bounds(x, gamma, beta, eps, None, gy)
            worst = max(worst, R.worst_ratio({'y': y1, 'gx': gx1}[key], ref[key], bd[key]))
        assert worst > factor, (kind, key, worst)


@pytest.mark.parametrize('cus', (1, 3, 256))
def test_backward_workspace_follows_the_assumed_compute_units(monkeypatch, cus):
    """the partial sums of nmsa_ln_nhwc_nchw_bwd are one line [2][C] of floats per workgroup, and the
    grid is min(tiles, 4 workgroups per compute unit) (csrc/ln_transpose.hip LNT_BWD_BLOCKS_PER_CU):
    the size query follows NMSA_ASSUME_CUS, on both sides of the cap and at it.  No device needed."""
    monkeypatch.setenv('NMSA_ASSUME_CUS', str(cus))
    assert L.device_geometry()[0] == cus
    cap, query = 4 * cus, L.lib().nmsa_ln_nhwc_nchw_bwd_workspace_bytes
    for C in (64, 160):
        for tiles in (max(1, cap - 1), cap, cap + 1, 3 * cap + 1):
            for B, P in ((1, 32 * tiles), (1, 32 * tiles - 31)) + (((2, 16 * tiles),) if tiles % 2 == 0 else ()):
                assert B * -(-P // 32) == tiles
                assert query(B, P, C) == min(tiles, cap) * 2 * C * 4, (cus, C, B, P)


# ------------------------------------------------------------------------------ non-finite values
from nicr_mt_scene_analysis_amd.testing import nonfinite as NF      # noqa: E402


@pytest.mark.parametrize('case', NF.lnt_cases(), ids=repr)
def test_nonfinite_cases_show_the_poison_and_contain_it_in_the_composition(case):
    """the condition that keeps tests/test_nonfinite_model.py honest, on the composition alone: in every poisoned
    run an output element is touched and one is not, and a NaN and a +inf leave a non-finite output"""
    for dtype in NF.LNT_PAIRS:
        assert NF.run(case, dtype) > 0
