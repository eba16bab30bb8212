"""CPU tier of the MLP decoders: exports and types, the state dicts of the four decoders and the
`InstanceHead` against the reference's recorded results, the modules on CPU tensors (the torch
composition, the path a machine without a GPU takes) against the recorded outputs and gradients, the
fixture's input digests, `ops._mlpdec_shifts`, the refusal of CPU tensors by the ops, and the two
conditions the error bounds of `testing.mlp_decoder_ref` must meet: torch's own float32 CPU result
stays inside them on every input the GPU tier uses, and two defective restatements (bilinear without
the half-pixel offset, nearest by rounding) do not."""
import numpy as np
import pytest
import torch

from nicr_mt_scene_analysis_amd import _lib as L
from nicr_mt_scene_analysis_amd import model
from nicr_mt_scene_analysis_amd import ops
from nicr_mt_scene_analysis_amd import types as T
from nicr_mt_scene_analysis_amd import utils
from nicr_mt_scene_analysis_amd.model import decoder as D
from nicr_mt_scene_analysis_amd.model.decoder import mlp_base
from nicr_mt_scene_analysis_amd.testing import mlp_decoder_cases as mc
from nicr_mt_scene_analysis_amd.testing import mlp_decoder_ref as R
from nicr_mt_scene_analysis_amd.testing.synthetic import input_digest

import _golden

MODES = ('nearest', 'bilinear')
# the cases whose every module has a CPU path (no swin LayerNorm fusion, no learned upsampling)
CPU_CASES = [k for k, c in mc.MLP_DECODER_CASES.items()
             if c['fusion'] == 'select' and 'prediction_upsampling' not in c['kwargs']]


@pytest.fixture(scope='module')
def golden():
    return _golden.load('mlp_decoder')


def build(case):
    """the decoder of a case with the case's state, in eval mode, and its inputs"""
    module = mc.build_decoder(D, model.get_encoder_decoder_fusion_class, model.get_upsampling_class, case)
    inp = mc.make_decoder_inputs(case, mc.state_shapes(module), mc.output_shapes(case))
    missing, unexpected = module.load_state_dict({k: torch.from_numpy(v) for k, v in inp['state'].items()},
                                                 strict=False)
    assert not unexpected and all(k.endswith('num_batches_tracked') for k in missing)
    return module.eval(), inp


def test_exports_and_types():
    for attr in ('DecoderBase', 'MLPDecoderBase', 'SemanticMLPDecoder', 'EmbeddingMLPDecoder', 'NormalMLPDecoder',
                 'InstanceMLPDecoder', 'InstanceHead', 'create_task_head'):
        assert getattr(model, attr) is getattr(D, attr), attr
    assert issubclass(D.MlpUpsampleConcatFunction, torch.autograd.Function)
    for cls in (D.SemanticMLPDecoder, D.EmbeddingMLPDecoder, D.NormalMLPDecoder, D.InstanceMLPDecoder):
        assert issubclass(cls, D.MLPDecoderBase) and issubclass(D.MLPDecoderBase, D.DecoderBase)
    for attr in ('EncoderSkipType', 'EncoderSkipsType', 'DecoderInputType', 'DecoderOutputType',
                 'DecoderRawOutputType', 'BatchType'):
        assert hasattr(T, attr), attr
    for fn in ('mlpdec_upsample_concat', 'mlpdec_upsample_concat_backward', 'mlpdec_route', '_mlpdec_shifts'):
        assert callable(getattr(ops, fn)), fn
    assert L.NMSA_MLPDEC_MAX_BRANCHES == 4
    x = torch.tensor([[[[3.0]], [[4.0]]]])
    for cls in (utils.NormalOutputNormalization, utils.OrientationOutputNormalization):
        got = cls()(x)
        assert torch.equal(got, x / (torch.sqrt((x ** 2).sum(1, keepdim=True)) + 1e-7))
    m, _ = build('sem_select_nearest_3')
    assert m.side_output_downscales == () and m.postprocessing is m._postprocessing
    assert type(m.postprocessing).__name__ == 'SemanticPostprocessing'
    # 'normal' stays unregistered in the factory; the decoder's default is the class itself
    with pytest.raises(NotImplementedError):
        model.postprocessing.get_postprocessing_class('normal')
    assert type(build('normal_select_bilinear_4')[0].postprocessing).__name__ == 'NormalPostprocessing'


@pytest.mark.parametrize('name', tuple(mc.MLP_DECODER_STATE_KWARGS))
def test_state_dict_keys_and_shapes(golden, name):
    recorded = _golden.jload(golden['state'])[name]
    case = dict(mc.MLP_DECODER_STATE_PROBE, decoder=name, mode='bilinear', kwargs=mc.MLP_DECODER_STATE_KWARGS[name])
    m = mc.build_decoder(D, model.get_encoder_decoder_fusion_class, model.get_upsampling_class, case)
    got = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert got == recorded and list(got) == list(recorded)
    for prefix in ('main_branch.embedding.conv.', 'skip_fusions.0.ln.', 'skip_branches.2.embedding.conv.',
                   'fuse.conv.weight', 'fuse.norm.'):
        assert any(k.startswith(prefix) for k in got), prefix
    # a reference-shaped state dict loads strictly, num_batches_tracked aside
    state = {k: torch.zeros(s) for k, s in recorded.items() if not k.endswith('num_batches_tracked')}
    state.update({k: v for k, v in m.state_dict().items() if k.endswith('num_batches_tracked')})
    m.load_state_dict(state, strict=True)


def test_learned_head_upsampling_keys():
    m, _ = build('ins_swin_bilinear_2_learned')
    keys = list(m.state_dict())
    assert '_task_head.upsampling.0.conv.weight' in keys and '_task_head.shared_conv.conv.weight' in keys
    case = dict(mc.MLP_DECODER_CASES['sem_select_nearest_3'])
    case['kwargs'] = dict(case['kwargs'], prediction_upsampling='learned-3x3')
    m = mc.build_decoder(D, model.get_encoder_decoder_fusion_class, model.get_upsampling_class, case)
    assert tuple(m.state_dict()['_task_head.upsample_0.conv.weight'].shape) == (3, 1, 3, 3)


@pytest.mark.parametrize('case', list(mc.MLP_DECODER_CASES))
def test_fixture_input_digests(golden, case):
    assert case in _golden.jload(golden['names'])
    _, inp = build(case)
    p = _golden.jload(golden[f'{case}__params'])
    assert mc.decoder_input_digest(inp) == p['digest'], 'regenerated inputs differ from the recorded ones'
    assert p['skip_keys'] == [str(d) for d in mc.MLP_DECODER_CASES[case]['skip_downs']]
    assert p['n_outputs'] == len(mc.output_shapes(case))


def test_fixture_covers_what_it_should():
    cases = mc.MLP_DECODER_CASES.values()
    assert {c['decoder'] for c in cases} == {'semantic', 'embedding', 'normal', 'instance'}
    assert {c['mode'] for c in cases} == set(MODES)
    assert {c['fusion'] for c in cases} == {'select', 'swin-ln-select'}
    assert {len(c['n_channels']) for c in cases} == {2, 3, 4}
    assert any(c['main_hw'] == (1, 2) for c in cases) and any(c['n_channels'] == (6, 5, 4, 3) for c in cases)


@pytest.mark.parametrize('case', CPU_CASES)
def test_modules_on_cpu_tensors_against_the_fixture(golden, case):
    """CPU tensors take the torch composition.  The concatenation must lie within twice the bounds of
    `mlp_decoder_ref.bounds` of the recorded one (two float32 evaluations of the recorded branch maps,
    each within one bound of the float64 value); behind it the same torch ops run on the same
    machine class: a few ulps of slack for another BLAS or thread count."""
    module, inp = build(case)
    c = mc.MLP_DECODER_CASES[case]
    p = _golden.jload(golden[f'{case}__params'])
    taps = {}
    module.fuse.register_forward_pre_hook(lambda _, args: taps.__setitem__('cat', args[0]))
    x = torch.from_numpy(inp['x']).requires_grad_(True)
    skips = mc.skips_to(inp, requires_grad=True)
    outs, side = module((x, ()), skips, {}, do_postprocessing=False)
    assert side == ()
    outs = outs if isinstance(outs, tuple) else (outs,)
    assert len(outs) == p['n_outputs']
    torch.autograd.backward(outs, [torch.from_numpy(g) for g in inp['gys']])
    embs = tuple(torch.from_numpy(golden[f'{case}__emb{i}']) for i in range(len(c['n_channels'])))
    bd = R.bounds(embs, c['mode'])
    worst = R.worst_ratio(taps['cat'], torch.from_numpy(golden[f'{case}__cat']).double(), 2 * bd['cat'])
    print('cpu module', case, 'cat / (2 bound):', round(worst, 3))
    assert worst <= 1.0
    for k, o in enumerate(outs):
        np.testing.assert_allclose(o.detach().numpy(), golden[f'{case}__out{k}'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(x.grad.numpy(), golden[f'{case}__gx'], rtol=1e-5, atol=1e-6)
    for d, s in skips.items():
        np.testing.assert_allclose(s['rgb'].grad.numpy(), golden[f'{case}__gskip{d}'], rtol=1e-5, atol=1e-6)


def test_train_mode_on_cpu_matches_the_recorded_shapes(golden):
    case = mc.MLP_DECODER_TRAIN_CASE
    module, inp = build(case)
    module.train()
    out, side = module((torch.from_numpy(inp['x']), ()), mc.skips_to(inp), {}, do_postprocessing=False)
    assert side == () and [list(out.shape)] == _golden.jload(golden['train'])['out']
    out.backward(torch.from_numpy(inp['gys'][0]))
    assert all(q.grad is not None for q in module.parameters())


@pytest.mark.parametrize('with_orientation', (False, True))
def test_instance_head_against_the_fixture(golden, with_orientation):
    k = int(with_orientation)
    n_in, per_task, (B, H, W), seed = mc.INSTANCE_HEAD_PROBE
    head = D.InstanceHead(n_in, n_channels_per_task=per_task, with_orientation=with_orientation,
                          upsampling=model.get_upsampling_class('bilinear'), n_upsamplings=1).eval()
    rng = np.random.default_rng(seed + k)
    state = mc.draw_state(rng, mc.state_shapes(head))
    x = rng.standard_normal((B, n_in, H, W)).astype(np.float32)
    assert input_digest(x, *state.values()) == _golden.jload(golden[f'head__digest{k}'])
    mc.load_state(head, state)
    outs = head(torch.from_numpy(x))
    assert len(outs) == 2 + k
    for j, o in enumerate(outs):
        np.testing.assert_allclose(o.detach().numpy(), golden[f'head__{k}_{j}'], rtol=1e-5, atol=1e-6)
    # a side-output head: 1x1 task convolutions, no upsampling
    side = D.InstanceHead(n_in, n_channels_per_task=per_task)
    assert side.task_convs[0].kernel_size == (1, 1) and len(side.upsampling) == 0
    assert head.task_convs[1].kernel_size == (3, 3)


def test_mlpdec_shifts_accepts_and_refuses():
    assert ops._mlpdec_shifts([(2, 6, 1, 2), (2, 5, 2, 4), (2, 4, 4, 8), (2, 3, 8, 16)]) == (8, 16, (3, 2, 1, 0))
    assert ops._mlpdec_shifts([(1, 1, 15, 20), (1, 9, 120, 160)]) == (120, 160, (3, 0))
    assert ops._mlpdec_shifts([(1, 1, 7, 5)]) == (7, 5, (0,))
    assert ops._mlpdec_shifts([(1, 1, 1, 1)], size=(16, 16)) == (16, 16, (4,))
    assert ops._mlpdec_shifts([(1, 1, 1, 1), (1, 1, 16, 16)]) == (16, 16, (4, 0))
    for bad in ([(1, 1, 2, 2), (1, 1, 6, 6)],               # factor 3
                [(1, 1, 1, 1), (1, 1, 32, 32)],             # factor 32
                [(1, 1, 2, 4), (1, 1, 4, 16)],              # 2 along H, 4 along W
                [(1, 1, 4, 4), (1, 1, 6, 8)],               # do not meet at one size
                [(1, 1, 8, 2), (1, 1, 2, 8)],               # neither is the output size
                [(1, 1, 4, 4)] * 5,                         # five branches
                [],
                [(1, 1, 4)],
                [(1, 0, 4, 4)]):
        with pytest.raises(ValueError):
            ops._mlpdec_shifts(bad)
    with pytest.raises(ValueError):
        ops._mlpdec_shifts([(1, 1, 4, 4)], size=(2, 2))     # a downscale


def test_cpu_tensors_are_refused_by_the_ops():
    ys, g = R.make_inputs(2, (3, 2), (2, 1), (4, 8), 0)
    with pytest.raises(L.NmsaError):
        ops.mlpdec_upsample_concat(ys, 'bilinear')
    with pytest.raises(L.NmsaError):
        ops.mlpdec_upsample_concat_backward(g, [tuple(y.shape) for y in ys], 'bilinear')
    with pytest.raises(ValueError):
        ops.mlpdec_upsample_concat(ys, 'bicubic')


def test_the_composition_runs_where_the_fused_step_does_not_apply():
    """CPU tensors, a learned mode, mixed modes and an odd factor all answer None (the composition)"""
    up = model.get_upsampling_class
    ys, _ = R.make_inputs(2, (3, 2), (2, 1), (4, 8), 0)
    ups = [up('bilinear')(n_channels=3, scale_factor=2), up('bilinear')(n_channels=2, scale_factor=1)]
    assert mlp_base._fused_mode(ups, ys) is None            # on the CPU
    got = mlp_base.upsample_concat(ups, ys)
    assert torch.equal(got, R.torch_upcat(ys, 'bilinear'))


def gpu_tier_inputs():
    """(channels, factors, hw, seed) of every input the bounds and element tiers of the GPU tests use"""
    seed = 100
    for channels, factors, sizes in mc.BOUNDS_CASES:
        for hw in sizes:
            seed += 1
            yield channels, factors, hw, seed
    for channels, factors, hw in mc.ELEMENT_CASES:
        seed += 1
        yield channels, factors, hw, seed


def torch_both(ys, g_out, mode, hw):
    """torch's float32 CPU forward and backward of the composition"""
    leaves = [y.clone().requires_grad_(True) for y in ys]
    cat = R.torch_upcat(leaves, mode, size=hw)
    cat.backward(g_out)
    return cat.detach(), tuple(t.grad for t in leaves)


@pytest.mark.parametrize('mode', MODES)
def test_torch_float32_stays_inside_the_bounds(mode):
    for channels, factors, hw, seed in gpu_tier_inputs():
        ys, g_out = R.make_inputs(mc.GPU_B, channels, factors, hw, seed)
        ref = R.reference64(ys, mode, g_out, size=hw)
        bd = R.bounds(ys, mode, g_out, size=hw)
        cat, gys = torch_both(ys, g_out, mode, hw)
        worst = [R.worst_ratio(cat, ref['cat'], bd['cat'])]
        worst += [R.worst_ratio(g, r, b) for g, r, b in zip(gys, ref['gys'], bd['gys'])]
        assert max(worst) <= 1.0, (channels, factors, hw, mode, worst)


def test_torch_float32_is_exact_on_the_exact_tier():
    """integers in -8..8 and power-of-two factors: every weight is a multiple of 1/32 and every sum is
    exact in float32, so torch's own float32 result equals the float64 value"""
    for hw in mc.EXACT_HW:
        for mode in MODES:
            ys, g_out = R.make_inputs(mc.GPU_B, mc.EXACT_CHANNELS, mc.EXACT_FACTORS, hw, 0, integer=True)
            ref = R.reference64(ys, mode, g_out, size=hw)
            cat, gys = torch_both(ys, g_out, mode, hw)
            assert torch.equal(cat.double(), ref['cat'])
            for g, r in zip(gys, ref['gys']):
                assert torch.equal(g.double(), r)


@pytest.mark.parametrize('mode,defect', (('bilinear', 'no_half_pixel'), ('nearest', 'round')))
def test_defective_restatements_fall_outside_the_bounds(mode, defect):
    ys, g_out = R.make_inputs(mc.GPU_B, (3, 2, 1, 5), (8, 4, 2, 1), (8, 16), 7)
    ref = R.reference64(ys, mode, g_out)
    bd = R.bounds(ys, mode, g_out)
    bad_cat = R.upcat64(ys, mode, defect)
    bad_gys = R.upcat_backward64(g_out, [tuple(y.shape) for y in ys], mode, defect)
    assert R.worst_ratio(bad_cat, ref['cat'], bd['cat']) > 1.0
    # the branch that already has the output size is untouched by either defect
    for i in range(3):
        assert R.worst_ratio(bad_gys[i], ref['gys'][i], bd['gys'][i]) > 1.0, i


# ------------------------------------------------------------------------------ non-finite values
from nicr_mt_scene_analysis_amd.testing import nonfinite as NF      # noqa: E402


@pytest.mark.parametrize('case', NF.mld_cases(), ids=repr)
def test_nonfinite_cases_show_the_poison_and_contain_it_in_the_composition(case):
    """the condition that keeps tests/test_nonfinite_model.py honest, on the composition alone: in every poisoned
    run an output element is touched and one is not, and a NaN and a +inf leave a non-finite output"""
    for dtype in NF.DTYPES:
        assert NF.run(case, dtype) > 0
