"""CPU tier: the host side of the scene classification decoder and the panoptic helper.  On CPU tensors the
decoder runs the reference's `adaptive_avg_pool2d -> flatten -> linear` in plain torch; the per-condition routing
on device tensors is in tests/test_scene_decoder.py."""
import pytest
import torch
import torch.nn.functional as F

from nicr_mt_scene_analysis_amd import _lib as L
from nicr_mt_scene_analysis_amd import model
from nicr_mt_scene_analysis_amd import ops
from nicr_mt_scene_analysis_amd.model import decoder as D
from nicr_mt_scene_analysis_amd.testing import mlp_decoder_cases as mc
from nicr_mt_scene_analysis_amd.testing import scene_head_ref as sr


def build(name):
    case, inp = sr.SCENE_HEAD_CASES[name], sr.case_inputs(name)
    C = (case['features'] or case['cm_output'])[1]
    m = D.SceneClassificationDecoder(n_channels_in=C, n_classes=case['n_classes'], unused_parameter=3)
    m.load_state_dict({'_task_head.weight': torch.from_numpy(inp['weight']),
                       '_task_head.bias': torch.from_numpy(inp['bias'])}, strict=True)
    return m, inp


def test_exports():
    for attr in ('SceneClassificationDecoder', 'SceneHeadFunction', 'PanopticHelper'):
        assert getattr(model, attr) is getattr(D, attr), attr
    assert issubclass(D.SceneClassificationDecoder, D.DecoderBase)
    assert issubclass(D.SceneHeadFunction, torch.autograd.Function)
    assert issubclass(D.PanopticHelper, torch.nn.Module)
    for fn in ('scene_head', 'scene_head_backward', 'scene_head_route'):
        assert callable(getattr(ops, fn)), fn
    assert L.NMSA_SCENE_HEAD_MAX_CHANNELS == 2048
    assert (L.NMSA_SH_ROUTE_UNIT, L.NMSA_SH_ROUTE_VECTOR, L.NMSA_SH_ROUTE_ELEMENT) == (1, 2, 4)
    assert 'scene classification decoder' in D.__doc__ and 'panoptic helper' in D.__doc__


def test_default_postprocessing_is_the_class_and_the_factory_still_refuses_scene():
    with pytest.raises(NotImplementedError):
        model.postprocessing.get_postprocessing_class('scene')
    m, _ = build('ppm_1x1')
    assert type(m.postprocessing).__name__ == 'ScenePostprocessing' and m.postprocessing is m._postprocessing
    assert m.side_output_downscales == ()


@pytest.mark.parametrize('name', tuple(sr.SCENE_HEAD_CASES))
@pytest.mark.parametrize('train', (True, False))
def test_module_on_cpu_tensors_is_the_torch_composition(name, train):
    m, inp = build(name)
    m.train(train)
    x, pooled_map = sr.decoder_input(inp, requires_grad=True)
    assert not m.takes_hip_path(pooled_map)
    out, side = m(x, None, {}, do_postprocessing=False)
    assert side is None
    g = torch.from_numpy(inp['g'])
    out.backward(g)
    x2 = pooled_map.detach().clone().requires_grad_(True)
    w = m._task_head.weight.detach().clone().requires_grad_(True)
    b = m._task_head.bias.detach().clone().requires_grad_(True)
    want = sr.torch_composition(x2, w, b)
    want.backward(g)
    assert torch.equal(out, want)
    assert torch.equal(pooled_map.grad, x2.grad)
    assert torch.equal(m._task_head.weight.grad, w.grad) and torch.equal(m._task_head.bias.grad, b.grad)
    # only the first context feature is read
    for t in x[1][1:] + ((x[0],) if x[1] else ()):
        assert t.grad is None


def test_takes_hip_path_is_false_for_every_fallback_input_on_the_cpu():
    m = D.SceneClassificationDecoder(n_channels_in=4, n_classes=3)
    x = torch.zeros((2, 4, 2, 4))
    fallbacks = {
        'cpu': x,
        'float64': x.double(),
        'integer': x.to(torch.int32),
        'empty': x[:0],
        'non-dense': x[:, :, :, ::2],
        'channels-last': x.contiguous(memory_format=torch.channels_last),
        '3-d': x[0],
    }
    for what, t in fallbacks.items():
        assert not m.takes_hip_path(t), what
    # the limits of the entry points
    assert not D.SceneClassificationDecoder(L.NMSA_SCENE_HEAD_MAX_CHANNELS + 1, 3).takes_hip_path(
        torch.zeros((1, L.NMSA_SCENE_HEAD_MAX_CHANNELS + 1, 1, 1)))
    assert not D.SceneClassificationDecoder(4, L.NMSA_SCENE_MAX_CLASSES + 1).takes_hip_path(x)
    out, _ = m((fallbacks['channels-last'], ()), None, {}, do_postprocessing=False)
    assert torch.equal(out, F.linear(x.mean((2, 3)), m._task_head.weight, m._task_head.bias))


def test_cpu_tensors_are_refused_by_the_ops():
    x, w, b = torch.zeros((1, 2, 1, 1)), torch.zeros((3, 2)), torch.zeros((3,))
    with pytest.raises(L.NmsaError):
        ops.scene_head(x, w, b)
    with pytest.raises(L.NmsaError):
        ops.scene_head_backward(torch.zeros((1, 3)), torch.zeros((1, 2)), w, x.shape, x.dtype)


class _Recorder:
    calls = []

    def postprocess(self, output, batch, is_training):
        _Recorder.calls.append((output, batch, is_training))
        return 'postprocessed'


def _pair():
    """a semantic and an instance MLP decoder over the same encoder geometry (the CPU-capable 'select' case of
    tests/test_mlp_decoder_host.py, once per decoder) and their shared inputs"""
    sem_case = mc.MLP_DECODER_CASES['sem_select_nearest_3']
    ins_case = dict(sem_case, decoder='instance', kwargs=dict(n_channels_per_task=4, with_orientation=True), seed=911)
    modules = []
    for case in (sem_case, ins_case):
        m = mc.build_decoder(D, model.get_encoder_decoder_fusion_class, model.get_upsampling_class, case)
        rng_inp = mc.make_decoder_inputs(case, mc.state_shapes(m), mc.output_shapes(case))
        mc.load_state(m, rng_inp['state'])
        modules.append(m.eval())
    inp = mc.make_decoder_inputs(sem_case, {}, ())
    return modules[0], modules[1], inp


def test_panoptic_helper_runs_both_decoders_and_combines_their_raw_outputs():
    sem, ins, inp = _pair()
    helper = D.PanopticHelper(sem, ins, postprocessing=_Recorder).eval()
    assert helper.semantic_decoder is sem and helper.instance_decoder is ins
    assert isinstance(helper.postprocessing, _Recorder)
    x = (torch.from_numpy(inp['x']), ())
    skips = mc.skips_to(inp)
    with torch.no_grad():
        (s_out, i_out), (s_side, i_side) = helper(x, skips, {}, do_postprocessing=False)
        want_s, want_s_side = sem(x, skips, {}, do_postprocessing=False)
        want_i, want_i_side = ins(x, skips, {}, do_postprocessing=False)
    assert torch.equal(s_out, want_s) and s_side == want_s_side
    assert isinstance(i_out, tuple) and len(i_out) == len(want_i) == 3
    assert all(torch.equal(a, b) for a, b in zip(i_out, want_i)) and i_side == want_i_side
    assert not _Recorder.calls
    batch = {'marker': 1}
    with torch.no_grad():
        assert helper(x, skips, batch) == 'postprocessed'
    (output, got_batch, is_training), = _Recorder.calls
    assert got_batch is batch and is_training is False
    assert torch.equal(output[0][0], want_s) and output[1] == (want_s_side, want_i_side)
    _Recorder.calls.clear()


def test_panoptic_helper_side_output_downscales_is_the_union():
    class Stub(torch.nn.Module):
        def __init__(self, scales):
            super().__init__()
            self.side_output_downscales = scales

    helper = D.PanopticHelper(Stub((8, 16)), Stub((16, 32)), postprocessing=_Recorder)
    assert sorted(helper.side_output_downscales) == [8, 16, 32]
    sem, ins, _ = _pair()
    assert D.PanopticHelper(sem, ins, postprocessing=_Recorder).side_output_downscales == ()
