"""CPU tier: the restatement of the scene head (testing/scene_head_ref.py: the kernels' sums in their order, in
float32) against the fixture tests/golden/scene_decoder.npz, recorded from the reference's unmodified
`SceneClassificationDecoder` in float32 and float64 (tools/gen_golden_scene_decoder.py).  The restatement differs
from the reference's float32 run by the order of one float32 sum per quantity, so each quantity must lie within
4 x the distance the reference's own float32 run has from its float64 run: the project's margin for one
reordered float32 sum."""
import pytest
import torch

from nicr_mt_scene_analysis_amd import model
from nicr_mt_scene_analysis_amd.testing import scene_head_ref as sr
from nicr_mt_scene_analysis_amd.testing.synthetic import input_digest

import _golden

CASES = tuple(sr.SCENE_HEAD_CASES)
QUANTITIES = ('logits', 'gx', 'gweight', 'gbias')


@pytest.fixture(scope='module')
def golden():
    return _golden.load('scene_decoder')


@pytest.fixture(scope='module')
def restated():
    out = {}
    for name in CASES:
        inp = sr.case_inputs(name)
        _, x = sr.decoder_input(inp)
        w, b, g = (torch.from_numpy(inp[k]) for k in ('weight', 'bias', 'g'))
        logits, pooled = sr.forward(x, w, b)
        gx, gw, gb = sr.backward(g, pooled, w, x.shape, x.dtype)
        out[name] = dict(logits=logits, gx=gx, gweight=gw, gbias=gb)
    return out


def test_fixture_covers_the_three_inputs(golden):
    assert tuple(_golden.jload(golden['names'])) == CASES
    shapes = [c['features'] for c in sr.SCENE_HEAD_CASES.values()]
    assert any(s is not None and s[2:] == (1, 1) for s in shapes)           # the PPM's bin-1 branch
    assert any(s is not None and s[2:] == (2, 3) for s in shapes)           # APPM at a larger validation input
    assert any(s is None for s in shapes)                                   # NoContextModule


@pytest.mark.parametrize('name', CASES)
def test_input_digests(golden, name):
    p = _golden.jload(golden[f'{name}__params'])
    assert input_digest(*sr.case_arrays(sr.case_inputs(name))) == p['digest'], \
        'regenerated inputs differ from the recorded ones'


@pytest.mark.parametrize('name', CASES)
@pytest.mark.parametrize('quantity', QUANTITIES)
def test_restatement_against_the_fixture(golden, restated, name, quantity):
    p = _golden.jload(golden[f'{name}__params'])
    want = torch.from_numpy(golden[f'{name}__{quantity}'])
    got = restated[name][quantity]
    assert want.dtype == torch.float64 and got.dtype == torch.float32 and got.shape == want.shape
    dist = float((got.double() - want).abs().max())
    bound = 4.0 * p['dist'][quantity]
    print(f'{name} {quantity}: distance {dist:.3e}, bound {bound:.3e}')
    assert p['dist'][quantity] > 0.0 and dist <= bound, (name, quantity, dist, bound)


@pytest.mark.parametrize('name', CASES)
def test_reference_float32_logits_are_as_far_as_recorded(golden, name):
    p = _golden.jload(golden[f'{name}__params'])
    d = float((torch.from_numpy(golden[f'{name}__logits32']).double() - torch.from_numpy(golden[f'{name}__logits']))
              .abs().max())
    assert d == p['dist']['logits']


@pytest.mark.parametrize('name', CASES)
def test_state_dict_keys_and_shapes(golden, name):
    p = _golden.jload(golden[f'{name}__params'])
    case = sr.SCENE_HEAD_CASES[name]
    C = (case['features'] or case['cm_output'])[1]
    m = model.SceneClassificationDecoder(n_channels_in=C, n_classes=case['n_classes'])
    own = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert own == p['state'] and list(own) == list(p['state']) == ['_task_head.weight', '_task_head.bias']
    state = {k: torch.zeros(s) for k, s in p['state'].items()}
    m.load_state_dict(state, strict=True)
