"""GPU tier of `model.backbone` and `model.encoder`: the golden configurations (tests/golden/backbone.npz, the
reference's own modules on the CPU) on the device, train and eval: which fused nodes are in the graph, and the
outputs, skips and gradients against the golden.

The tolerance.  A ResNet on the device differs from the CPU golden by the float32 re-association of MIOpen's
convolutions and batch norms, whatever this package adds.  That distance, the noise floor, was measured with
the plain torch composition (`backbone_cases.fused_paths_off`: `F.max_pool2d`, torch batch norm, the torch SE
fusion; the same filled weights; no code under test) against the CPU golden on an MI355X, as the largest
`backbone_cases.distance` over all records and fields of a class (docs/measurement_log.md):

    FLOOR_MAP  7.7e-6   maps and running statistics: max |d| / max |ref|       (nonbottleneck1d/se/train stage4)
    FLOOR_GRAD 7.2e-6   gx and parameter gradients: |d|_2 / |ref|_2             (nonbottleneck1d/se/train norm1.bias)

One record is apart: in basicblock/se/train the plain composition's GRADIENTS lie 5.8e-3 .. 7.1e-3 from the
golden while its maps lie within 3.1e-6: layer4 normalises over 8 values a channel there, and one discrete gate
decision below it differs between the CPU and the device.  Its gradients are held to their own measured floor,
FLOOR_GRAD_APART.  The fused paths get 4 x the floor: they add one more float32 re-association of the same size,
and the MIOpen algorithm choice varies box to box.  Measured for the fused paths with the same script: maps
7.2e-6, gradients 6.6e-6 (7.1e-3 in the record that is apart)."""
import os

import pytest
import torch

from nicr_mt_scene_analysis_amd import model
from nicr_mt_scene_analysis_amd.model import block
from nicr_mt_scene_analysis_amd.testing import backbone_cases as BC

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'backbone.npz')
RECORDS = BC.records()
FLOOR_MAP = 7.7e-6                      # measured: plain torch composition on the device against the CPU golden
FLOOR_GRAD = 7.2e-6                     # measured, the same runs
FLOOR_GRAD_APART = {'basicblock/se/train': 7.1e-3}      # measured, the same runs (see the module docstring)
FACTOR = 4.0
POOL, TAIL, FUSION = 'MaxPool3x3S2FunctionBackward', 'BatchNormTailFunctionBackward', 'SEWeightedAddFunctionBackward'


@pytest.fixture(scope='module')
def golden():
    return BC.GoldenFile(GOLDEN)


def bound(name, field):
    if BC.is_gradient(field):
        return FACTOR * FLOOR_GRAD_APART.get(name, FLOOR_GRAD)
    return FACTOR * FLOOR_MAP


def held(got, rec, name):
    worst = {}
    assert set(got) == set(rec.fields)
    for field, t in got.items():
        assert tuple(t.shape) == rec.shapes[field] and t.is_cuda, field
        d = BC.distance(BC.digest(t, field), rec.fields[field], field)
        cls = 'grad' if BC.is_gradient(field) else 'map'
        worst[cls] = max(worst.get(cls, 0.0), d)
        assert d <= bound(name, field), (name, field, d, bound(name, field))
    print(name, ' '.join(f'{k} {v:.2e}' for k, v in sorted(worst.items())))


@pytest.mark.parametrize('config,mode', RECORDS)
def test_golden_configuration_on_the_device(golden, config, mode):
    name = BC.record_name(config, mode)
    rec = golden.record(name)
    module, sha = BC.build(config)
    assert sha == rec.sha256, 'the parameter fill changed: regenerate tests/golden/backbone.npz'
    module.to(DEV)
    nodes = set()
    got = BC.run(config, mode, module, DEV, nodes)
    # 2 x 64 x 32 x 32 and below: every batch-norm tail is under block.FUSED_MIN_ELEMENTS and takes torch
    assert 2 * 64 * 32 * 32 < block.FUSED_MIN_ELEMENTS
    assert POOL in nodes and TAIL not in nodes and 'MaxPool2DWithIndicesBackward0' not in nodes, sorted(nodes)
    assert (FUSION in nodes) == (config == 'encoder/fused')
    held(got, rec, name)


@pytest.mark.parametrize('config,mode', [r for r in RECORDS if r[0] in ('basicblock/plain', 'nonbottleneck1d/se',
                                                                        'encoder/fused')])
def test_the_stem_takes_the_fused_tail_above_the_threshold(golden, monkeypatch, config, mode):
    """with the threshold lowered to these maps, stage 0 (and every block) runs `BatchNormTailFunction`"""
    monkeypatch.setattr(block, 'FUSED_MIN_ELEMENTS', 1)
    name = BC.record_name(config, mode)
    rec = golden.record(name)
    module, _ = BC.build(config)
    module.to(DEV)
    stem = (module if config != 'encoder/fused' else module.backbone_rgb).stages[0]
    x = BC.golden_input(3).to(DEV).requires_grad_(True)
    module.train(mode == 'train')
    tracked = int(stem.norm.num_batches_tracked)
    out = stem(x)
    first = out.grad_fn if stem.se is None else None
    assert first is None or type(first).__name__ == TAIL
    assert TAIL in BC.graph_node_names(out) and 'MiopenBatchNormBackward0' not in BC.graph_node_names(out)
    assert int(stem.norm.num_batches_tracked) - tracked == (1 if mode == 'train' else 0)
    module, _ = BC.build(config)                        # fresh running statistics
    module.to(DEV)
    nodes = set()
    got = BC.run(config, mode, module, DEV, nodes)
    assert {POOL, TAIL} <= nodes
    assert any('BatchNorm' in n and n != TAIL for n in nodes), sorted(nodes)     # the downsample branches stay torch
    held(got, rec, name)


def test_fused_encoder_returns_the_fused_tensor_under_rgb_and_the_depth_tensor_untouched():
    module, _ = BC.build('encoder/fused')
    module.to(DEV).eval()
    x = {'rgb': BC.golden_input(3).to(DEV), 'depth': BC.golden_input(1).to(DEV)}
    before = dict(x)
    seen = []                                           # (input dict, output dict) of every fusion, in stage order
    for f in module.fusions:
        f.register_forward_hook(lambda m, i, o: seen.append((dict(i[0]), dict(o))))      # copies: the encoder reuses the dict
    with torch.no_grad():
        feats, skips = module(x)
    assert x.keys() == before.keys() and all(x[k] is before[k] for k in x)
    assert len(seen) == 5 and sorted(skips) == ['16', '4', '8'] and feats['rgb'].shape == (2, 512, 2, 2)
    for idx, (given, out) in enumerate(seen):
        assert out['depth'] is given['depth'] and out['rgb'] is not given['rgb']
        fusion = module.fusions[idx]
        with torch.no_grad():                           # the torch composition of the same SE weighting
            want = fusion.weighting_rgb(given['rgb']) + fusion.weighting_depth(given['depth'])
        assert torch.allclose(out['rgb'], want, rtol=1e-5, atol=1e-6 * float(want.abs().max()))
        ds = str(module.backbone_rgb.stages_downsampling[idx])
        if idx in (1, 2, 3):
            assert skips[ds]['rgb'] is out['rgb'] and skips[ds]['depth'] is out['depth']
        if idx + 1 < 5:                                 # the next stage of the rgb backbone reads the FUSED tensor
            assert seen[idx + 1][0]['rgb'].shape[1] == module.backbone_rgb.stages_n_channels[idx + 1]
    assert feats['rgb'] is seen[-1][1]['rgb'] and feats['depth'] is seen[-1][1]['depth']


def test_reference_keyed_state_dicts_load_on_the_device_module(golden):
    for config in ('basicblock/se', 'encoder/fused', 'nonbottleneck1d/d16'):
        rec = golden.record(BC.record_name(config, 'train'))
        source, _ = BC.build(config)
        state = {k: source.state_dict()[k].clone() for k in rec.keys}          # the reference's keys, its order
        module, _ = BC.build(config)
        module.to(DEV)
        with torch.no_grad():
            for p in module.parameters():
                p.zero_()
        module.load_state_dict(state, strict=True)
        assert list(module.state_dict()) == rec.keys
        for k, v in module.state_dict().items():
            assert v.is_cuda and torch.equal(v.cpu(), state[k]), k


def test_half_backbone_runs_the_pool_in_its_dtype():
    b = model.get_backbone('resnet18', 'nonbottleneck1d', pretrained=False).to(DEV).to(torch.bfloat16).eval()
    x = BC.golden_input(3).to(DEV).to(torch.bfloat16).requires_grad_(True)
    s0 = b.forward_stage(0, x)
    pooled = b.maxpool(s0)
    assert pooled.dtype == torch.bfloat16 and type(pooled.grad_fn).__name__ == POOL
    assert torch.equal(pooled, torch.nn.functional.max_pool2d(s0.detach(), 3, 2, 1))
    b(x).float().sum().backward()
    assert x.grad is not None and x.grad.dtype == torch.bfloat16 and bool(torch.isfinite(x.grad.float()).all())
