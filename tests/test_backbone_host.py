"""CPU tier of `model.backbone` and `model.encoder`: on CPU tensors every module takes its torch path, and that
composition is held to the recorded reference (tests/golden/backbone.npz, written by
tools/gen_golden_backbone.py from the reference's own modules); the interface, the stage properties of all
twelve names and three blocks, the skip choice, the checkpoint rewriting and the refusals.  No test needs a
device."""
import inspect
import os
import warnings
from collections import OrderedDict

import pytest
import torch
from torch import nn

from nicr_mt_scene_analysis_amd import model, ops
from nicr_mt_scene_analysis_amd.model import backbone as backbone_module
from nicr_mt_scene_analysis_amd.testing import backbone_cases as BC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'backbone.npz')
RECORDS = BC.records()


@pytest.fixture(scope='module')
def golden():
    return BC.GoldenFile(GOLDEN)


def quiet_backbone(*args, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                 # resnet50 / resnet101 with a non-bottleneck block
        return model.get_backbone(*args, **kwargs)


# ------------------------------------------------------------------------------ the fixture
def test_the_fixture_is_data_of_the_stated_layout(golden):
    assert sorted(golden.index) == sorted(BC.record_name(*r) for r in RECORDS)
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(GOLDEN), 'mlp_decoder.npz')) \
        or os.path.getsize(GOLDEN) <= 400 * 1024
    kinds = {BC.CONFIGS[c][0] for c, _ in RECORDS}
    assert kinds == {'backbone', 'encoder', 'fused'} and any(BC.CONFIGS[c][3] for c, _ in RECORDS)
    for config, mode in RECORDS:
        rec = golden.record(BC.record_name(config, mode))
        assert all(t.dtype == torch.float32 and t.ndim == 1 for t in rec.fields.values())
        if BC.CONFIGS[config][0] == 'backbone':
            assert {f'stage{i}' for i in range(5)} | {'gx'} <= set(rec.fields)
        else:
            assert {'skip/4/depth', 'skip/8/depth', 'skip/16/depth', 'out/depth', 'gx/depth'} <= set(rec.fields)


def same(a, b, rtol=1e-6):
    # the comparison tests/test_block_host.py holds its CPU composition to: the same ATen ops in the same order
    # give the same bits on the machine and with the thread count the fixture was recorded with; torch's CPU
    # convolutions split their sums by thread count and instruction set, so elsewhere the last place differs
    return torch.equal(a, b) or torch.allclose(a, b, rtol=rtol, atol=1e-7)


@pytest.mark.parametrize('config,mode', RECORDS)
def test_cpu_composition_reproduces_the_recorded_reference(golden, config, mode):
    rec = golden.record(BC.record_name(config, mode))
    module, sha = BC.build(config)
    assert sha == rec.sha256, 'the parameter fill changed: regenerate tests/golden/backbone.npz'
    assert list(module.state_dict()) == rec.keys                   # the reference's state-dict keys, in its order
    tracked = {k: int(v) for k, v in module.state_dict().items() if k.endswith('num_batches_tracked')}
    got = BC.run(config, mode, module)
    assert set(got) == set(rec.fields)
    for field, t in got.items():
        assert tuple(t.shape) == rec.shapes[field], field
        rtol = 1e-5 if field.startswith('grad/') else 1e-6
        assert same(BC.digest(t, field), rec.fields[field], rtol), field
    for k, v in module.state_dict().items():
        if k.endswith('num_batches_tracked'):
            assert int(v) - tracked[k] == (1 if mode == 'train' else 0), k


def test_fused_encoder_outputs_and_untouched_input(golden):
    module, _ = BC.build('encoder/fused')
    module.eval()
    x = {'rgb': BC.golden_input(3), 'depth': BC.golden_input(1)}
    before = dict(x)
    with torch.no_grad():
        feats, skips = module(x)
    assert x.keys() == before.keys() and all(x[k] is before[k] for k in x)
    assert sorted(feats) == ['depth', 'rgb'] and sorted(skips) == ['16', '4', '8']
    assert all(sorted(v) == ['depth', 'rgb'] for v in skips.values())
    assert feats['rgb'].shape == (2, 512, 2, 2) and skips['4']['rgb'].shape == (2, 64, 16, 16)
    # se-add-uni-rgb: the depth branch is the depth backbone's own output
    with torch.no_grad():
        d = x['depth']
        for idx in range(5):
            d = module.backbone_depth.forward_stage(idx, d)
    assert torch.equal(d, feats['depth']) and not torch.equal(feats['rgb'], feats['depth'])
    assert module.skips_n_channels == (64, 128, 256) and module.n_channels_out == 512 and module.downsampling == 32


# ------------------------------------------------------------------------------ interface
def test_exports_and_signatures():
    for name in ('KNOWN_BACKBONES', 'Backbone', 'ResNetBackbone', 'ResNetSEBackbone', 'get_resnet_backbone',
                 'get_backbone', 'convert_torchvision_resnet_state_dict', 'EncoderBase', 'Encoder',
                 'FusedRGBDEncoder', 'EncoderType', 'get_encoder', 'MaxPool2d', 'MaxPool3x3S2Function'):
        assert hasattr(model, name), name
    assert list(model.KNOWN_BACKBONES) == [f'resnet{n}{s}' for s in ('', '-d16', 'se') for n in (18, 34, 50, 101)]
    for cls in (model.ResNetBackbone, model.ResNetSEBackbone):
        sig = inspect.signature(cls.__init__).parameters
        assert list(sig) == ['self', 'block', 'layers', 'zero_init_residual', 'groups', 'width_per_group',
                             'replace_stride_with_dilation', 'normalization', 'activation', 'n_input_channels']
        assert (sig['groups'].default, sig['width_per_group'].default, sig['n_input_channels'].default) == (1, 64, 3)
    sig = inspect.signature(model.get_backbone).parameters
    assert list(sig) == ['name', 'resnet_block', 'n_input_channels', 'normalization', 'activation', 'pretrained',
                         'pretrained_filepath', 'kwargs']
    assert sig['pretrained'].default is True and sig['pretrained_filepath'].default is None
    sig = inspect.signature(model.get_encoder).parameters
    assert list(sig) == ['backbone_rgb', 'backbone_depth', 'backbone_rgbd', 'fusion', 'normalization', 'activation',
                         'skip_downsamplings']
    assert sig['skip_downsamplings'].default == (4, 8, 16)
    with pytest.raises(ValueError):
        model.ResNetBackbone(model.BasicBlock, [1, 1, 1, 1], replace_stride_with_dilation=[True])
    with pytest.raises(TypeError):
        model.Backbone()                                # abstract


def test_sub_module_names_and_the_stage_list():
    b = quiet_backbone('resnet18se', 'basicblock', pretrained=False)
    assert [k for k, _ in b.named_children()] == ['conv1', 'norm1', 'act', 'maxpool', 'layer1', 'layer2', 'layer3',
                                                  'layer4', 'se_conv1', 'se_layer1', 'se_layer2', 'se_layer3',
                                                  'se_layer4']
    assert isinstance(b.maxpool, model.MaxPool2d) and isinstance(b.maxpool, nn.MaxPool2d)
    assert (b.maxpool.kernel_size, b.maxpool.stride, b.maxpool.padding) == (3, 2, 1)
    assert (b.conv1.kernel_size, b.conv1.stride, b.conv1.padding, b.conv1.bias) == ((7, 7), (2, 2), (3, 3), None)
    down = b.layer2[0].downsample
    assert isinstance(down, nn.Sequential) and [k for k, _ in down.named_children()] == ['0', '1']
    assert isinstance(down[0], nn.Conv2d) and down[0].kernel_size == (1, 1) and isinstance(down[1], nn.BatchNorm2d)
    assert b.layer1[0].downsample is None and len(b.layer1) == 2
    stem = b.stages[0]
    assert stem.conv is b.conv1 and stem.norm is b.norm1 and stem.act is b.act and stem.se is b.se_conv1
    assert b.stages[1][0] is b.maxpool and b.stages[1][1] is b.layer1 and b.stages[1][2] is b.se_layer1
    assert not any(k.startswith(('_stages', 'stages', 'stem')) for k in b.state_dict())
    plain = quiet_backbone('resnet18', 'basicblock', pretrained=False)
    assert plain.stages[0].se is None and plain.stages[2] is plain.layer2 and len(plain.stages) == 5
    assert len(quiet_backbone('resnet34', 'nonbottleneck1d', pretrained=False).layer3) == 6
    assert len(quiet_backbone('resnet101', 'bottleneck', pretrained=False).layer3) == 23


@pytest.mark.parametrize('block', model.KNOWN_BLOCKS)
@pytest.mark.parametrize('name', model.KNOWN_BACKBONES)
def test_stage_properties_of_every_name_and_block(name, block):
    if block == 'basicblock' and 'd16' in name:
        with pytest.raises(NotImplementedError):        # BasicBlock refuses the dilation of layer4's later blocks
            quiet_backbone(name, block, pretrained=False)
        return
    b = quiet_backbone(name, block, pretrained=False)
    e = 4 if block == 'bottleneck' else 1
    assert b.stages_n_channels == [64, 64 * e, 128 * e, 256 * e, 512 * e]
    assert b.stages_downsampling == ([2, 4, 8, 16, 16] if 'd16' in name else [2, 4, 8, 16, 32])
    assert b.stages_memory_layout == ['nchw'] * 5
    assert isinstance(b, model.ResNetSEBackbone) == name.endswith('se') and isinstance(b, model.Backbone)
    assert b.layer4[0].downsample is not None


def test_skip_choice_on_a_d16_backbone():
    from nicr_mt_scene_analysis_amd.model.encoder import select_skip_stages
    assert select_skip_stages([2, 4, 8, 16, 16], (4, 8, 16)) == [False, True, True, True, False]
    assert select_skip_stages([2, 4, 8, 16, 32], (4, 8, 16)) == [False, True, True, True, False]
    assert select_skip_stages([2, 4, 8, 16, 32], (2, 32)) == [True, False, False, False, True]
    assert select_skip_stages([2, 4, 4, 8, 8], (4, 8)) == [False, False, True, True, False]
    with pytest.raises(ValueError):
        select_skip_stages([2, 4, 8, 16, 32], (3,))
    enc = model.get_encoder(backbone_depth=quiet_backbone('resnet18-d16', 'nonbottleneck1d', 1, pretrained=False))
    assert isinstance(enc, model.Encoder) and enc.skips_n_channels == (64, 128, 256) and enc.downsampling == 16
    assert enc.skips_downsamplings == (4, 8, 16) and enc.n_channels_out == 512
    enc.eval()
    x = {'depth': torch.randn(1, 1, 64, 64)}
    with torch.no_grad():
        feats, skips = enc(x)
    assert list(x) == ['depth'] and list(feats) == ['depth'] and list(skips) == ['4', '8', '16']
    assert skips['16']['depth'].shape == (1, 256, 4, 4) and feats['depth'].shape == (1, 512, 4, 4)
    assert skips['16']['depth'] is not feats['depth']


def test_get_encoder_chooses_the_encoder():
    def bb(c):
        return quiet_backbone('resnet18', 'nonbottleneck1d', c, pretrained=False)
    fused = model.get_encoder(bb(3), bb(1), fusion='se-add-uni-rgb')
    assert isinstance(fused, model.FusedRGBDEncoder) and len(fused.fusions) == 5
    assert all(isinstance(f, model.EncoderRGBDFusionWeightedAdd) for f in fused.fusions)
    assert isinstance(model.get_encoder(backbone_rgbd=bb(4)), model.Encoder)
    assert model.get_encoder(backbone_rgb=bb(3)).backbone.conv1.in_channels == 3
    with pytest.raises(ValueError):
        model.get_encoder()


# ------------------------------------------------------------------------------ weights
def checkpoint_of(b, container, prefix):
    state = OrderedDict((prefix + k, v.clone()) for k, v in b.state_dict().items())
    state[prefix + 'fc.weight'], state[prefix + 'fc.bias'] = torch.zeros(10, 512), torch.zeros(10)
    state[prefix + 'fc_embedding.weight'], state[prefix + 'fc_embedding.bias'] = torch.zeros(4, 512), torch.zeros(4)
    return {container: state}


@pytest.mark.parametrize('container', ('state_dict', 'model'))
@pytest.mark.parametrize('prefix', ('', 'model.', 'backbone.', '_orig_mod.', 'model.backbone._orig_mod.'))
def test_checkpoint_rewriting_through_a_file(tmp_path, container, prefix):
    src = quiet_backbone('resnet18', 'basicblock', pretrained=False)
    BC.fill_parameters(src, 17)
    path = str(tmp_path / 'ckpt.pth')
    torch.save(checkpoint_of(src, container, prefix), path)
    w = src.conv1.weight.detach()
    for channels, want in ((3, w), (1, w.sum(1, keepdim=True)), (4, torch.cat([w, w.sum(1, keepdim=True)], 1) / 2)):
        got = model.get_backbone('resnet18', 'basicblock', channels, pretrained=True, pretrained_filepath=path)
        assert got.conv1.weight.shape == (64, channels, 7, 7) and torch.equal(got.conv1.weight.detach(), want)
        for k, v in src.state_dict().items():
            if k != 'conv1.weight':
                assert torch.equal(got.state_dict()[k], v), k
    with pytest.raises(RuntimeError):                   # strict: another architecture's keys do not load
        model.get_backbone('resnet18se', 'basicblock', pretrained=True, pretrained_filepath=path)


def test_torchvision_key_conversion():
    src = quiet_backbone('resnet18', 'basicblock', pretrained=False)
    BC.fill_parameters(src, 23)
    tv = OrderedDict((k.replace('norm', 'bn'), v) for k, v in src.state_dict().items())
    tv['fc.weight'], tv['fc.bias'] = torch.zeros(1000, 512), torch.zeros(1000)
    assert 'bn1.weight' in tv and 'layer2.0.bn2.running_var' in tv and 'layer2.0.downsample.1.weight' in tv
    frozen = list(tv)
    for channels in (3, 1):
        conv = model.convert_torchvision_resnet_state_dict(tv, channels)
        assert list(tv) == frozen and list(conv) == list(src.state_dict())
        target = quiet_backbone('resnet18', 'basicblock', channels, pretrained=False)
        target.load_state_dict(conv, strict=True)
        want = src.conv1.weight.detach() if channels == 3 else src.conv1.weight.detach().sum(1, keepdim=True)
        assert torch.equal(target.conv1.weight.detach(), want)
    bott = quiet_backbone('resnet50', 'bottleneck', pretrained=False)
    tv50 = OrderedDict((k.replace('norm', 'bn'), v) for k, v in bott.state_dict().items())
    assert 'layer1.0.bn3.weight' in tv50
    assert list(model.convert_torchvision_resnet_state_dict(tv50)) == list(bott.state_dict())


def test_the_library_never_downloads_and_refuses_swin():
    with pytest.raises(ValueError, match='pretrained_filepath'):
        model.get_backbone('resnet18', 'basicblock')                        # pretrained defaults to True
    with pytest.raises(ValueError, match='pretrained_filepath'):
        model.get_backbone('resnet34', 'nonbottleneck1d', pretrained=True)
    with pytest.raises(ValueError, match='never downloads'):
        model.get_resnet_backbone('resnet18', model.BasicBlock, pretrained_torchvision=True)
    for name in ('swin-t', 'swin-t-v2', 'swin-multi-t-128', 'SWIN-B'):
        with pytest.raises(ValueError, match='torchvision'):
            model.get_backbone(name, 'basicblock', pretrained=False)
    with pytest.raises(ValueError, match='Unknown backbone'):
        model.get_backbone('vgg16', 'basicblock', pretrained=False)
    assert not any('swin' in n for n in model.KNOWN_BACKBONES) and len(model.KNOWN_BACKBONES) == 12
    assert backbone_module.get_backbone is model.get_backbone


# ------------------------------------------------------------------------------ torch path on the CPU
def test_cpu_tensors_never_touch_the_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError('the library must not be called on this path')
    for name in ('maxpool3x3s2', 'maxpool3x3s2_backward', 'bntail_stats', 'bntail_apply', 'sefuse_squeeze'):
        monkeypatch.setattr(ops, name, refuse)
    module, _ = BC.build('encoder/fused')
    x = {'rgb': BC.golden_input(3).requires_grad_(True), 'depth': BC.golden_input(1)}
    feats, _ = module(x)
    feats['rgb'].sum().backward()
    assert x['rgb'].grad is not None
