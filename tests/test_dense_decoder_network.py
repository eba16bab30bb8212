"""GPU tier: the dense decoders composed with the rest of the package in one training step.

`FusedRGBDEncoder` (two ResNet18 backbones of NonBottleneck1D blocks, SE-weighted add) -> pyramid pooling context
module -> `SemanticDecoder` and `InstanceDecoder` (NonBottleneck1D, 'add-rgb' fusion, learned upsampling) -> the
package's task helpers' losses, one step at 64x96 (`testing.network_cases.step`).  Every gradient is finite and the
fused node appears once per decoder module that upsamples and fuses: three per decoder.  The helpers run without
multiscale supervision (the side targets are the business of the multiscale generator's own tests), so the side
heads take no gradient here."""
import collections

import pytest
import torch

from nicr_mt_scene_analysis_amd import model
from nicr_mt_scene_analysis_amd import task_helper as T
from nicr_mt_scene_analysis_amd.testing import backbone_cases as BC
from nicr_mt_scene_analysis_amd.testing import block_cases
from nicr_mt_scene_analysis_amd.testing import network_cases as NC

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
HW = (64, 96)
NODE = 'UpsampleAddFunctionBackward'


def build_network(upsampling='learned-3x3'):
    block = model.get_block_class('nonbottleneck1d', dropout_p=0.0)
    encoder = model.FusedRGBDEncoder(
        model.get_backbone('resnet18', block, n_input_channels=3, pretrained=False),
        model.get_backbone('resnet18', block, n_input_channels=1, pretrained=False),
        fusion=model.get_encoder_fusion_class('se-add'), skip_downsamplings=BC.SKIPS)
    ctx = model.get_context_module('ppm', n_channels_in=encoder.n_channels_out, n_channels_out=NC.CONTEXT_CHANNELS,
                                   input_size=(HW[0] // encoder.downsampling, HW[1] // encoder.downsampling),
                                   activation='relu', upsampling='bilinear')
    common = dict(n_channels_in=NC.CONTEXT_CHANNELS, downsampling_in=encoder.downsampling, n_channels=(64, 48, 32),
                  downsamplings=(16, 8, 4), block=block, n_blocks=1,
                  fusion=model.get_encoder_decoder_fusion_class('add-rgb'),
                  fusion_n_channels=tuple(reversed(encoder.skips_n_channels)),
                  fusion_downsamplings=tuple(reversed(BC.SKIPS)), upsampling=model.get_upsampling_class(upsampling),
                  prediction_upsampling=model.get_upsampling_class('learned-3x3'))
    decoders = {'semantic': model.SemanticDecoder(n_classes=NC.N_CLASSES, **common),
                'instance': model.InstanceDecoder(with_orientation=True, **common)}
    net = NC.Network(encoder, ctx, decoders)
    BC.fill_parameters(net)
    block_cases.randomise_running_stats(net, NC.STATS_SEED)
    return net


def helpers():
    out = {'semantic': T.SemanticTaskHelper(n_classes=NC.N_CLASSES, disable_multiscale_supervision=True),
           'instance': T.InstanceTaskHelper(semantic_n_classes=NC.N_CLASSES, semantic_classes_is_thing=NC.IS_THING,
                                            disable_multiscale_supervision=True)}
    for h in out.values():
        h.initialize(DEV)
    return out


@pytest.mark.parametrize('upsampling', ('learned-3x3', 'bilinear'))
def test_one_training_step_with_the_dense_decoders(upsampling):
    net = build_network(upsampling).to(DEV).train()
    batch = NC.make_batch(2, HW, seed=3, device=DEV)
    nodes = collections.Counter()
    out = NC.step(net, batch, helpers(), nodes=nodes)
    fused_steps = sum(1 for d in net.decoders.values() for m in d.decoder_modules
                      if isinstance(m.upsample, model.Upsampling))
    assert fused_steps == 6 and nodes[NODE] == 6
    assert tuple(out['raw/semantic'].shape) == (2, NC.N_CLASSES) + HW
    assert [tuple(out[f'raw/instance/{i}'].shape) for i in range(3)] == [(2, c) + HW for c in (1, 2, 2)]
    for d in net.decoders.values():
        assert d.side_output_downscales == (32, 16, 8)
    losses = {k: float(v) for k, v in out.items() if k.startswith('loss/')}
    assert losses and all(v == v and abs(v) != float('inf') for v in losses.values()), losses
    grads = {k: v for k, v in out.items() if k.startswith(('grad/', 'gx/'))}
    assert all(bool(torch.isfinite(v).all()) for v in grads.values())
    for name in ('grad/decoders.semantic.decoder_modules.0.conv.conv.weight',
                 'grad/decoders.instance.decoder_modules.2.blocks.0.conv1_1.weight',
                 'grad/decoders.semantic.fusions.0.layer.conv.weight', 'gx/depth', 'gx/rgb'):
        assert float(grads[name].abs().max()) > 0, name
    if upsampling == 'learned-3x3':
        assert float(grads['grad/decoders.semantic.decoder_modules.1.upsample.conv.weight'].abs().max()) > 0
