"""CPU tier of the composed network (`testing/network_cases.py`): the builder is deterministic, the plain
composition in float32 lies near its float64 self, three deliberately defective compositions lie OUTSIDE the bound
the GPU tier holds the fused network to (an end-to-end bound over a whole network still sees one wrong node), and
the input seeds keep every stem max-pool window clear of a tie.

The bound is the GPU tier's: `network_cases.bound`, FACTOR x the floor measured on the device (see
tests/test_network.py).  The CPU's float32 is one more re-association of the same arithmetic, so it is held to it
too."""
import copy

import pytest
import torch
import torch.nn.functional as F

from nicr_mt_scene_analysis_amd.model import encoder_fusion, upsampling
from nicr_mt_scene_analysis_amd.model.context_module import appm, ppm
from nicr_mt_scene_analysis_amd.model.decoder import mlp_base
from nicr_mt_scene_analysis_amd.testing import network_cases as NC

SMALL = NC.SHAPES[1]
SHA256 = {'A': '846c29621d84a32f1b8980d9217fc56e61fbfc0ddb03b9d7b4a3d4595c9eb769',
          'B': '5712c1c4a684f20c16f1b8d01a730f6daf4118d379d50581adb19fd1d9bcd78e'}


def doubled(batch):
    return {k: v.double() if v.is_floating_point() else v for k, v in batch.items()}


@pytest.fixture(scope='module')
def cases():
    """config -> (float32 network in training mode, float32 batch, the float64 oracle's step) at 64 x 160"""
    made = {}

    def get(config):
        if config not in made:
            net, _ = NC.build(config, SMALL)
            net.train()
            batch = NC.make_batch(2, SMALL, NC.input_seed(config, 2, SMALL, 'train'))
            with NC.plain_composition():
                ref = NC.step(copy.deepcopy(net).double(), doubled(batch), NC.plain_helpers())
            made[config] = (net, batch, ref)
        return made[config]
    return get


@pytest.mark.parametrize('config', NC.CONFIGS)
def test_builder_is_deterministic(config):
    shas = {NC.build(config, hw)[1] for hw in NC.SHAPES} | {NC.build(config, SMALL)[1]}
    assert shas == {SHA256[config]}


@pytest.mark.parametrize('config', NC.CONFIGS)
def test_module_tree_gives_the_node_counts(config):
    net, _ = NC.build(config, SMALL)
    assert NC.expected_node_counts(net) == {'pool': 2, 'tail': 18, 'se': 5, 'ppm_pool': 1, 'ppm_upcat': 1,
                                            'mlp_upcat': 3, 'learned_up': 6, 'losses': 3}
    # 2 x 3 downsample branches, the context module's branches and final convolution, 3 x fuse, the instance head
    assert NC.expected_torch_batch_norms(net) == {'A': 6 + 3 + 3 + 1, 'B': 6 + 5 + 3 + 1}[config]


@pytest.mark.parametrize('config', NC.CONFIGS)
def test_step_returns_every_loss_output_gradient_and_buffer(cases, config):
    net, _, ref = cases(config)
    losses = {k for k in ref if k.startswith('loss/')}
    assert losses == {'loss/' + k for k in (
        'semantic_loss_main', 'semantic_total_loss', 'instance_center_loss_main', 'instance_offset_loss_main',
        'instance_orientation_loss_main', 'instance_center_total_loss', 'instance_offset_total_loss',
        'instance_orientation_total_loss', 'normal_loss_main', 'normal_total_loss')}
    assert {k for k in ref if k.startswith('raw/')} == {'raw/semantic', 'raw/instance/0', 'raw/instance/1',
                                                        'raw/instance/2', 'raw/normal'}
    assert ref['raw/semantic'].shape == (2, NC.N_CLASSES) + SMALL and ref['raw/instance/2'].shape == (2, 2) + SMALL
    assert {k for k in ref if k.startswith(('out/', 'skip/'))} == {f'{p}/{m}' for p in ('out', 'skip/4', 'skip/8',
                                                                                       'skip/16')
                                                                   for m in ('rgb', 'depth')}
    assert ref['out/rgb'].shape == (2, 512, 2, 5)
    params = dict(net.named_parameters())
    assert {k[len('grad/'):] for k in ref if k.startswith('grad/')} == set(params)
    assert {k[len('after/'):] for k in ref if k.startswith('after/')} == set(net.state_dict()) - set(params)
    assert all(bool(torch.isfinite(v.double()).all()) for v in ref.values())
    assert all(int(v) == 1 for k, v in ref.items() if k.endswith('num_batches_tracked'))
    assert float(ref['gx/rgb'].abs().max()) > 0 and float(ref['gx/depth'].abs().max()) > 0


def test_plain_composition_restores_what_it_replaces():
    fusion = encoder_fusion.EncoderRGBDFusionWeightedAdd
    before = (ppm.pyramid_forward, appm.pyramid_forward, mlp_base.upsample_concat, upsampling.Upsampling.forward,
              fusion.forward, fusion._fused_act, F.batch_norm)
    for defect in (None,) + NC.DEFECTS:
        with pytest.raises(ZeroDivisionError):
            with NC.plain_composition(defect):
                assert ppm.pyramid_forward is not before[0] and mlp_base.upsample_concat is not before[2]
                1 / 0
        assert (ppm.pyramid_forward, appm.pyramid_forward, mlp_base.upsample_concat, upsampling.Upsampling.forward,
                fusion.forward, fusion._fused_act, F.batch_norm) == before


@pytest.mark.parametrize('config', NC.CONFIGS)
def test_float32_plain_composition_lies_near_the_oracle(cases, config):
    net, batch, ref = cases(config)
    name = NC.case_name(config, 2, SMALL, 'train')
    with NC.plain_composition():
        got = NC.step(copy.deepcopy(net), batch, NC.plain_helpers())
    print(name, {k: f'{d:.2e} ({f})' for k, (d, f) in NC.worst_distances(got, ref).items()})
    for field, d in NC.distances(got, ref).items():
        assert d <= NC.bound(name, NC.field_class(field)), (field, d)


@pytest.mark.parametrize('defect', NC.DEFECTS)
@pytest.mark.parametrize('config', NC.CONFIGS)
def test_defective_composition_lies_outside_the_bound(cases, config, defect):
    net, batch, ref = cases(config)
    name = NC.case_name(config, 2, SMALL, 'train')
    with NC.plain_composition(defect):
        got = NC.step(copy.deepcopy(net).double(), doubled(batch), NC.plain_helpers())
    worst = NC.worst_distances(got, ref)
    print(name, defect, {k: f'{d:.2e} ({f})' for k, (d, f) in worst.items()})
    outside = {cls for cls, (d, _) in worst.items() if d > NC.bound(name, cls)}
    assert outside, worst
    want = {'se_depth': {'map', 'grad', 'loss', 'stat'}, 'ppm_branch_grad': {'grad'}, 'biased_var': {'stat'}}[defect]
    assert outside == want


@pytest.mark.parametrize('config,B,hw,mode', sorted(NC.INPUT_SEEDS))
def test_input_seed_keeps_the_pool_windows_clear_of_a_tie(config, B, hw, mode):
    net, _ = NC.build(config, hw, **({'appm_input_size': NC.B1_APPM_INPUT_SIZE} if B == 1 else {}))
    net.double().train(mode == 'train')
    batch = NC.make_batch(B, hw, NC.input_seed(config, B, hw, mode), dtype=torch.float64)
    with NC.plain_composition():
        margin = NC.stem_pool_margin(net, batch)
    print(NC.case_name(config, B, hw, mode), f'margin {margin:.1f} roundings')
    assert margin >= NC.MARGIN


def test_floors_are_measured_numbers():
    assert all(v > 0 for v in NC.FLOOR.values()) and all(v > 0 for f in NC.FLOOR_STEPS for v in f.values())
    assert all(key[0].startswith('A/') for key in list(NC.FLOOR_APART) + list(NC.FLOOR_STEPS_APART))
