"""TEST INFRASTRUCTURE — never imported by the product path.

The seeded cases of tests/golden/mlp_decoder.npz (tools/gen_golden_mlp_decoder.py) and the shapes of
the GPU tier (tests/test_mlp_decoder.py).  The inputs are regenerated here; the fixture holds the
reference's results and a digest of these inputs."""
from typing import Dict

import numpy as np
import torch

from .synthetic import input_digest

# name: dict(decoder, mode, fusion, n_in, down_in, n_channels, skip_channels, skip_downs, heads, main_hw,
#            B, kwargs, seed).  The main map has downsampling `down_in`, the heads work at `heads`, so
# the factors are down_in / heads and skip_downs / heads.  BatchNorm runs in eval mode with seeded
# running statistics.  'swin-ln-select' skips are NHWC dicts {'<down>': {'rgb': [B, h, w, C]}},
# 'select' skips NCHW.  A 'select' case runs on CPU tensors too (the torch composition); the
# swin LayerNorm fusion and the 'learned-3x3' head upsampling have no CPU path.
MLP_DECODER_CASES = {
    # four branches, factors (8, 4, 2, 1), a main map of 1x2: both source rows clamp
    'sem_swin_bilinear_4': dict(decoder='semantic', mode='bilinear', fusion='swin-ln-select', n_in=5, down_in=32,
                                n_channels=(6, 5, 4, 3), skip_channels=(4, 3, 2), skip_downs=(16, 8, 4), heads=4,
                                main_hw=(1, 2), B=1, kwargs=dict(n_classes=2, n_upsamplings=1), seed=310),
    # three branches, factors (8, 4, 1)
    'sem_select_nearest_3': dict(decoder='semantic', mode='nearest', fusion='select', n_in=4, down_in=32,
                                 n_channels=(3, 2, 2), skip_channels=(3, 2), skip_downs=(16, 4), heads=4,
                                 main_hw=(1, 2), B=2, kwargs=dict(n_classes=3, n_upsamplings=1), seed=311),
    # two branches, factors (2, 1), odd map sizes
    'emb_select_bilinear_2': dict(decoder='embedding', mode='bilinear', fusion='select', n_in=3, down_in=8,
                                  n_channels=(4, 3), skip_channels=(2,), skip_downs=(4,), heads=4,
                                  main_hw=(3, 5), B=2, kwargs=dict(embedding_dim=4, n_upsamplings=1), seed=312),
    'emb_swin_nearest_3': dict(decoder='embedding', mode='nearest', fusion='swin-ln-select', n_in=3, down_in=16,
                               n_channels=(2, 3, 2), skip_channels=(3, 2), skip_downs=(8, 4), heads=4,
                               main_hw=(2, 3), B=1, kwargs=dict(embedding_dim=3, n_channels_out=5, n_upsamplings=1),
                               seed=313),
    # heads at 1/2: one x2 upsampling in the head; factors (8, 4, 2, 1)
    'normal_select_bilinear_4': dict(decoder='normal', mode='bilinear', fusion='select', n_in=4, down_in=16,
                                     n_channels=(3, 2, 2, 1), skip_channels=(3, 2, 2), skip_downs=(8, 4, 2), heads=2,
                                     main_hw=(2, 1), B=1, kwargs=dict(), seed=314),
    'normal_swin_nearest_2': dict(decoder='normal', mode='nearest', fusion='swin-ln-select', n_in=3, down_in=8,
                                  n_channels=(2, 2), skip_channels=(3,), skip_downs=(2,), heads=2,
                                  main_hw=(2, 3), B=1, kwargs=dict(), seed=315),
    'ins_select_bilinear_3': dict(decoder='instance', mode='bilinear', fusion='select', n_in=4, down_in=16,
                                  n_channels=(3, 2, 1), skip_channels=(2, 2), skip_downs=(8, 2), heads=2,
                                  main_hw=(1, 2), B=1, kwargs=dict(n_channels_per_task=4, with_orientation=True),
                                  seed=316),
    # the head's upsampling learned (HIP), the branches' bilinear
    'ins_swin_bilinear_2_learned': dict(decoder='instance', mode='bilinear', fusion='swin-ln-select', n_in=3, down_in=4,
                                        n_channels=(2, 2), skip_channels=(2,), skip_downs=(2,), heads=2,
                                        main_hw=(2, 4), B=1,
                                        kwargs=dict(n_channels_per_task=3, prediction_upsampling='learned-3x3'),
                                        seed=317),
}
# one train-mode case: only that it runs, and its shapes
MLP_DECODER_TRAIN_CASE = dict(MLP_DECODER_CASES['sem_select_nearest_3'], mode='bilinear', seed=330)
# the probe of the state-dict record of the four decoders (constructor arguments besides the task's own)
MLP_DECODER_STATE_PROBE = dict(n_in=12, down_in=32, n_channels=(8, 6, 4, 2), skip_channels=(10, 6, 4),
                               skip_downs=(16, 8, 4), fusion='swin-ln-select', heads=4)
MLP_DECODER_STATE_KWARGS = {'semantic': dict(n_classes=5), 'embedding': dict(embedding_dim=6, n_channels_out=7),
                            'normal': dict(), 'instance': dict(with_orientation=True, n_channels_per_task=4)}
# InstanceHead on its own: (n_channels_in, n_channels_per_task, (B, H, W), seed)
INSTANCE_HEAD_PROBE = (3, 2, (1, 3, 4), 340)

# ---- the GPU tier: B = 2 everywhere (tests/test_mlp_decoder.py says why these)
GPU_B = 2
EXACT_CHANNELS, EXACT_FACTORS = (3, 2, 1, 5), (8, 4, 2, 1)
EXACT_HW = ((8, 16), (16, 24))
# widths off the vector width: (channel counts, factors, output size)
ELEMENT_CASES = (((3, 2), (2, 1), (4, 6)), ((3,), (1,), (3, 5)))
# (channel counts, factors, output sizes)
BOUNDS_CASES = (
    ((3, 2, 1, 5), (8, 4, 2, 1), ((8, 16), (40, 48))),
    ((64, 3), (2, 1), ((6, 8), (40, 48))),
    ((3,), (1,), ((7, 8), (48, 64))),
    ((5,), (16,), ((16, 16),)),                 # a 1x1 source
    ((3, 2, 4), (4, 4, 2), ((8, 8), (48, 64))),
)


def case_of(case) -> dict:
    return MLP_DECODER_CASES[case] if isinstance(case, str) else case


def decoder_class(pkg, name: str):
    """the class of decoder `name` in `pkg` (this package's model.decoder, or the reference's)"""
    return getattr(pkg, {'semantic': 'SemanticMLPDecoder', 'embedding': 'EmbeddingMLPDecoder',
                         'normal': 'NormalMLPDecoder', 'instance': 'InstanceMLPDecoder'}[name])


def build_decoder(pkg, fusion_factory, upsampling_factory, case, postprocessing=None):
    """decoder of `case` from the classes of `pkg` with the given factories (name -> class)"""
    c = case_of(case)
    kwargs = dict(c['kwargs'])
    if 'prediction_upsampling' in kwargs:
        kwargs['prediction_upsampling'] = upsampling_factory(kwargs['prediction_upsampling'])
    if postprocessing is not None:
        kwargs['postprocessing'] = postprocessing
    return decoder_class(pkg, c['decoder'])(
        n_channels_in=c['n_in'], downsampling_in=c['down_in'], n_channels=c['n_channels'],
        fusion=fusion_factory(c['fusion']), fusion_n_channels=c['skip_channels'],
        fusion_downsamplings=c['skip_downs'], downsampling_in_heads=c['heads'],
        upsampling=upsampling_factory(c['mode']), **kwargs)


def state_shapes(module) -> Dict[str, tuple]:
    """parameters and buffers without num_batches_tracked, state-dict order"""
    return {k: tuple(v.shape) for k, v in module.state_dict().items() if not k.endswith('num_batches_tracked')}


def draw_state(rng, shapes: Dict[str, tuple]) -> Dict[str, np.ndarray]:
    state = {}
    for key, shape in shapes.items():
        draw = rng.standard_normal(shape)
        if key.endswith('running_var'):
            state[key] = (0.5 + draw * draw).astype(np.float32)
        elif key.endswith('norm.weight') or key.endswith('ln.weight'):
            state[key] = (1.0 + 0.25 * draw).astype(np.float32)
        else:
            state[key] = (0.5 * draw).astype(np.float32)
    return state


def make_decoder_inputs(case, shapes: Dict[str, tuple], out_shapes) -> Dict[str, object]:
    """The inputs of one case, float32: 'x' [B, n_in, h, w], 'skips' {'<down>': {'rgb': map}} (NHWC for a
    swin fusion, NCHW otherwise), 'gys' (one upstream gradient per output, shapes `out_shapes`),
    'state' {state-dict key: values} for the parameter `shapes`.  Generator draws and float32 casts."""
    c = case_of(case)
    rng = np.random.default_rng(c['seed'])
    B, (h, w) = c['B'], c['main_hw']
    x = rng.standard_normal((B, c['n_in'], h, w)).astype(np.float32)
    skips = {}
    for n, down in zip(c['skip_channels'], c['skip_downs']):
        f = c['down_in'] // down
        shape = (B, h * f, w * f, n) if c['fusion'].startswith('swin') else (B, n, h * f, w * f)
        skips[str(down)] = {'rgb': rng.standard_normal(shape).astype(np.float32)}
    gys = tuple(rng.standard_normal(tuple(s)).astype(np.float32) for s in out_shapes)
    return {'x': x, 'skips': skips, 'gys': gys, 'state': draw_state(rng, shapes)}


def output_shapes(case):
    """the shapes of the decoder's outputs (a tuple for the instance decoder) from the case alone"""
    c = case_of(case)
    f = c['down_in'] // c['heads']
    n_up = c['kwargs'].get('n_upsamplings', c['heads'] // 2)
    H, W = c['main_hw'][0] * f << n_up, c['main_hw'][1] * f << n_up
    B = c['B']
    if c['decoder'] == 'semantic':
        return ((B, c['kwargs']['n_classes'], H, W),)
    if c['decoder'] == 'embedding':
        return ((B, c['kwargs']['embedding_dim'], H, W),)
    if c['decoder'] == 'normal':
        return ((B, 3, H, W),)
    return ((B, 1, H, W), (B, 2, H, W)) + (((B, 2, H, W),) if c['kwargs'].get('with_orientation') else ())


def decoder_input_digest(inputs) -> str:
    return input_digest(inputs['x'], *(s['rgb'] for s in inputs['skips'].values()), *inputs['gys'],
                        *inputs['state'].values())


def load_state(module, state) -> None:
    module.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=False)


def skips_to(inputs, device=None, requires_grad=False):
    """the skip dict as torch tensors (leaves)"""
    out = {}
    for key, d in inputs['skips'].items():
        t = torch.from_numpy(d['rgb'])
        if device is not None:
            t = t.to(device)
        out[key] = {'rgb': t.requires_grad_(requires_grad)}
    return out
