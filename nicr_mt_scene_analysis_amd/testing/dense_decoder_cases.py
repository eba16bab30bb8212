"""TEST INFRASTRUCTURE — never imported by the product path.

The seeded cases of tests/golden/dense_decoder.npz (tools/gen_golden_dense_decoder.py).  The inputs are
regenerated here; the fixture holds the reference's results and a digest of these inputs."""
from typing import Dict

import numpy as np
import torch

from .mlp_decoder_cases import draw_state
from .mlp_decoder_cases import load_state         # noqa: F401  (the tests take them from here)
from .mlp_decoder_cases import skips_to           # noqa: F401
from .mlp_decoder_cases import state_shapes       # noqa: F401
from .synthetic import input_digest

# name: dict(decoder, mode, block, n_in, down_in, n_channels, downs, skip_channels, skip_downs, main_hw, B, kwargs,
#            seed).  The main map has downsampling `down_in`; module i brings it to downs[i]; the head upsamples
# log2(downs[-1]) times, so every output has 16x the main map's size.  The fusion is 'add-rgb', the head's
# upsampling bilinear, n_blocks 1.  The records are taken in training mode (side outputs exist) with every
# BatchNorm in eval mode (the seeded running statistics) and the NonBottleneck1D dropout at p = 0.
# The 'nearest' / 'bilinear' cases run on CPU tensors too (the torch composition); the learned modes have no CPU
# path in this package.
DENSE_DECODER_CASES = {
    # three modules, one fusion with the 1x1 channel adapter (5 -> 3)
    'sem_nb1d_bilinear_3': dict(decoder='semantic', mode='bilinear', block='nonbottleneck1d', n_in=6, down_in=16,
                                n_channels=(4, 3, 2), downs=(8, 4, 2), skip_channels=(4, 5, 2),
                                skip_downs=(8, 4, 2), main_hw=(1, 2), B=1, kwargs=dict(n_classes=2), seed=410),
    'ins_basic_learned_2': dict(decoder='instance', mode='learned-3x3', block='basicblock', n_in=5, down_in=16,
                                n_channels=(4, 2), downs=(8, 4), skip_channels=(4, 2), skip_downs=(8, 4),
                                main_hw=(1, 2), B=1, kwargs=dict(n_channels_per_task=3), seed=411),
    # a skip only at 1/4: the first module's upsampling is not followed by a fusion
    'nor_nb1d_nearest_2': dict(decoder='normal', mode='nearest', block='nonbottleneck1d', n_in=4, down_in=16,
                               n_channels=(3, 2), downs=(8, 4), skip_channels=(3,), skip_downs=(4,),
                               main_hw=(1, 2), B=1, kwargs=dict(), seed=412),
    # a skip only at 1/8; the last module keeps the resolution: no upsampling, no side output, no fusion
    'sem_basic_zeropad_3': dict(decoder='semantic', mode='learned-3x3-zeropad', block='basicblock', n_in=4,
                                down_in=16, n_channels=(3, 2, 2), downs=(8, 4, 4), skip_channels=(3,),
                                skip_downs=(8,), main_hw=(1, 2), B=1, kwargs=dict(n_classes=2), seed=413),
}
# one case fully in training mode (batch statistics: B = 2): only that it runs, and its shapes
DENSE_DECODER_TRAIN_CASE = dict(DENSE_DECODER_CASES['sem_nb1d_bilinear_3'], B=2, main_hw=(2, 3), seed=430)
# the probe of the state-dict record of the three decoders (constructor arguments besides the task's own)
DENSE_DECODER_STATE_PROBE = dict(mode='learned-3x3', block='nonbottleneck1d', n_in=24, down_in=32,
                                 n_channels=(16, 12, 8), downs=(16, 8, 4), skip_channels=(16, 10, 8),
                                 skip_downs=(16, 8, 4))
DENSE_DECODER_STATE_KWARGS = {'semantic': dict(n_classes=5), 'normal': dict(),
                              'instance': dict(with_orientation=True, n_channels_per_task=4)}
N_BLOCKS = 1
FUSION = 'add-rgb'
HEAD_UPSAMPLING = 'bilinear'


def case_of(case) -> dict:
    return DENSE_DECODER_CASES[case] if isinstance(case, str) else case


def decoder_class(pkg, name: str):
    """the class of decoder `name` in `pkg` (this package's model.decoder, or the reference's)"""
    return getattr(pkg, {'semantic': 'SemanticDecoder', 'normal': 'NormalDecoder', 'instance': 'InstanceDecoder'}[name])


def build_decoder(pkg, fusion_factory, upsampling_factory, block_factory, case, fusion=FUSION, postprocessing=None):
    """decoder of `case` from the classes of `pkg` with the given factories (name -> class)"""
    c = case_of(case)
    kwargs = dict(c['kwargs'])
    if postprocessing is not None:
        kwargs['postprocessing'] = postprocessing
    block_kwargs = dict(dropout_p=0.0) if c['block'] == 'nonbottleneck1d' else {}
    return decoder_class(pkg, c['decoder'])(
        n_channels_in=c['n_in'], downsampling_in=c['down_in'], n_channels=c['n_channels'], downsamplings=c['downs'],
        block=block_factory(c['block'], **block_kwargs), n_blocks=N_BLOCKS, fusion=fusion_factory(fusion),
        fusion_n_channels=c['skip_channels'], fusion_downsamplings=c['skip_downs'],
        upsampling=upsampling_factory(c['mode']), prediction_upsampling=upsampling_factory(HEAD_UPSAMPLING), **kwargs)


def record_mode(module) -> None:
    """the mode the records are taken in: training (side outputs), every BatchNorm on its running statistics"""
    module.train()
    for m in module.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.eval()


def fused_steps(case):
    """(module index, fusion index, downsampling) of every step that upsamples and then fuses a skip"""
    c = case_of(case)
    steps, current, j = [], c['down_in'], 0
    for i, down in enumerate(c['downs']):
        upsamples = down < current
        current = min(current, down)
        if current in c['skip_downs']:
            if upsamples:
                steps.append((i, j, current))
            j += 1
    return tuple(steps)


def output_shapes(case):
    """the shapes of the decoder's outputs (a tuple for the instance decoder) from the case alone"""
    c = case_of(case)
    B, H, W = c['B'], c['main_hw'][0] * c['down_in'], c['main_hw'][1] * c['down_in']
    if c['decoder'] == 'semantic':
        return ((B, c['kwargs']['n_classes'], H, W),)
    if c['decoder'] == 'normal':
        return ((B, 3, H, W),)
    return ((B, 1, H, W), (B, 2, H, W)) + (((B, 2, H, W),) if c['kwargs'].get('with_orientation') else ())


def side_output_shapes(case):
    """per side output (one per module that upsamples) the shapes of its head's outputs"""
    c = case_of(case)
    outs, current = [], c['down_in']
    for down in c['downs']:
        if down < current:
            f = c['down_in'] // current
            hw = (c['main_hw'][0] * f, c['main_hw'][1] * f)
            outs.append(tuple(s[:2] + hw for s in output_shapes(case)))
            current = down
    return tuple(outs)


def make_decoder_inputs(case, shapes: Dict[str, tuple]) -> Dict[str, object]:
    """The inputs of one case, float32: 'x' [B, n_in, h, w], 'skips' {'<down>': {'rgb': NCHW map}}, 'gys' (one
    upstream gradient per output), 'gsides' (per side output one per head output), 'state' {state-dict key:
    values} for the parameter `shapes`.  Generator draws and float32 casts."""
    c = case_of(case)
    rng = np.random.default_rng(c['seed'])
    B, (h, w) = c['B'], c['main_hw']
    x = rng.standard_normal((B, c['n_in'], h, w)).astype(np.float32)
    skips = {}
    for n, down in zip(c['skip_channels'], c['skip_downs']):
        f = c['down_in'] // down
        skips[str(down)] = {'rgb': rng.standard_normal((B, n, h * f, w * f)).astype(np.float32)}
    gys = tuple(rng.standard_normal(s).astype(np.float32) for s in output_shapes(case))
    gsides = tuple(tuple(rng.standard_normal(s).astype(np.float32) for s in side) for side in side_output_shapes(case))
    return {'x': x, 'skips': skips, 'gys': gys, 'gsides': gsides, 'state': draw_state(rng, shapes)}


def decoder_input_digest(inputs) -> str:
    return input_digest(inputs['x'], *(s['rgb'] for s in inputs['skips'].values()), *inputs['gys'],
                        *(g for side in inputs['gsides'] for g in side), *inputs['state'].values())


def flat_outputs(outs, sides):
    """the main outputs and every side output's outputs as one flat tuple of tensors, in order"""
    flat = list(outs) if isinstance(outs, tuple) else [outs]
    for side in sides:
        flat += list(side) if isinstance(side, tuple) else [side]
    return tuple(flat)


def flat_gradients(inputs, dtype=torch.float32, device=None):
    """the upstream gradients in the order of `flat_outputs`"""
    gs = list(inputs['gys']) + [g for side in inputs['gsides'] for g in side]
    return [torch.from_numpy(g).to(dtype=dtype, device=device) for g in gs]
