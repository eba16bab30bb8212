"""TEST INFRASTRUCTURE — never imported by the product path.

The seeded cases of tests/golden/context_module.npz (tools/gen_golden_context_module.py) and the
shapes of the GPU tier (tests/test_context_module.py).  The inputs are regenerated here; the fixture
holds the reference's results and a digest of these inputs."""
from typing import Dict

import numpy as np

from .synthetic import input_digest

# name: (module name, n_channels_in, n_channels_out, (B, H, W), input_size, upsampling, seed)
# BatchNorm runs in eval mode with seeded running statistics in all of them
CONTEXT_CASES = {
    'ppm_1_5_3x2': ('ppm-1-5', 4, 3, (2, 3, 2), (3, 2), 'bilinear', 210),             # ph > H
    'ppm_1_5_7x9_nearest': ('ppm', 4, 3, (2, 7, 9), (7, 9), 'nearest', 211),          # overlapping windows
    'ppm_1_5_10_15x20': ('ppm-1-5-10', 3, 2, (1, 15, 20), (15, 20), 'bilinear', 212),
    'ppm_1_2_4_8_8x16': ('ppm-1-2-4-8', 4, 3, (1, 8, 16), (8, 16), 'bilinear', 213),  # equal windows
    'ppm_1_2_4_8_7x9_nearest': ('ppm-1-2-4-8', 4, 2, (1, 7, 9), (7, 9), 'nearest', 214),
    'appm_1_2_4_8_8x16': ('appm-1-2-4-8', 4, 3, (1, 8, 16), (4, 8), 'bilinear', 215),  # pools (2,4,8,16)^2
    'appm_1_5_6x4': ('appm-1-5', 4, 4, (2, 6, 4), (3, 4), 'bilinear', 216),           # multipliers (2, 1)
    'none_4_6': ('none', 4, 6, (2, 3, 4), (3, 4), 'bilinear', 217),
}
# one train-mode case: only that it runs, and its shapes
CONTEXT_TRAIN_CASE = ('ppm-1-5', 4, 3, (2, 7, 9), (7, 9), 'bilinear', 230)
# the probe of the state-dict record of all nine names: (n_channels_in, n_channels_out, input_size)
CONTEXT_STATE_PROBE = (8, 6, (15, 20))
# (h, w) -> multipliers recorded for an APPM built for input_size (15, 20)
CONTEXT_APPM_PROBES = ((15, 20), (30, 40), (22, 29), (23, 31), (8, 10), (38, 50), (60, 61))

NAME_BINS = {'ppm': (1, 5), 'ppm-1-5': (1, 5), 'ppm-1-5-10': (1, 5, 10), 'ppm-1-2-4-8': (1, 2, 4, 8),
             'appm': (1, 5), 'appm-1-5': (1, 5), 'appm-1-5-10': (1, 5, 10), 'appm-1-2-4-8': (1, 2, 4, 8),
             'none': ()}

# ---- the GPU tier: B = 2 everywhere
GPU_CHANNELS = (3, 8, 64)           # not a multiple of the planes per workgroup, one group, several
GPU_HW = ((1, 1), (3, 2), (7, 9), (8, 16), (15, 20), (16, 32), (30, 40))
GPU_BINS = ((1, 5), (1, 5, 10), (1, 2, 4, 8), (1, 2, 3, 6))
# the exact tier: every window area and resize weight a power of two
EXACT_HW = ((8, 16), (16, 32))
EXACT_BINS = (1, 2, 4, 8)
# APPM off the square: a (32, 64) map for input_size (16, 32), pools (2, 4, 8, 16) squared
APPM_HW, APPM_INPUT_SIZE, APPM_BINS = (32, 64), (16, 32), (1, 2, 4, 8)
# one geometry on each side of both route limits (plane <= 2048 elements, H * pw <= 512 row sums):
# ((H, W), sizes, expect the LDS route)
ROUTE_CASES = (((32, 64), ((2, 2), (16, 16)), True), ((3, 683), ((1, 1), (2, 5)), False),
               ((64, 32), ((3, 8),), True), ((64, 32), ((3, 9),), False))


def sizes_of(bins):
    return tuple((b, b) for b in bins)


def context_param_shapes(name: str, n_in: int, n_out: int) -> Dict[str, tuple]:
    """parameters and buffers (without num_batches_tracked) of a context module, state-dict order"""
    shapes = {}

    def cna(prefix, ci, co):
        shapes[f'{prefix}.conv.weight'] = (co, ci, 1, 1)
        for key in ('weight', 'bias', 'running_mean', 'running_var'):
            shapes[f'{prefix}.norm.{key}'] = (co,)

    bins = NAME_BINS[name]
    if name == 'none':
        if n_in != n_out:
            cna('layer', n_in, n_out)
        return shapes
    red = n_in // len(bins)
    for i in range(len(bins)):
        cna(f'features.{i}.1', n_in, red)
    cna('final_conv', n_in + red * len(bins), n_out)
    return shapes


def make_context_inputs(case) -> Dict[str, object]:
    """The inputs of one case (a name of CONTEXT_CASES or a case tuple), float32: 'x' [B, n_in, H, W],
    'gy' [B, n_out, H, W] (the upstream gradient of the module output), 'state' {state-dict key:
    values}.  Generator draws and float32 casts only."""
    name, n_in, n_out, (B, H, W), _, _, seed = CONTEXT_CASES[case] if isinstance(case, str) else case
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, n_in, H, W)).astype(np.float32)
    gy = rng.standard_normal((B, n_out, H, W)).astype(np.float32)
    state = {}
    for key, shape in context_param_shapes(name, n_in, n_out).items():
        draw = rng.standard_normal(shape)
        if key.endswith('conv.weight'):
            state[key] = (0.5 * draw).astype(np.float32)
        elif key.endswith('running_var'):
            state[key] = (0.5 + draw * draw).astype(np.float32)
        elif key.endswith('norm.weight'):
            state[key] = (1.0 + 0.25 * draw).astype(np.float32)
        else:
            state[key] = (0.5 * draw).astype(np.float32)
    return {'x': x, 'gy': gy, 'state': state}


def context_input_digest(inputs) -> str:
    return input_digest(inputs['x'], inputs['gy'], *inputs['state'].values())
