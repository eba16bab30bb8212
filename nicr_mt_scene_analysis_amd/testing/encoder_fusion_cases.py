"""TEST INFRASTRUCTURE — never imported by the product path.

The shapes and the fixture layout of the encoder RGB-D fusion tests, shared by the host tier, the GPU
tier and tools/gen_golden_encoder_fusion.py."""
import json

import numpy as np
import torch

from .. import _lib as L

ACTS = ('relu', 'silu')
NAMES = ('se-add', 'add', 'add-uni-rgb', 'add-uni-depth', 'se-add-uni-rgb', 'se-add-uni-depth', 'none')
# name -> (use_se_weighting, destinations) as the reference sets them
EXPECTED = {
    'se-add': (True, ('rgb', 'depth')), 'add': (False, ('rgb', 'depth')),
    'add-uni-rgb': (False, ('rgb',)), 'add-uni-depth': (False, ('depth',)),
    'se-add-uni-rgb': (True, ('rgb',)), 'se-add-uni-depth': (True, ('depth',)),
    'none': (False, ()),
}

# ---------------------------------------------------------------------------- GPU-tier shapes
B = 2                                   # a plane index must not run into the next image
CHANNELS = (16, 48, 80)                 # C // 16 = 1, 3, 5; B * C no multiple of 64 planes
WIDE_C, WIDE_HW = 512, (3, 5)           # once, for the loops of the excite kernels
WAVE_MAX = L.NMSA_SEFUSE_WAVE_PLANE_MAX
BLOCK_HW = (3, (WAVE_MAX + 3) // 3)     # 3 x 683 = 2049 elements: one past the wave route
EXACT_HW = (8, 16)
# 1 element; fewer than a wave's lanes; exact; 300, no multiple of 8; several trips of a wave; block route
PLANES = ((1, 1), (3, 5), EXACT_HW, (15, 20), (30, 40), BLOCK_HW)
# (C, (H, W)) of the bounds tier: every plane at 48 channels, the other channel counts at two planes
SHAPES = tuple((48, hw) for hw in PLANES) + tuple((c, hw) for c in (16, 80) for hw in ((3, 5), (15, 20))) \
    + ((WIDE_C, WIDE_HW),)

assert BLOCK_HW[0] * BLOCK_HW[1] > WAVE_MAX >= 30 * 40


def vec_width(dtype) -> int:
    """elements of a 16-byte access"""
    return 4 if dtype == torch.float32 else 8


def expected_route(dtype, hw, aligned: bool = True) -> int:
    n = hw[0] * hw[1]
    return ((L.NMSA_SEFUSE_ROUTE_VECTOR if aligned and n % vec_width(dtype) == 0 else L.NMSA_SEFUSE_ROUTE_ELEMENT)
            | (L.NMSA_SEFUSE_ROUTE_WAVE if n <= WAVE_MAX else L.NMSA_SEFUSE_ROUTE_BLOCK))


# ---------------------------------------------------------------------------- the fixture
GOLDEN_SHAPES = ((2, 32, 5, 7), (2, 48, 4, 6))
GOLDEN_FIELDS = ('x_rgb', 'x_depth', 'gy_rgb', 'gy_depth', 'y_rgb', 'y_depth', 'gx_rgb', 'gx_depth')


def record_name(name: str, act: str, shape_index: int) -> str:
    return f'{name}/{act}/{shape_index}'


def golden_records():
    return [(name, act, k) for name in NAMES for act in ACTS for k in range(len(GOLDEN_SHAPES))]


def golden_inputs(shape_index: int):
    """seeded float32 inputs of a fixture shape: x_rgb, x_depth multiples of 1/16 in about -3..3.5, the
    fixed upstream gradients gy_rgb, gy_depth multiples of 1/8 on about one position in twelve and 0
    elsewhere (coarse and sparse values keep the compressed fixture small; the dense gradients are the
    business of the exact and the bounds tier)"""
    shape = GOLDEN_SHAPES[shape_index]
    gen = torch.Generator().manual_seed(7100 + shape_index)
    out = {}
    for key in ('x_rgb', 'x_depth'):
        out[key] = torch.round((0.3 + torch.randn(shape, generator=gen)) * 16) / 16
    for key in ('gy_rgb', 'gy_depth'):
        g = torch.round(torch.randn(shape, generator=gen) * 8) / 8
        out[key] = g * (torch.rand(shape, generator=gen) < 0.08)
    return out


class GoldenFile:
    """tests/golden/encoder_fusion.npz: `index` is JSON {record: {field: array key}}; an array that
    several records hold (the inputs of a shape, the fused map of the three 'se-add*' names, a
    handed-through input) is stored once.  A record holds GOLDEN_FIELDS and, for the 'se-add*' names,
    `state` and `grad`: the state dict and the parameter gradients, each as ONE flat array in the order
    and with the shapes of `layouts[str(C)]` = [[state-dict key, shape], ...]."""

    def __init__(self, path):
        self._npz = np.load(path)
        meta = json.loads(bytes(self._npz['index']).decode())
        self.index, self.layouts = meta['records'], meta['layouts']

    def record(self, name):
        """dict field -> float32 torch tensor; the packed ones as `state/<key>` and `grad/<key>`"""
        out = {}
        for field, key in self.index[name].items():
            a = torch.from_numpy(self._npz[key].copy())
            if field not in ('state', 'grad'):
                out[field] = a
                continue
            at = 0
            for pkey, shape in self.layouts[str(out['x_rgb'].shape[1])]:
                n = int(np.prod(shape))
                out[f'{field}/{pkey}'] = a[at:at + n].reshape(shape)
                at += n
            assert at == a.numel()
        return out

    @staticmethod
    def state_dict(record, prefix='state/'):
        return {k[len(prefix):]: v for k, v in record.items() if k.startswith(prefix)}
