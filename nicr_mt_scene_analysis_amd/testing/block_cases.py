"""TEST INFRASTRUCTURE — never imported by the product path.

The shapes and the fixture layout of the residual-block tests, shared by the host tier, the GPU tier and
tools/gen_golden_block.py."""
import json

import numpy as np
import torch

from .. import _lib as L

ACTS = ('relu', 'silu')
NAMES = ('basicblock', 'bottleneck', 'nonbottleneck1d')
EXPANSION = {'basicblock': 1, 'bottleneck': 4, 'nonbottleneck1d': 1}

# ---------------------------------------------------------------------------- GPU-tier shapes
SEGMENT = L.NMSA_BNTAIL_SEGMENT
BATCHES = (2, 3)                        # a plane index must not run into the next image; an odd merge
CHANNELS = (5, 16, 53)                  # B * C * segments no multiple of the four units of a workgroup
WIDE_C, WIDE_HW = 512, (3, 5)
EXACT_HW = (8, 16)
SEG_HW = (3, (SEGMENT + 3) // 3)        # 3 x 683 = 2049 elements: one past a segment, the second holds ONE element
# 1 element; fewer than a wave's lanes; exact; 300, no multiple of 8; several chunks per lane; two segments
PLANES = ((1, 1), (3, 5), EXACT_HW, (15, 20), (30, 40), SEG_HW)
# (B, C, (H, W)) of the bounds tier: every plane at B 2, C 16; the other channel counts and B 3 at two planes
SHAPES = tuple((2, 16, hw) for hw in PLANES) + tuple((b, c, hw) for b, c in ((3, 5), (2, 53), (3, 53))
                                                     for hw in ((3, 5), (15, 20))) + ((2, WIDE_C, WIDE_HW),)

assert SEG_HW[0] * SEG_HW[1] == SEGMENT + 1 and 30 * 40 <= SEGMENT


def vec_width(dtype) -> int:
    """elements of a 16-byte access"""
    return 4 if dtype == torch.float32 else 8


def expected_route(dtype, hw, aligned: bool = True):
    n = hw[0] * hw[1]
    route = L.NMSA_BNTAIL_ROUTE_VECTOR if aligned and n % vec_width(dtype) == 0 else L.NMSA_BNTAIL_ROUTE_ELEMENT
    return route, -(-n // SEGMENT)


# ---------------------------------------------------------------------------- the fixture
GOLDEN_B, GOLDEN_HW, GOLDEN_PLANES = 2, (5, 6), 4
GOLDEN_STRIDE = 2                       # of the records with a downsample branch
GOLDEN_SEED = 9100


def golden_records():
    """(name, act, mode, downsample, dropout_p)"""
    out = []
    for name in NAMES:
        for act in ACTS:
            for mode in ('train', 'eval'):
                for ds in (False, True):
                    for p in ((0.0, 0.2) if name == 'nonbottleneck1d' else (None,)):
                        out.append((name, act, mode, ds, p))
    return out


def record_name(name, act, mode, ds, p) -> str:
    return f"{name}/{act}/{mode}/{'ds' if ds else 'id'}" + ('' if p is None else f'/p{p}')


def golden_channels(name: str, ds: bool):
    """(inplanes, planes, stride): without a downsample branch the block keeps its shape"""
    planes = GOLDEN_PLANES // 2 if name == 'bottleneck' else GOLDEN_PLANES
    return (planes * 2, planes, GOLDEN_STRIDE) if ds else (planes * EXPANSION[name], planes, 1)


def golden_seed(name, act, ds) -> int:
    """one module initialisation per (name, act, downsample): the records of both modes and both dropout
    rates share their parameters, which the fixture stores once"""
    return GOLDEN_SEED + 100 * NAMES.index(name) + 10 * ACTS.index(act) + int(ds)


# input seeds per (name, downsample), chosen on the CPU so that in every record no ReLU of the float64
# restatement comes closer to 0 than 64 times the bound of its segment's own forward arithmetic, nor than the bound
# accumulated from the block's input (tools/gen_golden_block.py and the tests check both)
INPUT_SEEDS = {('basicblock', False): 0, ('basicblock', True): 0, ('bottleneck', False): 2, ('bottleneck', True): 1,
               ('nonbottleneck1d', False): 188, ('nonbottleneck1d', True): 0}


def golden_input(name: str, ds: bool) -> torch.Tensor:
    """seeded float32 input: multiples of 1/8 in about -3..3"""
    inplanes = golden_channels(name, ds)[0]
    gen = torch.Generator().manual_seed(GOLDEN_SEED + INPUT_SEEDS[(name, ds)])
    return torch.round(torch.randn((GOLDEN_B, inplanes) + GOLDEN_HW, generator=gen) * 8) / 8


def golden_gy(shape, name: str, ds: bool) -> torch.Tensor:
    """the fixed upstream gradient: multiples of 1/8 on about one position in three, 0 elsewhere"""
    gen = torch.Generator().manual_seed(GOLDEN_SEED + 50 + 7 * NAMES.index(name) + int(ds))
    g = torch.round(torch.randn(shape, generator=gen) * 8) / 8
    return g * (torch.rand(shape, generator=gen) < 0.35)


def randomise_running_stats(module, seed: int) -> None:
    """coarse seeded running statistics, so that eval mode is no identity: means multiples of 1/8, variances
    multiples of 1/8 in 0.5..1.5"""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for key, buf in module.named_buffers():
            if key.endswith('running_mean'):
                buf.copy_(torch.round(torch.randn(buf.shape, generator=gen) * 4) / 8)
            elif key.endswith('running_var'):
                buf.copy_(0.5 + torch.round(torch.rand(buf.shape, generator=gen) * 8) / 8)


class GoldenFile:
    """tests/golden/block.npz: `index` is JSON {record: {field: array key}}; an array several records hold is
    stored once.  Fields: x, gy, y, gx; `scale` [B, C] (the Dropout2d scale, training records with
    dropout_p > 0); `state`, `state_after`, `grad`: the state dict before the step, its buffers after the step
    and the parameter gradients, each ONE flat float32 array in the order and with the shapes of
    `layouts[<name>/<ds|id>]` = {'state': [[key, shape], ...], 'after': [...], 'grad': [...]}
    (num_batches_tracked as a float32 value)."""

    def __init__(self, path):
        self._npz = np.load(path)
        meta = json.loads(bytes(self._npz['index']).decode())
        self.index, self.layouts = meta['records'], meta['layouts']

    def record(self, name):
        out = {}
        layout = self.layouts['/'.join((name.split('/')[0], name.split('/')[3]))]
        for field, key in self.index[name].items():
            a = torch.from_numpy(self._npz[key].copy())
            if field not in ('state', 'state_after', 'grad'):
                out[field] = a
                continue
            at = 0
            for pkey, shape in layout[{'grad': 'grad', 'state': 'state', 'state_after': 'after'}[field]]:
                n = int(np.prod(shape)) if shape else 1
                out[f'{field}/{pkey}'] = a[at:at + n].reshape(shape)
                at += n
            assert at == a.numel()
        return out

    @staticmethod
    def state_dict(record, prefix='state/'):
        out = {}
        for k, v in record.items():
            if k.startswith(prefix):
                out[k[len(prefix):]] = v.long() if k.endswith('num_batches_tracked') else v
        return out


DROPOUT_SEED = 77                       # tools/gen_golden_block.py seeds the reference's forward pass with it


def build_block(name: str, act: str, ds: bool, p=None):
    """the block of a fixture record from this package's `model` (its parameters come from the record)"""
    from .. import model
    from ..model.activation import get_activation_class
    from ..model.utils import ConvNormAct
    inplanes, planes, stride = golden_channels(name, ds)
    down = ConvNormAct(inplanes, planes * EXPANSION[name], kernel_size=1, stride=stride, activation=None) if ds else None
    kwargs = {} if p is None else {'dropout_p': p}
    return model.get_block_class(name)(inplanes, planes, stride=stride, downsample=down,
                                       activation=get_activation_class(act), **kwargs)


def run_record(module, rec, device=None):
    """y, gx, parameter gradients and buffers of `module` (state loaded from the record) after one step on the
    record's input and upstream gradient, under the record's dropout seed -> dict like `block_ref.block_reference`"""
    x = rec['x'].to(device).requires_grad_(True)
    module.zero_grad(set_to_none=True)
    torch.manual_seed(DROPOUT_SEED)
    y = module(x)
    y.backward(rec['gy'].to(device))
    out = {'y': y.detach(), 'gx': x.grad}
    out.update({f'grad/{k}': v.grad for k, v in module.named_parameters()})
    out.update({f'state/{k}': v for k, v in module.state_dict().items() if 'running' in k or 'num_batches' in k})
    return out
