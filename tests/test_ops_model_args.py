"""What the model ops of `ops.py` refuse, and with which exception: one table over every wrapper from the learned
upsampling to the scene head and their eight route queries.

Every row starts from ONE valid call of an op at its smallest legal shape ([1, 16, 2, 2] maps: 16 channels is
the SE minimum; [1, 2, 2, 16] for the NHWC op; pool sizes (1, 2)), applies the mistakes its second field names,
one `argument:mistake` each, and states the exception type the call ends in, or OK where the wrappers accept
it.  The types are literals, written down from runs of the wrappers as they stood before their argument checks
were gathered into shared helpers; they are never computed from the code under test.  Rows with two mistakes
pin which defect is reported: the device before the dtype, an argument checked earlier before a later one.

The host table builds every tensor on the CPU: what is refused before any device access (a CPU tensor is a
NmsaError, not a TypeError; bad strings; bad pool sizes and branch shapes; the route queries, which only read
shapes, dtypes and addresses).  The device table needs the MI355X; each row is at most one tiny launch.
For the ops that make their inputs contiguous, a channels-last or sliced input must give the bits of its
`.contiguous()` copy.

Found while writing the rows down, and kept as it is (tightening is a change of its own):
`ln_nhwc_to_nchw_backward` compares only the element count of `mean` and `rstd`, so [B, P] passes for [B * P];
`sefuse_route` and `bntail_route` look at the first tensor's dtype alone; `mlpdec_route` takes its `out`
through `L.ptr`, so a pageable host tensor is a ValueError there and not a NmsaError."""
import pytest
import torch

from nicr_mt_scene_analysis_amd import ops
from nicr_mt_scene_analysis_amd._lib import NmsaError

N, T, V, OK = NmsaError, TypeError, ValueError, None
F32 = torch.float32


def _sliced(t):
    buf = t.new_zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],))
    buf[..., ::2] = t
    return buf[..., ::2]


MISTAKES = {
    'cpu': lambda t: t.cpu(),
    'int64': lambda t: t.long(),
    'int32': lambda t: t.int(),
    'float64': lambda t: t.double(),
    'float16': lambda t: t.half(),
    'bfloat16': lambda t: t.bfloat16(),
    'flat': lambda t: t.reshape(-1),                            # wrong rank
    'empty': lambda t: t[:0],
    'wider': lambda t: torch.cat([t, t], -1),                   # same rank, another shape
    'batch2': lambda t: torch.cat([t, t], 0),
    'c8': lambda t: t[:, :8].contiguous(),
    'px1': lambda t: t[..., :1, :1].contiguous(),
    'pairs': lambda t: t.reshape(-1, 2),                        # the same elements under another shape
    'conv': lambda t: t[..., None, None],                       # a 1x1 convolution's weight
    'sliced': _sliced,                                          # same values, not contiguous
    'chlast': lambda t: t.contiguous(memory_format=torch.channels_last),
    'none': lambda t: None,
    'first': lambda v: v[:1],                                   # of a sequence
    'twice': lambda v: v + v,
    'drop': lambda v: v[:0],
}


def valid_call(op, dev):
    """the arguments of one valid call of `op`, tensors on `dev`; '*' holds positional arguments"""
    gen = torch.Generator().manual_seed(7)

    def t(*shape, dtype=F32):
        return torch.randn(shape, generator=gen).to(dtype).to(dev)

    def m():
        return t(1, 16, 2, 2)

    def v():
        return t(16)

    def se(n_each):
        return (t(1, 16), t(1), t(16, 1), t(16)) if n_each == 4 else (t(1, 16), t(16, 1))

    def code():
        return torch.full((1, 16, 1, 1), 4, dtype=torch.uint8, device=dev)

    def bnbwd():
        return dict(gy=m(), x=m(), aux=m(), gamma=v(), beta=v(), mean=v(), invstd=v().abs() + 0.5, act='relu',
                    scale=t(1, 16), part=t(4096))

    shapes2 = ((1, 16, 2, 2), (1, 16, 1, 1))
    calls = {
        'upsample2x_dw3x3': lambda: dict(x=m(), weight=t(16, 1, 3, 3), bias=v(), out=t(1, 16, 4, 4)),
        'upsample2x_dw3x3_backward': lambda: dict(gy=t(1, 16, 4, 4), x=m(), weight=t(16, 1, 3, 3)),
        'upsample2x_dw3x3_route': lambda: dict(x=m(), other=t(1, 16, 4, 4)),
        'ln_nhwc_to_nchw': lambda: dict(x=t(1, 2, 2, 16), gamma=v(), beta=v(), eps=1e-5, add=m(), out=m(),
                                        out_dtype=None),
        'ln_nhwc_to_nchw_backward': lambda: dict(gy=m(), x=t(1, 2, 2, 16), gamma=v(), mean=t(4),
                                                 rstd=t(4).abs() + 0.5),
        'ln_nhwc_to_nchw_route': lambda: dict(x=t(1, 2, 2, 16), y=m()),
        'ppm_pool': lambda: dict(x=m(), sizes=(1, 2)),
        'ppm_pool_backward': lambda: dict(gps=(t(1, 16, 1, 1), m()), x_shape=(1, 16, 2, 2), sizes=(1, 2)),
        'ppm_upsample_concat': lambda: dict(x=m(), ys=(t(1, 4, 1, 1), t(1, 4, 2, 2)), mode='bilinear',
                                            out=t(1, 24, 2, 2)),
        'ppm_upsample_concat_backward': lambda: dict(g_out=t(1, 24, 2, 2), n_channels_x=16,
                                                     branch_shapes=((1, 4, 1, 1), (1, 4, 2, 2)), mode='bilinear',
                                                     need=None),
        'ppm_route': lambda: dict(hw=(2, 2), sizes=(1, 2)),
        'mlpdec_upsample_concat': lambda: dict(ys=(m(), t(1, 16, 1, 1)), mode='bilinear', size=None),
        'mlpdec_upsample_concat_backward': lambda: dict(g_out=t(1, 32, 2, 2), branch_shapes=shapes2,
                                                        mode='bilinear', need=None),
        'mlpdec_route': lambda: dict(ys=(m(), t(1, 16, 1, 1)), out=t(1, 32, 2, 2)),
        'sefuse_squeeze': lambda: dict(x_rgb=m(), x_depth=m(), out=t(2, 1, 16)),
        'sefuse_excite': lambda: dict(s=t(2, 1, 16), params_rgb=se(4), params_depth=se(4), act='relu',
                                      save_z1=True),
        'sefuse_scale_add': lambda: dict(x_rgb=m(), x_depth=m(), w=t(2, 1, 16), out=m()),
        'sefuse_weight_grad': lambda: dict(gy=m(), x_rgb=m(), x_depth=m(), out=t(2, 1, 16)),
        'sefuse_excite_backward': lambda: dict(gw=t(2, 1, 16), w=t(2, 1, 16), z1=t(2, 1, 1), weights_rgb=se(2),
                                               weights_depth=se(2), act='relu'),
        'sefuse_apply_backward': lambda: dict(gy=m(), w=t(2, 1, 16), gs=t(2, 1, 16), need_rgb=True,
                                              need_depth=True, out_rgb=m(), out_depth=m()),
        'sefuse_route': lambda: {'*': [m(), m(), m()]},
        'bntail_stats': lambda: dict(x=m(), part=t(4096)),
        'bntail_apply': lambda: dict(x=m(), gamma=v(), beta=v(), running_mean=v(), running_var=v().abs() + 0.5,
                                     eps=1e-5, momentum=0.1, act='relu', part=t(4096), identity=m(),
                                     scale=t(1, 16), save=True, out=m()),
        'bntail_backward_reduce': lambda: dict(bnbwd(), finish=False),
        'bntail_backward_apply': lambda: dict(bnbwd(), need_x=True, need_identity=True, need_params=True,
                                              out_x=m(), out_identity=m()),
        'bntail_route': lambda: {'*': [m(), m(), m()]},
        'maxpool3x3s2': lambda: dict(x=m(), need_code=True, out=t(1, 16, 1, 1)),
        'maxpool3x3s2_backward': lambda: dict(gy=t(1, 16, 1, 1), code=code(), input_hw=(2, 2), out=m()),
        'maxpool3x3s2_route': lambda: {'*': [m(), t(1, 16, 1, 1), code()]},
        'scene_head': lambda: dict(x=m(), weight=t(3, 16), bias=t(3), need_pooled=True, out_dtype=None),
        'scene_head_backward': lambda: dict(g=t(1, 3), pooled=t(1, 16), weight=t(3, 16), x_shape=(1, 16, 2, 2),
                                            x_dtype=F32, need=(True, True, True)),
        'scene_head_route': lambda: dict(x=m(), n_classes=3),
        '_ppm_sizes': lambda: dict(sizes=(1, (2, 3))),
        '_mlpdec_shifts': lambda: dict(shapes=shapes2, size=None),
    }
    return calls[op]()


def _edit(args, path, fn):
    keys = [int(k) if k.isdigit() else k for k in path.split('.')]
    if len(keys) == 1:
        args[keys[0]] = fn(args[keys[0]])
    else:
        seq = list(args[keys[0]])
        seq[keys[1]] = fn(seq[keys[1]])
        args[keys[0]] = type(args[keys[0]])(seq)


def call(op, dev, spec='', override=None):
    args = valid_call(op, dev)
    for item in spec.split():
        path, mistake = item.split(':')
        _edit(args, path, MISTAKES[mistake])
    args.update(override or {})
    return getattr(ops, op)(*args.pop('*', ()), **args)


# (op, mistakes, what the call ends in[, arguments replaced outright]) with every tensor on the CPU
HOST = [
    # a CPU tensor is a NmsaError, whatever else is wrong with it or with a later argument
    ('upsample2x_dw3x3', '', N), ('upsample2x_dw3x3', 'x:int64', N), ('upsample2x_dw3x3', 'x:flat', N),
    ('upsample2x_dw3x3_backward', '', N), ('upsample2x_dw3x3_backward', 'gy:wider', N),
    ('ln_nhwc_to_nchw', '', N), ('ln_nhwc_to_nchw', 'x:float64', N, {'out_dtype': torch.float64}),
    ('ln_nhwc_to_nchw_backward', '', N),
    ('ppm_pool', '', N), ('ppm_pool', '', N, {'sizes': (0,)}), ('ppm_pool', 'x:int64', N),
    ('ppm_pool_backward', '', N), ('ppm_pool_backward', '', V, {'sizes': (0,)}),
    ('ppm_pool_backward', 'gps:first', T), ('ppm_pool_backward', 'gps.0:none gps.1:none', T),
    ('ppm_upsample_concat', '', N), ('ppm_upsample_concat', '', N, {'mode': 'cubic'}),
    ('ppm_upsample_concat_backward', '', N), ('ppm_upsample_concat_backward', '', N, {'mode': 'cubic'}),
    ('mlpdec_upsample_concat', '', N), ('mlpdec_upsample_concat', '', V, {'mode': 'cubic'}),
    ('mlpdec_upsample_concat', 'ys.0:flat', N), ('mlpdec_upsample_concat', 'ys:drop', V),
    ('mlpdec_upsample_concat_backward', '', N), ('mlpdec_upsample_concat_backward', '', N, {'mode': 'cubic'}),
    ('sefuse_squeeze', '', N), ('sefuse_squeeze', 'x_rgb:c8 x_depth:c8', N),
    ('sefuse_excite', '', N), ('sefuse_excite', '', V, {'act': 'tanh'}), ('sefuse_excite', 's:float16', N),
    ('sefuse_scale_add', '', N), ('sefuse_weight_grad', '', N),
    ('sefuse_excite_backward', '', N), ('sefuse_excite_backward', '', V, {'act': 'tanh'}),
    ('sefuse_apply_backward', '', N),
    ('bntail_stats', '', N), ('bntail_stats', 'x:sliced', N),
    ('bntail_apply', '', N), ('bntail_apply', '', V, {'act': 'tanh'}),
    ('bntail_backward_reduce', '', N), ('bntail_backward_reduce', '', V, {'act': 'tanh'}),
    ('bntail_backward_apply', '', N), ('bntail_backward_apply', '', V, {'act': 'tanh'}),
    ('maxpool3x3s2', '', N), ('maxpool3x3s2', 'x:sliced', N),
    ('maxpool3x3s2_backward', '', N), ('maxpool3x3s2_backward', 'code:int32', N),
    ('scene_head', '', N), ('scene_head', 'weight:float16', N, {'out_dtype': torch.float64}),
    ('scene_head_backward', '', N), ('scene_head_backward', 'g:int64', N),
    # the route queries read shapes, dtypes and addresses only: host tensors will do
    ('upsample2x_dw3x3_route', '', OK), ('upsample2x_dw3x3_route', 'x:flat', V),
    ('upsample2x_dw3x3_route', 'x:int64', T), ('upsample2x_dw3x3_route', 'x:flat x:int64', V),
    ('upsample2x_dw3x3_route', 'x:empty', N), ('upsample2x_dw3x3_route', 'x:bfloat16', OK),
    ('ln_nhwc_to_nchw_route', '', OK), ('ln_nhwc_to_nchw_route', 'x:flat', V),
    ('ln_nhwc_to_nchw_route', 'x:int64', T), ('ln_nhwc_to_nchw_route', 'y:float64', T),
    ('ln_nhwc_to_nchw_route', 'x:flat y:int64', V), ('ln_nhwc_to_nchw_route', 'x:empty', N),
    ('ppm_route', '', OK), ('ppm_route', '', V, {'sizes': (0,)}), ('ppm_route', '', V, {'sizes': ()}),
    ('ppm_route', '', V, {'sizes': (1, 2, 3, 4, 5)}), ('ppm_route', '', N, {'hw': (0, 2)}),
    ('mlpdec_route', '', V), ('mlpdec_route', 'ys.0:flat', V), ('mlpdec_route', 'ys:drop', V),
    ('sefuse_route', '', OK), ('sefuse_route', '*.0:flat', V), ('sefuse_route', '*.2:flat', V),
    ('sefuse_route', '*:drop', V), ('sefuse_route', '*:twice', V), ('sefuse_route', '*.0:int64', T),
    ('sefuse_route', '*.1:int64', OK), ('sefuse_route', '*.0:flat *.0:int64', V),
    ('bntail_route', '', OK), ('bntail_route', '*.0:flat', V), ('bntail_route', '*:drop', V),
    ('bntail_route', '*:twice', V), ('bntail_route', '*.0:float64', T), ('bntail_route', '*.1:int64', OK),
    ('maxpool3x3s2_route', '', OK), ('maxpool3x3s2_route', '*.0:flat', V), ('maxpool3x3s2_route', '*:first', V),
    ('maxpool3x3s2_route', '*.0:int64', T), ('maxpool3x3s2_route', '*.0:empty', N),
    ('scene_head_route', '', OK), ('scene_head_route', 'x:flat', V), ('scene_head_route', 'x:int64', T),
    ('scene_head_route', 'x:flat x:int64', V), ('scene_head_route', 'x:empty', N),
    ('scene_head_route', '', N, {'n_classes': 0}),
    # the two shape helpers the model layer imports
    ('_ppm_sizes', '', OK), ('_ppm_sizes', '', V, {'sizes': (0,)}), ('_ppm_sizes', '', V, {'sizes': ((2, 0),)}),
    ('_ppm_sizes', '', V, {'sizes': ()}), ('_ppm_sizes', '', V, {'sizes': (1, 2, 3, 4, 5)}),
    ('_mlpdec_shifts', '', OK), ('_mlpdec_shifts', 'shapes:drop', V),
    ('_mlpdec_shifts', '', V, {'shapes': ((1, 1, 1, 1),) * 5}), ('_mlpdec_shifts', '', V, {'shapes': ((16, 2, 2),)}),
    ('_mlpdec_shifts', '', V, {'shapes': ((1, 16, 0, 2),)}),
    ('_mlpdec_shifts', '', V, {'shapes': ((1, 16, 3, 3), (1, 16, 2, 2))}),          # no whole factor
    ('_mlpdec_shifts', '', V, {'shapes': ((1, 16, 4, 4), (1, 16, 2, 1))}),          # 2 along H, 4 along W
    ('_mlpdec_shifts', '', V, {'shapes': ((1, 16, 3, 3), (1, 16, 1, 1))}),          # 3: no power of two
    ('_mlpdec_shifts', '', V, {'shapes': ((1, 16, 32, 32), (1, 16, 1, 1))}),        # 32: above 16
    ('_mlpdec_shifts', '', V, {'size': (3, 3)}),
]

# the same with every tensor on the device, the mistaken one apart
DEVICE = [
    # learned upsampling: a wrong rank or an empty x is a ValueError here, a TypeError in the other ops
    ('upsample2x_dw3x3', 'x:cpu', N), ('upsample2x_dw3x3', 'weight:cpu', N), ('upsample2x_dw3x3', 'bias:cpu', N),
    ('upsample2x_dw3x3', 'out:cpu', N), ('upsample2x_dw3x3', 'x:int64', T), ('upsample2x_dw3x3', 'x:float64', T),
    ('upsample2x_dw3x3', 'x:flat', V), ('upsample2x_dw3x3', 'x:empty', V), ('upsample2x_dw3x3', 'x:int64 x:cpu', N),
    ('upsample2x_dw3x3', 'x:int64 x:flat', T), ('upsample2x_dw3x3', 'x:flat weight:cpu', V),
    ('upsample2x_dw3x3', 'weight:float16', T), ('upsample2x_dw3x3', 'weight:wider', T),
    ('upsample2x_dw3x3', 'weight:flat', T), ('upsample2x_dw3x3', 'bias:bfloat16', T),
    ('upsample2x_dw3x3', 'bias:wider', T), ('upsample2x_dw3x3', 'weight:float16 bias:cpu', T),
    ('upsample2x_dw3x3', 'out:wider', T), ('upsample2x_dw3x3', 'out:sliced', T),
    ('upsample2x_dw3x3', 'out:bfloat16', T), ('upsample2x_dw3x3', 'bias:none', OK),
    ('upsample2x_dw3x3_backward', 'gy:cpu', N), ('upsample2x_dw3x3_backward', 'x:cpu', N),
    ('upsample2x_dw3x3_backward', 'weight:cpu', N), ('upsample2x_dw3x3_backward', 'x:int64', T),
    ('upsample2x_dw3x3_backward', 'x:flat', V), ('upsample2x_dw3x3_backward', 'x:empty', V),
    ('upsample2x_dw3x3_backward', 'gy:bfloat16', T), ('upsample2x_dw3x3_backward', 'gy:int64', T),
    ('upsample2x_dw3x3_backward', 'gy:wider', T), ('upsample2x_dw3x3_backward', 'gy:flat', T),
    ('upsample2x_dw3x3_backward', 'weight:float16', T), ('upsample2x_dw3x3_backward', 'gy:cpu x:int64', T),
    ('upsample2x_dw3x3_backward', 'gy:cpu gy:wider', N),
    # Swin fusion
    ('ln_nhwc_to_nchw', 'x:cpu', N), ('ln_nhwc_to_nchw', 'gamma:cpu', N), ('ln_nhwc_to_nchw', 'beta:cpu', N),
    ('ln_nhwc_to_nchw', 'add:cpu', N), ('ln_nhwc_to_nchw', 'out:cpu', N), ('ln_nhwc_to_nchw', 'x:int64', T),
    ('ln_nhwc_to_nchw', 'x:float64', T), ('ln_nhwc_to_nchw', 'x:flat', V), ('ln_nhwc_to_nchw', 'x:empty', V),
    ('ln_nhwc_to_nchw', 'x:cpu x:int64', N), ('ln_nhwc_to_nchw', 'x:flat gamma:float16', V),
    ('ln_nhwc_to_nchw', 'gamma:float16', T), ('ln_nhwc_to_nchw', 'gamma:wider', T),
    ('ln_nhwc_to_nchw', 'beta:bfloat16', T), ('ln_nhwc_to_nchw', 'beta:wider', T),
    ('ln_nhwc_to_nchw', '', T, {'out_dtype': torch.float64}), ('ln_nhwc_to_nchw', '', T, {'out_dtype': torch.bfloat16}),
    ('ln_nhwc_to_nchw', 'add:cpu', T, {'out_dtype': torch.float64}),
    ('ln_nhwc_to_nchw', 'add:bfloat16', T), ('ln_nhwc_to_nchw', 'add:wider', T), ('ln_nhwc_to_nchw', 'add:flat', T),
    ('ln_nhwc_to_nchw', 'out:bfloat16', T), ('ln_nhwc_to_nchw', 'out:wider', T), ('ln_nhwc_to_nchw', 'out:sliced', T),
    ('ln_nhwc_to_nchw', 'add:none out:none', OK),
    ('ln_nhwc_to_nchw', 'x:bfloat16', OK, {'out_dtype': F32}),
    ('ln_nhwc_to_nchw_backward', 'gy:cpu', N), ('ln_nhwc_to_nchw_backward', 'x:cpu', N),
    ('ln_nhwc_to_nchw_backward', 'gamma:cpu', N), ('ln_nhwc_to_nchw_backward', 'mean:cpu', N),
    ('ln_nhwc_to_nchw_backward', 'rstd:cpu', N), ('ln_nhwc_to_nchw_backward', 'x:int64', T),
    ('ln_nhwc_to_nchw_backward', 'x:flat', V), ('ln_nhwc_to_nchw_backward', 'x:empty', V),
    ('ln_nhwc_to_nchw_backward', 'gy:float64', T), ('ln_nhwc_to_nchw_backward', 'gy:bfloat16', T),
    ('ln_nhwc_to_nchw_backward', 'gy:wider', T), ('ln_nhwc_to_nchw_backward', 'gamma:float16', T),
    ('ln_nhwc_to_nchw_backward', 'mean:float16', T), ('ln_nhwc_to_nchw_backward', 'mean:wider', T),
    ('ln_nhwc_to_nchw_backward', 'rstd:float64', T), ('ln_nhwc_to_nchw_backward', 'rstd:wider', T),
    ('ln_nhwc_to_nchw_backward', 'gy:wider mean:cpu', T), ('ln_nhwc_to_nchw_backward', 'mean:float16 rstd:cpu', T),
    ('ln_nhwc_to_nchw_backward', 'x:bfloat16', OK),             # a float32 gy for a bfloat16 x
    ('ln_nhwc_to_nchw_backward', 'mean:pairs rstd:pairs', OK),  # only the element count is compared
    # context module
    ('ppm_pool', 'x:cpu', N), ('ppm_pool', 'x:int64', T), ('ppm_pool', 'x:float64', T), ('ppm_pool', 'x:flat', T),
    ('ppm_pool', 'x:empty', T), ('ppm_pool', 'x:int64 x:flat', T), ('ppm_pool', 'x:flat', T, {'sizes': (0,)}),
    ('ppm_pool', '', V, {'sizes': (0,)}), ('ppm_pool', '', V, {'sizes': (1, 2, 3, 4, 5)}),
    ('ppm_pool_backward', 'gps.0:cpu', N), ('ppm_pool_backward', 'gps.1:cpu', N),
    ('ppm_pool_backward', 'gps.0:int64', T), ('ppm_pool_backward', 'gps.0:flat', T),
    ('ppm_pool_backward', 'gps.0:empty', T), ('ppm_pool_backward', 'gps.0:wider', T),
    ('ppm_pool_backward', 'gps.1:bfloat16', T), ('ppm_pool_backward', 'gps.1:wider', T),
    ('ppm_pool_backward', 'gps.1:flat', T), ('ppm_pool_backward', 'gps.0:int64 gps.1:cpu', T),
    ('ppm_pool_backward', 'gps.0:none', OK), ('ppm_pool_backward', 'gps.0:none gps.1:wider', T),
    ('ppm_upsample_concat', 'x:cpu', N), ('ppm_upsample_concat', 'ys.0:cpu', N), ('ppm_upsample_concat', 'ys.1:cpu', N),
    ('ppm_upsample_concat', 'out:cpu', N), ('ppm_upsample_concat', 'x:int64', T), ('ppm_upsample_concat', 'x:flat', T),
    ('ppm_upsample_concat', 'x:empty', T), ('ppm_upsample_concat', '', V, {'mode': 'cubic'}),
    ('ppm_upsample_concat', 'x:flat', T, {'mode': 'cubic'}), ('ppm_upsample_concat', 'ys.0:cpu', V, {'mode': 'cubic'}),
    ('ppm_upsample_concat', 'ys:drop', V), ('ppm_upsample_concat', 'ys:twice ys:twice', V),
    ('ppm_upsample_concat', 'ys.1:bfloat16', T), ('ppm_upsample_concat', 'ys.1:flat', T),
    ('ppm_upsample_concat', 'ys.1:empty', T), ('ppm_upsample_concat', 'ys.0:batch2', T),
    ('ppm_upsample_concat', 'out:wider', T), ('ppm_upsample_concat', 'out:sliced', T),
    ('ppm_upsample_concat', 'out:float16', T), ('ppm_upsample_concat', 'ys.1:wider', OK),
    ('ppm_upsample_concat_backward', 'g_out:cpu', N), ('ppm_upsample_concat_backward', 'g_out:int64', T),
    ('ppm_upsample_concat_backward', 'g_out:flat', T), ('ppm_upsample_concat_backward', 'g_out:empty', T),
    ('ppm_upsample_concat_backward', '', V, {'mode': 'cubic'}),
    ('ppm_upsample_concat_backward', 'branch_shapes:drop', V),
    ('ppm_upsample_concat_backward', '', T, {'n_channels_x': 15}),
    ('ppm_upsample_concat_backward', '', T, {'need': (True,)}),
    ('ppm_upsample_concat_backward', '', T, {'branch_shapes': ((2, 4, 1, 1), (1, 4, 2, 2))}),
    ('ppm_upsample_concat_backward', '', V, {'mode': 'cubic', 'n_channels_x': 15}),
    # MLP decoders: the branch shapes are looked at before the first branch's dtype
    ('mlpdec_upsample_concat', 'ys.0:cpu', N), ('mlpdec_upsample_concat', 'ys.1:cpu', N),
    ('mlpdec_upsample_concat', 'ys.0:int64', T), ('mlpdec_upsample_concat', 'ys.0:float64', T),
    ('mlpdec_upsample_concat', 'ys.0:flat', V), ('mlpdec_upsample_concat', 'ys.0:empty', V),
    ('mlpdec_upsample_concat', 'ys.0:int64 ys.0:flat', V), ('mlpdec_upsample_concat', 'ys.1:bfloat16', T),
    ('mlpdec_upsample_concat', 'ys.1:int64', T), ('mlpdec_upsample_concat', 'ys.1:batch2', T),
    ('mlpdec_upsample_concat', 'ys.1:cpu', V, {'mode': 'cubic'}), ('mlpdec_upsample_concat', '', V, {'mode': 'cubic'}),
    ('mlpdec_upsample_concat', '', V, {'size': (3, 3)}), ('mlpdec_upsample_concat', 'ys:drop', V),
    ('mlpdec_upsample_concat_backward', 'g_out:cpu', N), ('mlpdec_upsample_concat_backward', 'g_out:int64', T),
    ('mlpdec_upsample_concat_backward', 'g_out:flat', T), ('mlpdec_upsample_concat_backward', 'g_out:empty', T),
    ('mlpdec_upsample_concat_backward', '', V, {'mode': 'cubic'}),
    ('mlpdec_upsample_concat_backward', 'branch_shapes:drop', V),
    ('mlpdec_upsample_concat_backward', 'branch_shapes:first', T),
    ('mlpdec_upsample_concat_backward', '', T, {'need': (True,)}),
    ('mlpdec_upsample_concat_backward', '', T, {'branch_shapes': ((2, 16, 2, 2), (1, 16, 1, 1))}),
    ('mlpdec_upsample_concat_backward', '', V, {'branch_shapes': ((1, 16, 3, 3), (1, 16, 1, 1))}),
    ('mlpdec_route', '', OK), ('mlpdec_route', 'out:int64', T), ('mlpdec_route', 'ys.0:flat', V),
    ('mlpdec_route', 'ys.0:flat out:int64', V), ('mlpdec_route', 'out:cpu', V),
    # SE fusion: 16 channels at least (ValueError), asked after the first map's own checks
    ('sefuse_squeeze', 'x_rgb:cpu', N), ('sefuse_squeeze', 'x_depth:cpu', N), ('sefuse_squeeze', 'out:cpu', N),
    ('sefuse_squeeze', 'x_rgb:int64', T), ('sefuse_squeeze', 'x_rgb:float64', T), ('sefuse_squeeze', 'x_rgb:flat', T),
    ('sefuse_squeeze', 'x_rgb:empty', T), ('sefuse_squeeze', 'x_rgb:c8 x_depth:c8', V),
    ('sefuse_squeeze', 'x_rgb:c8 x_depth:cpu', V), ('sefuse_squeeze', 'x_rgb:c8 x_rgb:int64', T),
    ('sefuse_squeeze', 'x_depth:bfloat16', T), ('sefuse_squeeze', 'x_depth:wider', T),
    ('sefuse_squeeze', 'x_depth:flat', T), ('sefuse_squeeze', 'x_depth:cpu x_depth:int64', N),
    ('sefuse_squeeze', 'out:wider', T), ('sefuse_squeeze', 'out:bfloat16', T), ('sefuse_squeeze', 'out:sliced', T),
    ('sefuse_squeeze', 'x_depth:wider out:cpu', T),
    ('sefuse_excite', 's:cpu', N), ('sefuse_excite', 's:float16', T), ('sefuse_excite', 's:flat', T),
    ('sefuse_excite', 's:empty', T), ('sefuse_excite', 's:batch2', T), ('sefuse_excite', 's:cpu', V, {'act': 'tanh'}),
    ('sefuse_excite', '', V, {'s': torch.zeros(2, 1, 8)}), ('sefuse_excite', 'params_rgb.0:cpu', N),
    ('sefuse_excite', 'params_depth.3:cpu', N), ('sefuse_excite', 'params_rgb.0:float16', T),
    ('sefuse_excite', 'params_rgb.0:wider', T), ('sefuse_excite', 'params_depth.2:bfloat16', T),
    ('sefuse_excite', 'params_rgb:first', T), ('sefuse_excite', '', T, {'params_rgb': None}),
    ('sefuse_excite', '', T, {'params_depth': None}), ('sefuse_excite', 'params_rgb.0:conv params_rgb.2:conv', OK),
    ('sefuse_scale_add', 'x_rgb:cpu', N), ('sefuse_scale_add', 'x_depth:cpu', N), ('sefuse_scale_add', 'w:cpu', N),
    ('sefuse_scale_add', 'out:cpu', N), ('sefuse_scale_add', 'x_rgb:int64', T), ('sefuse_scale_add', 'x_depth:wider', T),
    ('sefuse_scale_add', 'w:float16', T), ('sefuse_scale_add', 'w:wider', T), ('sefuse_scale_add', 'w:flat', T),
    ('sefuse_scale_add', 'out:wider', T), ('sefuse_scale_add', 'out:sliced', T), ('sefuse_scale_add', 'out:bfloat16', T),
    ('sefuse_scale_add', 'w:float16 out:cpu', T),
    ('sefuse_weight_grad', 'gy:cpu', N), ('sefuse_weight_grad', 'x_rgb:cpu', N), ('sefuse_weight_grad', 'x_depth:cpu', N),
    ('sefuse_weight_grad', 'gy:int64', T), ('sefuse_weight_grad', 'gy:flat', T), ('sefuse_weight_grad', 'gy:c8', V),
    ('sefuse_weight_grad', 'x_rgb:bfloat16', T), ('sefuse_weight_grad', 'x_depth:wider', T),
    ('sefuse_weight_grad', 'out:wider', T), ('sefuse_weight_grad', 'out:float16', T),
    ('sefuse_weight_grad', 'x_rgb:none', OK), ('sefuse_weight_grad', 'x_rgb:none out:none', OK),
    ('sefuse_excite_backward', 'gw:cpu', N), ('sefuse_excite_backward', 'w:cpu', N), ('sefuse_excite_backward', 'z1:cpu', N),
    ('sefuse_excite_backward', 'gw:float16', T), ('sefuse_excite_backward', 'gw:flat', T),
    ('sefuse_excite_backward', 'gw:empty', T), ('sefuse_excite_backward', 'w:float64', T),
    ('sefuse_excite_backward', 'w:wider', T), ('sefuse_excite_backward', 'z1:wider', T),
    ('sefuse_excite_backward', 'z1:bfloat16', T), ('sefuse_excite_backward', 'gw:cpu', V, {'act': 'tanh'}),
    ('sefuse_excite_backward', 'weights_rgb.0:cpu', N), ('sefuse_excite_backward', 'weights_rgb.0:float16', T),
    ('sefuse_excite_backward', 'weights_depth.1:wider', T), ('sefuse_excite_backward', 'weights_rgb:first', T),
    ('sefuse_excite_backward', '', OK, {'weights_rgb': None}),
    ('sefuse_apply_backward', 'gy:cpu', N), ('sefuse_apply_backward', 'w:cpu', N), ('sefuse_apply_backward', 'gs:cpu', N),
    ('sefuse_apply_backward', 'out_rgb:cpu', N), ('sefuse_apply_backward', 'gy:int64', T),
    ('sefuse_apply_backward', 'gy:flat', T), ('sefuse_apply_backward', 'gy:c8', V),
    ('sefuse_apply_backward', 'w:float16', T), ('sefuse_apply_backward', 'gs:wider', T),
    ('sefuse_apply_backward', 'out_rgb:wider', T), ('sefuse_apply_backward', 'out_depth:sliced', T),
    ('sefuse_apply_backward', 'out_depth:bfloat16', T),
    ('sefuse_apply_backward', 'out_rgb:wider', OK, {'need_rgb': False}),
    # batch-norm tail: every map and vector must be dense as it is given
    ('bntail_stats', 'x:cpu', N), ('bntail_stats', 'x:int64', T), ('bntail_stats', 'x:float64', T),
    ('bntail_stats', 'x:flat', T), ('bntail_stats', 'x:empty', T), ('bntail_stats', 'x:sliced', T),
    ('bntail_stats', 'x:chlast', T), ('bntail_stats', 'part:cpu', N), ('bntail_stats', 'part:float16', T),
    ('bntail_stats', 'part:empty', T), ('bntail_stats', 'part:sliced', T), ('bntail_stats', 'part:none', OK),
    ('bntail_apply', 'x:cpu', N), ('bntail_apply', 'identity:cpu', N), ('bntail_apply', 'scale:cpu', N),
    ('bntail_apply', 'gamma:cpu', N), ('bntail_apply', 'running_var:cpu', N), ('bntail_apply', 'out:cpu', N),
    ('bntail_apply', 'part:cpu', N), ('bntail_apply', 'x:int64', T), ('bntail_apply', 'x:flat', T),
    ('bntail_apply', 'x:sliced', T), ('bntail_apply', 'x:cpu', V, {'act': 'tanh'}),
    ('bntail_apply', 'identity:bfloat16', T), ('bntail_apply', 'identity:wider', T),
    ('bntail_apply', 'identity:sliced', T), ('bntail_apply', 'x:px1 identity:none', V),
    ('bntail_apply', 'x:px1 identity:none part:none out:none', OK),     # eval takes one value per channel
    ('bntail_apply', 'x:px1', T), ('bntail_apply', 'scale:bfloat16', T), ('bntail_apply', 'scale:wider', T),
    ('bntail_apply', 'scale:conv', OK), ('bntail_apply', 'gamma:float16', T), ('bntail_apply', 'gamma:wider', T),
    ('bntail_apply', 'beta:sliced', T), ('bntail_apply', 'running_mean:float64', T),
    ('bntail_apply', 'scale:cpu gamma:float16', N), ('bntail_apply', 'gamma:float16 beta:cpu', T),
    ('bntail_apply', 'out:wider', T), ('bntail_apply', 'out:sliced', T), ('bntail_apply', 'out:bfloat16', T),
    ('bntail_apply', 'part:float16', T), ('bntail_apply', 'part:empty', T), ('bntail_apply', 'out:wider part:cpu', T),
    ('bntail_apply', 'part:none identity:none scale:none out:none', OK),
    ('bntail_backward_reduce', 'gy:cpu', N), ('bntail_backward_reduce', 'x:cpu', N), ('bntail_backward_reduce', 'aux:cpu', N),
    ('bntail_backward_reduce', 'mean:cpu', N), ('bntail_backward_reduce', 'scale:cpu', N),
    ('bntail_backward_reduce', 'part:cpu', N), ('bntail_backward_reduce', 'gy:int64', T),
    ('bntail_backward_reduce', 'gy:flat', T), ('bntail_backward_reduce', 'gy:sliced', T),
    ('bntail_backward_reduce', 'x:bfloat16', T), ('bntail_backward_reduce', 'x:wider', T),
    ('bntail_backward_reduce', 'x:sliced', T), ('bntail_backward_reduce', 'aux:chlast', T),
    ('bntail_backward_reduce', 'x:none', T), ('bntail_backward_reduce', 'aux:none', T),
    ('bntail_backward_reduce', 'aux:none', OK, {'act': 'silu'}), ('bntail_backward_reduce', 'beta:none', OK),
    ('bntail_backward_reduce', 'gamma:float16', T), ('bntail_backward_reduce', 'mean:wider', T),
    ('bntail_backward_reduce', 'invstd:sliced', T), ('bntail_backward_reduce', 'scale:bfloat16', T),
    ('bntail_backward_reduce', 'scale:cpu mean:float16', T), ('bntail_backward_reduce', 'part:empty', T),
    ('bntail_backward_reduce', 'part:none', OK, {'finish': True}),
    ('bntail_backward_apply', 'gy:cpu', N), ('bntail_backward_apply', 'out_x:cpu', N),
    ('bntail_backward_apply', 'gy:sliced', T), ('bntail_backward_apply', 'aux:wider', T),
    ('bntail_backward_apply', 'part:none', V), ('bntail_backward_apply', 'part:none out_x:wider', V),
    ('bntail_backward_apply', 'part:none', OK, {'need_params': False}), ('bntail_backward_apply', 'part:float16', T),
    ('bntail_backward_apply', 'out_x:wider', T), ('bntail_backward_apply', 'out_x:sliced', T),
    ('bntail_backward_apply', 'out_identity:bfloat16', T),
    ('bntail_backward_apply', 'out_identity:wider', OK, {'need_identity': False}),
    # stem max pool
    ('maxpool3x3s2', 'x:cpu', N), ('maxpool3x3s2', 'out:cpu', N), ('maxpool3x3s2', 'x:int64', T),
    ('maxpool3x3s2', 'x:float64', T), ('maxpool3x3s2', 'x:flat', T), ('maxpool3x3s2', 'x:empty', T),
    ('maxpool3x3s2', 'x:sliced', T), ('maxpool3x3s2', 'x:chlast', T), ('maxpool3x3s2', 'x:cpu x:int64', N),
    ('maxpool3x3s2', 'out:wider', T), ('maxpool3x3s2', 'out:sliced', T), ('maxpool3x3s2', 'out:bfloat16', T),
    ('maxpool3x3s2_backward', 'gy:cpu', N), ('maxpool3x3s2_backward', 'code:cpu', N),
    ('maxpool3x3s2_backward', 'out:cpu', N), ('maxpool3x3s2_backward', 'gy:int64', T),
    ('maxpool3x3s2_backward', 'gy:flat', T), ('maxpool3x3s2_backward', 'gy:sliced', T),
    ('maxpool3x3s2_backward', 'gy:wider', T), ('maxpool3x3s2_backward', 'code:int32', T),
    ('maxpool3x3s2_backward', 'code:wider', T), ('maxpool3x3s2_backward', 'code:sliced', T),
    ('maxpool3x3s2_backward', 'gy:wider code:cpu', N), ('maxpool3x3s2_backward', '', T, {'input_hw': (4, 4)}),
    ('maxpool3x3s2_backward', 'out:wider', T), ('maxpool3x3s2_backward', 'out:bfloat16', T),
    # scene head
    ('scene_head', 'x:cpu', N), ('scene_head', 'weight:cpu', N), ('scene_head', 'bias:cpu', N),
    ('scene_head', 'x:int64', T), ('scene_head', 'x:flat', T), ('scene_head', 'x:empty', T),
    ('scene_head', 'x:sliced', T), ('scene_head', 'x:chlast', T), ('scene_head', 'weight:float16', T),
    ('scene_head', 'weight:wider', T), ('scene_head', 'weight:flat', T), ('scene_head', 'weight:sliced', T),
    ('scene_head', 'bias:bfloat16', T), ('scene_head', 'bias:wider', T), ('scene_head', 'bias:sliced', T),
    ('scene_head', 'weight:float16 bias:cpu', T), ('scene_head', '', T, {'out_dtype': torch.float64}),
    ('scene_head', '', T, {'out_dtype': torch.int64}), ('scene_head', 'bias:none', OK, {'out_dtype': torch.bfloat16}),
    ('scene_head_backward', 'g:cpu', N), ('scene_head_backward', 'pooled:cpu', N), ('scene_head_backward', 'weight:cpu', N),
    ('scene_head_backward', 'g:int64', T), ('scene_head_backward', 'g:float64', T),
    ('scene_head_backward', '', T, {'x_dtype': torch.float64}), ('scene_head_backward', '', T, {'x_dtype': torch.int64}),
    ('scene_head_backward', 'g:cpu weight:float16', N), ('scene_head_backward', 'g:wider pooled:cpu', N),
    ('scene_head_backward', 'g:flat', T), ('scene_head_backward', 'g:wider', T), ('scene_head_backward', 'g:sliced', T),
    ('scene_head_backward', 'weight:float16', T), ('scene_head_backward', 'weight:sliced', T),
    ('scene_head_backward', 'pooled:float16', T), ('scene_head_backward', 'pooled:wider', T),
    ('scene_head_backward', 'pooled:sliced', T), ('scene_head_backward', '', T, {'x_shape': (1, 16, 0, 2)}),
    ('scene_head_backward', 'g:bfloat16', OK, {'x_dtype': torch.float16}),
]

# what the ops that make their inputs contiguous take in any layout
LAYOUTS = [
    ('upsample2x_dw3x3', 'x:chlast'), ('upsample2x_dw3x3', 'x:sliced'), ('upsample2x_dw3x3', 'weight:sliced bias:sliced'),
    ('upsample2x_dw3x3_backward', 'gy:chlast x:chlast'), ('upsample2x_dw3x3_backward', 'gy:sliced x:sliced weight:sliced'),
    ('ln_nhwc_to_nchw', 'x:sliced gamma:sliced beta:sliced'), ('ln_nhwc_to_nchw', 'x:chlast add:chlast'),
    ('ln_nhwc_to_nchw', 'add:sliced'),
    ('ln_nhwc_to_nchw_backward', 'gy:chlast x:sliced'), ('ln_nhwc_to_nchw_backward', 'gy:sliced gamma:sliced'),
    ('ln_nhwc_to_nchw_backward', 'mean:sliced rstd:sliced'),
    ('ppm_pool', 'x:chlast'), ('ppm_pool', 'x:sliced'), ('ppm_pool_backward', 'gps.0:sliced gps.1:chlast'),
    ('ppm_pool_backward', 'gps.1:sliced'),
    ('ppm_upsample_concat', 'x:chlast ys.1:chlast'), ('ppm_upsample_concat', 'x:sliced ys.0:sliced ys.1:sliced'),
    ('ppm_upsample_concat_backward', 'g_out:chlast'), ('ppm_upsample_concat_backward', 'g_out:sliced'),
    ('mlpdec_upsample_concat', 'ys.0:chlast'), ('mlpdec_upsample_concat', 'ys.0:sliced ys.1:sliced'),
    ('mlpdec_upsample_concat_backward', 'g_out:chlast'), ('mlpdec_upsample_concat_backward', 'g_out:sliced'),
    ('sefuse_squeeze', 'x_rgb:chlast x_depth:sliced'), ('sefuse_squeeze', 'x_rgb:sliced x_depth:chlast'),
    ('sefuse_excite', 's:sliced params_rgb.0:sliced params_rgb.3:sliced params_depth.2:sliced'),
    ('sefuse_scale_add', 'x_rgb:chlast x_depth:sliced w:sliced'), ('sefuse_scale_add', 'x_rgb:sliced x_depth:chlast'),
    ('sefuse_weight_grad', 'gy:chlast x_rgb:sliced'), ('sefuse_weight_grad', 'gy:sliced x_depth:chlast'),
    ('sefuse_excite_backward', 'gw:sliced w:sliced weights_rgb.0:sliced weights_depth.1:sliced'),
    ('sefuse_apply_backward', 'gy:chlast w:sliced gs:sliced'), ('sefuse_apply_backward', 'gy:sliced'),
]


def _name(op, spec, override=None):
    extra = '' if override is None else '-' + ','.join(f'{k}={"tensor" if isinstance(v, torch.Tensor) else v}'
                                                       for k, v in override.items())
    return f"{op}-{spec.replace(' ', '+') or 'valid'}{extra}"


def _rows():
    for row in HOST:
        row = row + (None,) * (4 - len(row))
        yield pytest.param('cpu', *row, id='host-' + _name(row[0], row[1], row[3]))
    for row in DEVICE:
        row = row + (None,) * (4 - len(row))
        yield pytest.param('cuda', *row, id='device-' + _name(row[0], row[1], row[3]), marks=pytest.mark.gpu)


@pytest.mark.parametrize('dev,op,spec,expected,override', list(_rows()))
def test_what_a_call_ends_in(dev, op, spec, expected, override):
    if override is not None and dev == 'cuda':
        override = {k: v.to(dev) if isinstance(v, torch.Tensor) else v for k, v in override.items()}
    if expected is OK:
        call(op, dev, spec, override)
        if dev == 'cuda':
            torch.cuda.synchronize()
        return
    with pytest.raises(Exception) as e:
        call(op, dev, spec, override)
    print(op, spec, override, '->', type(e.value).__name__, e.value)
    assert type(e.value) is expected, (type(e.value).__name__, str(e.value))


def _flat(out):
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in _flat(o)]
    return [out]


@pytest.mark.gpu
@pytest.mark.parametrize('op', sorted({row[0] for row in DEVICE}))
def test_valid_call_is_taken(op):
    out = call(op, 'cuda')
    torch.cuda.synchronize()
    assert all(o is None or isinstance(o, (torch.Tensor, int)) for o in _flat(out))


@pytest.mark.gpu
@pytest.mark.parametrize('op,spec', LAYOUTS, ids=[_name(*row) for row in LAYOUTS])
def test_any_layout_gives_the_bits_of_its_contiguous_copy(op, spec):
    want, got = _flat(call(op, 'cuda')), _flat(call(op, 'cuda', spec))
    assert len(want) == len(got) and any(w is not None for w in want)
    for w, g in zip(want, got):
        assert (w is None and g is None) or (w.dtype == g.dtype and w.shape == g.shape
                                             and torch.equal(w.view(torch.uint8), g.view(torch.uint8)))
