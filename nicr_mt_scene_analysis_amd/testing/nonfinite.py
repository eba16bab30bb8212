"""TEST INFRASTRUCTURE — never imported by the product path.

NaN, +inf and -inf through the model-side kernels: the class map of a tensor, the placer of ONE poisoned
value, the table of cases (inputs, placements and the plain torch composition of every entry point, on the
CPU in float64) and the three assertions tests/test_nonfinite_model.py holds the device to.

The oracle is the composition of torch operations the reference model runs (`F.batch_norm`, `F.relu`,
`F.adaptive_avg_pool2d`, `F.interpolate`, `F.layer_norm`, `F.conv2d`, ...), forward and through
`torch.autograd`, NOT the matrix restatements of the sibling `*_ref.py` files: a resize matrix multiplies
every cell by a weight, zeros included, and 0 * inf poisons pixels neither torch nor a kernel poisons.

A case is one chain of entry points on one shape.  `run(case, dtype, device_fn)` puts every poison at every
placement of every map input in turn and compares the device's results (`device_fn`; None: the composition
alone, which is what the host tier checks) with the composition of the same, already dtype-rounded inputs:
  touched      an output element at which the clean and the poisoned composition differ, or which is
               non-finite in the poisoned one
  class        the device's class map equals the composition's; a kernel of `REGROUPED` may answer another
               non-finite class at a touched element, never a finite value for a non-finite one or the reverse
  containment  every untouched element holds the bits of the device's own clean run
  touched and finite   the device's value is finite, exactly 0 where the composition's is, and within
               tol + (u_out + 8 u_f32) |value| of it: tol is the LARGEST bound the family's own `bounds`
               gives for that output on the clean input, and the second term is the rounding of the value
               itself (a touched value may be larger than every clean one: a saturated sigmoid weight);
               loose on purpose, it catches garbage, not rounding
A run is honest when the poison shows and stays contained in the composition itself: every poisoned run has
a touched and an untouched output element, NaN and +inf always leave a non-finite one, and -inf does unless
the composition maps it to finite values everywhere (the forward pass of a ReLU: relu(-inf) = 0).
"""
import math

import torch
import torch.nn.functional as F

from . import block_cases as BC
from . import block_ref as RB
from . import context_cases as CC
from . import context_ref as RC
from . import encoder_fusion_cases as EC
from . import encoder_fusion_ref as RE
from . import fusion_ref as RF
from . import mlp_decoder_cases as MC
from . import mlp_decoder_ref as RM
from . import upsampling_ref as RU

FINITE, NAN, POS_INF, NEG_INF = 0, 1, 2, 3
POISONS = {'nan': math.nan, '+inf': math.inf, '-inf': -math.inf}
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = (F32, BF16, F16)
U_OUT = {torch.float64: 2.0 ** -53, F32: 2.0 ** -24, BF16: 2.0 ** -8, F16: 2.0 ** -11}
EPS, MOM = 1e-5, 0.1

# The kernels whose arithmetic is grouped otherwise than ATen's: at a touched element they may answer NaN for
# an infinity or the reverse (inf - inf against inf + finite).  Every other kernel states ATen's operations in
# ATen's order and must give ATen's class at every element.
REGROUPED = {
    'bntail_stats': 'unit means first, deviations from the unit mean: Welford-style partials, not sum(x) / M',
    'bntail_apply/train': "merges the unit partials by Chan's formula (d = mb - ma, M2 + d * d * na * r)",
    'bntail_backward_apply/train': '(gu - dbeta / M) - xh * (dgamma / M), not (gy - mean(gy) - (x - mean) * k) of ATen',
    'ln_nhwc_to_nchw_backward': 'rstd * (a - mean(a) - xh * mean(a * xh)) with tree sums, not the three-term form of ATen',
    'ppm_pool_backward': 'a gather: one pixel sums gp / area over the cells above it, not a scatter of gp / area',
    'ppm_upsample_concat_backward': 'a gather over the output pixels of a cell, zero-weight taps included',
    'mlpdec_upsample_concat_backward': 'a gather over the output pixels of a cell, zero-weight taps included',
    'upsample2x_dw3x3': 'the 9 taps of the doubled map regrouped into pre-added weight sums over 4 source pixels',
    'upsample2x_dw3x3_backward': 'the transposed regrouping: weight sums per source pixel, plane sums as trees',
}


def classify(t: torch.Tensor) -> torch.Tensor:
    """uint8 map: 0 finite, 1 NaN, 2 +inf, 3 -inf"""
    t = t.detach()
    out = torch.zeros(t.shape, dtype=torch.uint8, device=t.device)
    out[torch.isnan(t)] = NAN
    out[t == math.inf] = POS_INF
    out[t == -math.inf] = NEG_INF
    return out


def place(inputs: dict, name: str, index: int, value: float) -> dict:
    """a copy of `inputs` in which the element `index` (flat) of the tensor `name` is `value`"""
    out = dict(inputs)
    t = inputs[name].clone()
    t.view(-1)[index] = value
    out[name] = t
    return out


def touched(clean64: torch.Tensor, poisoned64: torch.Tensor) -> torch.Tensor:
    return (clean64 != poisoned64) | ~torch.isfinite(poisoned64)


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_class(got, want64, mask, regrouped: bool, tag) -> None:
    a, b = classify(got).cpu(), classify(want64)
    if not regrouped:
        assert torch.equal(a, b), (tag, 'class', int((a != b).sum()))
        return
    assert torch.equal(a == FINITE, b == FINITE), (tag, 'finite where the composition is not, or the reverse')
    assert torch.equal(a[~mask], b[~mask]), (tag, 'class off the touched elements')


def assert_contained(got, got_clean, mask, tag) -> None:
    a, b = _bits(got), _bits(got_clean)
    assert torch.equal(a[~mask], b[~mask]), (tag, 'containment', int((a != b)[~mask].sum()))


def assert_touched_finite(got, want64, mask, tol: float, tag) -> None:
    m = mask & torch.isfinite(want64)
    if not bool(m.any()):
        return
    g, w = got.detach().cpu().double()[m], want64[m]
    assert bool(torch.isfinite(g).all()), (tag, 'touched and finite: not finite on the device')
    zero = w == 0
    assert bool((g[zero] == 0).all()), (tag, 'touched and finite: exactly 0 in the composition')
    room = tol + (U_OUT[got.dtype] + 8 * U_OUT[F32]) * w.abs()
    assert bool(((g - w).abs() <= room).all()), (tag, 'touched and finite', float(((g - w).abs() - room).max()))


class Case:
    """one chain of entry points on one shape.
    make(dtype) -> dict of CPU tensors (maps rounded to dtype, parameters float32)
    comp(inputs64) -> (outputs: dict of float64 tensors, feed: dict the device chain takes from the composition)
    tol(inputs, dtype) -> dict output -> the largest bound of the family on the clean input
    maps: the inputs that are poisoned in turn; places(name, tensor, dtype) -> flat indices
    kernel_of(output) -> the entry point that writes it (a key of REGROUPED or not)"""

    def __init__(self, ident, family, make, comp, tol, maps, places, kernel_of, **info):
        self.id, self.family, self.make, self.comp, self.tol = ident, family, make, comp, tol
        self.maps, self.places, self.kernel_of, self.info = maps, places, kernel_of, info

    def __repr__(self):
        return self.id


def to64(inputs: dict) -> dict:
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in inputs.items()}


def run(case: Case, dtype, device_fn=None, poisons=POISONS):
    """every poison at every placement of every map of the case (see the module docstring); with `device_fn`
    (inputs, feed) -> dict of device outputs the three assertions, always the honesty of the composition.
    -> the number of poisoned runs"""
    clean = case.make(dtype)
    want_clean, feed_clean = case.comp(to64(clean))
    got_clean = device_fn(clean, feed_clean) if device_fn else None
    tol = case.tol(clean, dtype) if device_fn else None
    runs = 0
    for name in case.maps:
        for index in case.places(name, clean[name], dtype):
            for pname, value in poisons.items():
                tag = (case.id, str(dtype), name, index, pname)
                inputs = place(clean, name, index, value)
                want, feed = case.comp(to64(inputs))
                masks = {k: touched(want_clean[k], want[k]) for k in want}
                n_touched = sum(int(m.sum()) for m in masks.values())
                n_bad = sum(int((~torch.isfinite(want[k])).sum()) for k in want)
                assert 0 < n_touched < sum(m.numel() for m in masks.values()), (tag, 'nothing touched or nothing left')
                if pname != '-inf':                                 # relu(-inf) = 0 may leave every output finite
                    assert n_bad > 0, (tag, 'a NaN and a +inf must reach an output')
                runs += 1
                if device_fn is None:
                    continue
                got = device_fn(inputs, feed)
                assert set(got) == set(want), tag
                for k in want:
                    regrouped = case.kernel_of(k) in REGROUPED
                    assert tuple(got[k].shape) == tuple(want[k].shape), (tag, k)
                    assert_class(got[k], want[k], masks[k], regrouped, tag + (k,))
                    assert_contained(got[k], got_clean[k], masks[k], tag + (k,))
                    assert_touched_finite(got[k], want[k], masks[k], tol[k], tag + (k,))
    return runs


def _grads(outputs, inputs, grad_outputs):
    """autograd of the composition; an input nothing depends on gives zeros"""
    got = torch.autograd.grad(outputs, inputs, grad_outputs, allow_unused=True)
    return [torch.zeros_like(i) if g is None else g for g, i in zip(got, inputs)]


def _default_places(boundary):
    def places(name, t, dtype):
        out = [0, t.numel() - 1, boundary(name, t, dtype)]
        assert len(set(out)) == 3 and all(0 <= i < t.numel() for i in out), (name, out)
        return out
    return places


def vec(dtype) -> int:
    """elements of a 16-byte access"""
    return 4 if dtype == F32 else 8


# ------------------------------------------------------------------------------ residual blocks: the BN tail
BLOCK_SHAPES = ((2, 5, (3, 5)), (2, 5, BC.EXACT_HW), (2, 16, (15, 20)), (3, 5, BC.SEG_HW))
BLOCK_STEPS = ('forward/train', 'forward/eval', 'backward/train', 'backward/eval')


def _block_boundary(name, t, dtype):
    """in a plane of the middle of the tensor: the single element of the second segment of a 3 x 683 plane, else
    the last element of the first 16-byte vector"""
    hw = t.shape[2] * t.shape[3]
    plane = t.shape[1] + 1                                          # image 1, channel 1
    return plane * hw + (BC.SEGMENT if hw > BC.SEGMENT else vec(dtype) - 1)


def _block_make(B, C, hw, seed, with_extras):
    def make(dtype):
        c = RB.make_tail_inputs(B, C, hw, seed, dtype, identity=with_extras, scale=with_extras)
        c = {k: v for k, v in c.items() if v is not None}
        # the gates at the placements are open (a closed ReLU gate answers 0 to every gy and nothing would be touched)
        for i in _default_places(_block_boundary)('x', c['x'], dtype):
            c['x'].view(-1)[i] = 8.0
            if with_extras:
                c['identity'].view(-1)[i] = 4.0
        return c
    return make


def block_composition(inp, act, training, backward):
    """F.batch_norm -> * scale -> + identity -> F.relu / F.silu in the inputs' precision, with the saved
    statistics by plain reductions and the unit partials of the statistics kernel"""
    x = inp['x'].clone().requires_grad_(True)
    B, C, H, W = x.shape
    gamma, beta = inp['gamma'].clone().requires_grad_(True), inp['beta'].clone().requires_grad_(True)
    rm, rv = inp['running_mean'].clone(), inp['running_var'].clone()
    identity = inp['identity'].clone().requires_grad_(True) if 'identity' in inp else None
    if training:
        mean, var = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)
    else:
        mean, var = rm.clone(), rv.clone()
    invstd = 1.0 / torch.sqrt(var + EPS)
    z = F.batch_norm(x, rm, rv, gamma, beta, training, MOM, EPS)
    if 'scale' in inp:
        z = z * inp['scale'].reshape(B, C, 1, 1)
    if identity is not None:
        z = z + identity
    y = F.relu(z) if act == 'relu' else F.silu(z)
    feed = {'y': y.detach(), 'mean': mean.detach(), 'invstd': invstd.detach()}
    if not backward:
        out = {'y': y.detach(), 'mean': mean.detach(), 'invstd': invstd.detach(), 'running_mean': rm, 'running_var': rv}
        if training:
            nseg = -(-H * W // BC.SEGMENT)
            parts = []
            for seg in x.detach().reshape(B, C, H * W).split(BC.SEGMENT, dim=2):
                m = seg.mean(2)
                parts.append(torch.stack((m, ((seg - m[..., None]) ** 2).sum(2)), -1))     # [B, C, 2]
            out['part'] = torch.stack(parts, 1).permute(2, 0, 1, 3).reshape(C, B * nseg, 2)
        return out, feed
    wrt = [x, gamma, beta] + ([identity] if identity is not None else [])
    g = _grads(y, wrt, inp['gy'])
    out = {'gx': g[0], 'dgamma': g[1], 'dbeta': g[2]}
    if identity is not None:
        out['gid'] = g[3]
    return out, feed


def _block_tol(act, training, backward):
    def tol(c, dtype):
        f = RB.tail_forward(c['x'], c['gamma'], c['beta'], c['running_mean'], c['running_var'], EPS, MOM, training, act,
                            c.get('identity'), c.get('scale'), dtype)
        if not backward:
            out = {k: float(f[k].e.max()) for k in ('y', 'mean', 'invstd', 'running_mean', 'running_var')}
            out['part'] = 0.0                                       # a unit with a poison has no finite partial
            return out
        b = RB.tail_backward(c['gy'], c['x'], c['gamma'], c['beta'], f['mean'].v.float(), f['invstd'].v.float(), training,
                             act, f['y'].v.to(dtype), c.get('identity'), c.get('scale'), dtype)
        return {k: float(b[k].e.max()) for k in ('gx', 'gid', 'dgamma', 'dbeta')}
    return tol


def block_cases():
    out = []
    for n, (B, C, hw) in enumerate(BLOCK_SHAPES):
        for act in BC.ACTS:
            for step in BLOCK_STEPS:
                for extras in (False, True):
                    backward, training = step.startswith('backward'), step.endswith('train')
                    # the ReLU backward reads y, not the identity: there the identity is no input of the step
                    maps = (('gy', 'x') if backward else ('x',))
                    maps += ('identity',) if extras and not (backward and act == 'relu') else ()
                    mode = step.split('/')[1]

                    def kernel_of(k, backward=backward, mode=mode):
                        if k == 'part':
                            return 'bntail_stats'
                        if backward and k in ('dgamma', 'dbeta') and mode == 'eval':
                            return 'bntail_backward_reduce'
                        return ('bntail_backward_apply/' if backward else 'bntail_apply/') + mode
                    out.append(Case(
                        f"block-{B}x{C}x{hw[0]}x{hw[1]}-{act}-{step}-{'scale+id' if extras else 'plain'}", 'block',
                        _block_make(B, C, hw, 900 + n, extras),
                        lambda inp, a=act, t=training, b=backward: block_composition(inp, a, t, b),
                        _block_tol(act, training, backward), maps, _default_places(_block_boundary), kernel_of,
                        act=act, training=training, backward=backward, hw=hw))
    return out


# ------------------------------------------------------------------------------ encoder RGB-D fusion
SEFUSE_SHAPES = ((48, (3, 5)), (48, (15, 20)), (48, EC.BLOCK_HW), (16, (3, 5)))
SEFUSE_KERNELS = {'s': 'sefuse_squeeze', 'z1': 'sefuse_excite', 'w': 'sefuse_excite', 'y': 'sefuse_scale_add',
                  'gw': 'sefuse_weight_grad', 'gz2': 'sefuse_excite_backward', 'gz1': 'sefuse_excite_backward',
                  'gs': 'sefuse_excite_backward', 'h': 'sefuse_excite_backward', 'gx_rgb': 'sefuse_apply_backward',
                  'gx_depth': 'sefuse_apply_backward'}
SEFUSE_PARAMS = tuple(f'{k}_{m}' for m in ('rgb', 'depth') for k in ('W1', 'b1', 'W2', 'b2'))


def sefuse_params(inp):
    return tuple(tuple(inp[f'{k}_{m}'] for k in ('W1', 'b1', 'W2', 'b2')) for m in ('rgb', 'depth'))


def _sefuse_boundary(name, t, dtype):
    """image 1, channel 1: the single element past the wave route's plane, else the last of a 16-byte vector"""
    hw = t.shape[2] * t.shape[3]
    return (t.shape[1] + 1) * hw + (EC.WAVE_MAX if hw > EC.WAVE_MAX else vec(dtype) - 1)


def _sefuse_make(C, hw, seed):
    def make(dtype):
        x_rgb, x_depth, gy = RE.make_inputs(EC.B, C, hw, seed, dtype)
        out = {'x_rgb': x_rgb, 'x_depth': x_depth, 'gy': gy}
        for m, group in zip(('rgb', 'depth'), RE.make_params(C, seed + 1)):
            out.update({f'{k}_{m}': v for k, v in zip(('W1', 'b1', 'W2', 'b2'), group)})
        return out
    return make


def sefuse_composition(inp, act):
    """`encoder_fusion_ref.torch_formulation` with its intermediates kept, and its gradients by autograd"""
    fn = F.relu if act == 'relu' else F.silu
    xs = [inp['x_rgb'].clone().requires_grad_(True), inp['x_depth'].clone().requires_grad_(True)]
    keep = {k: [] for k in ('s', 'z1', 'h', 'z2', 'w')}
    parts = []
    for x, (W1, b1, W2, b2) in zip(xs, sefuse_params(inp)):
        W1 = W1.reshape(W1.shape[0], W1.shape[1], 1, 1)
        W2 = W2.reshape(W2.shape[0], W2.shape[1], 1, 1)
        s = F.adaptive_avg_pool2d(x, 1)
        z1 = F.conv2d(s, W1, b1)
        h = fn(z1)
        z2 = F.conv2d(h, W2, b2)
        w = torch.sigmoid(z2)
        parts.append(x * w)
        for k, v in zip(('s', 'z1', 'h', 'z2', 'w'), (s, z1, h, z2, w)):
            keep[k].append(v)
    y = parts[0] + parts[1]
    wrt = xs + keep['s'] + keep['z1'] + keep['z2'] + keep['w']
    g = _grads(y, wrt, inp['gy'])

    def pair(seq):
        return torch.stack([t.detach().flatten(1) for t in seq])
    out = {'s': pair(keep['s']), 'z1': pair(keep['z1']), 'w': pair(keep['w']), 'y': y.detach(), 'h': pair(keep['h']),
           'gx_rgb': g[0], 'gx_depth': g[1], 'gs': pair(g[2:4]), 'gz1': pair(g[4:6]), 'gz2': pair(g[6:8]),
           'gw': pair(g[8:10])}
    return out, {}


def _sefuse_tol(act):
    def tol(c, dtype):
        b = RE.bounds(c['x_rgb'], c['x_depth'], sefuse_params(c), act, c['gy'], dtype)
        return {k: float(b[k].max()) for k in SEFUSE_KERNELS}
    return tol


def sefuse_cases():
    out = []
    for n, (C, hw) in enumerate(SEFUSE_SHAPES):
        for act in EC.ACTS:
            out.append(Case(f'sefuse-{C}x{hw[0]}x{hw[1]}-{act}', 'sefuse', _sefuse_make(C, hw, 920 + 2 * n),
                            lambda inp, a=act: sefuse_composition(inp, a), _sefuse_tol(act),
                            ('x_rgb', 'x_depth', 'gy'), _default_places(_sefuse_boundary), SEFUSE_KERNELS.get,
                            act=act, hw=hw))
    return out


# ------------------------------------------------------------------------------ LayerNorm-transpose (Swin fusion)
LNT_PAIRS = ((F32, F32), (BF16, BF16), (BF16, F32), (F16, F16), (F16, F32))      # (dtype_x, dtype_y): test_fusion.PAIRS
LNT_B, LNT_PS, LNT_CS, LNT_TILE = 2, (31, 33, 64), (6, 160), 32


def _lnt_places(name, t, pair):
    """the first, the last, and one at the tile of 32 pixels: its first pixel past the tile (P > 32), else the
    last pixel of a 16-byte vector of the NCHW side; image 1, a channel in the middle"""
    if name == 'x':                                                 # [B, P, C]
        _, P, C = t.shape
        p = LNT_TILE if P > LNT_TILE else vec(pair[1]) - 1
        mid = (P + p) * C + C // 2
    else:                                                           # [B, C, P]
        _, C, P = t.shape
        p = LNT_TILE if P > LNT_TILE else vec(pair[1]) - 1
        mid = (C + C // 2) * P + p
    return [0, t.numel() - 1, mid]


def _lnt_make(P, C, seed, with_add):
    def make(pair):
        x, gamma, beta, gy, add = RF.make_inputs('normal', LNT_B, P, C, seed, pair[0])
        out = {'x': x, 'gamma': gamma, 'beta': beta, 'gy': gy.to(pair[1])}
        if with_add:
            out['add'] = add.to(pair[1])
        return out
    return make


def lnt_composition(inp):
    x = inp['x'].clone().requires_grad_(True)                       # [B, P, C] as [B, 1, P, C]
    B, P, C = x.shape
    gamma, beta = inp['gamma'].clone().requires_grad_(True), inp['beta'].clone().requires_grad_(True)
    add = inp['add'].reshape(B, C, 1, P) if 'add' in inp else None
    y = RF.torch_formulation(x.reshape(B, 1, P, C), gamma, beta, EPS, add)
    g = _grads(y, [x, gamma, beta], inp['gy'].reshape(B, C, 1, P))
    return {'y': y.detach().reshape(B, C, P), 'gx': g[0], 'ggamma': g[1], 'gbeta': g[2]}, {}


def _lnt_tol(c, pair):
    b = RF.bounds(c['x'], c['gamma'], c['beta'], EPS, c.get('add'), c['gy'], dtype_y=pair[1], dtype_x=pair[0])
    return {k: float(b[k].max()) for k in ('y', 'gx', 'ggamma', 'gbeta')}


def lnt_cases():
    out = []
    for P in LNT_PS:
        for C in LNT_CS:
            for with_add in (False, True):
                maps = ('x', 'gy') + (('add',) if with_add else ())
                out.append(Case(f"lnt-P{P}-C{C}-{'add' if with_add else 'plain'}", 'lnt',
                                _lnt_make(P, C, 940 + P + C, with_add), lnt_composition, _lnt_tol, maps, _lnt_places,
                                lambda k: 'ln_nhwc_to_nchw' if k == 'y' else 'ln_nhwc_to_nchw_backward', P=P, C=C))
    return out


# ------------------------------------------------------------------------------ context module
PPM_B, PPM_C, PPM_CR = 2, 3, 3
PPM_GEOMETRIES = (((7, 9), CC.sizes_of((1, 5))), ((8, 16), CC.sizes_of((1, 2, 4, 8))),
                  next((hw, sizes) for hw, sizes, lds in CC.ROUTE_CASES if not lds))
PPM_MODES = ('nearest', 'bilinear')


def _ppm_places(name, t, dtype):
    """the first, the last, and in image 1, channel 1 (of the branches in g_out): for the full-size maps a pixel in the overlap of two adaptive
    windows ((1, 1) of 7 x 9 under 5 bins) or the last pixel of the first 16-byte vector of row 1, for a pooled map
    its middle cell"""
    H, W = t.shape[2:]
    skip = PPM_C if name == 'g_out' else 0                          # the channels of x in g_out reach no kernel output
    plane = (t.shape[1] + skip + 1) * H * W
    if name in ('x', 'g_out'):
        mid = plane + W + (1 if (H, W) == (7, 9) else min(vec(dtype), W) - 1)
    else:
        mid = plane + (H * W) // 2
    return sorted({skip * H * W, t.numel() - 1, mid})


def _ppm_make(hw, sizes, seed):
    def make(dtype):
        x, ys, g_out, gps = RC.make_inputs(PPM_B, PPM_C, PPM_CR, hw, sizes, seed, dtype)
        out = {'x': x, 'g_out': g_out}
        out.update({f'ys{i}': y for i, y in enumerate(ys)})
        out.update({f'gps{i}': g for i, g in enumerate(gps)})
        return out
    return make


def ppm_composition(inp, sizes, mode):
    n = len(sizes)
    x = inp['x'].clone().requires_grad_(True)
    ys = [inp[f'ys{i}'].clone().requires_grad_(True) for i in range(n)]
    pooled = RC.torch_pool(x, sizes)
    out = {f'pooled{i}': p.detach() for i, p in enumerate(pooled)}
    out['gx_pool'] = _grads(pooled, [x], [inp[f'gps{i}'] for i in range(n)])[0]
    cat = RC.torch_upcat(x, ys, mode)
    out['cat'] = cat.detach()
    for i, g in enumerate(_grads(cat, ys, inp['g_out'])):
        out[f'gys{i}'] = g
    return out, {}


def _ppm_tol(sizes, mode):
    def tol(c, dtype):
        n = len(sizes)
        ys, gps = [c[f'ys{i}'] for i in range(n)], [c[f'gps{i}'] for i in range(n)]
        b = RC.bounds(c['x'], sizes, ys, mode, c['g_out'], gps, dtype)
        out = {'cat': float(b['cat'].max()), 'gx_pool': float(b['gx_pool'].max())}
        for i in range(n):
            out[f'pooled{i}'], out[f'gys{i}'] = float(b['pooled'][i].max()), float(b['gys'][i].max())
        return out
    return tol


def _ppm_kernel(k):
    if k.startswith('pooled'):
        return 'ppm_pool'
    return {'gx_pool': 'ppm_pool_backward', 'cat': 'ppm_upsample_concat'}.get(k, 'ppm_upsample_concat_backward')


def _resized_branch(hw, shapes, mode):
    """the branch whose map is poisoned: the last one; under 'bilinear' the last one NO axis of which already has
    the output size.  ATen's CPU kernel states such an axis as the taps (d, d) with the weights (1, 0), so that an
    infinity answers inf * 1 + inf * 0 = NaN at its own pixel, where ATen's device kernel, a copy and the four-tap
    sum all give the infinity: on such a branch the CPU composition is no oracle for the class of an infinity"""
    ok = [i for i, (h, w) in enumerate(shapes) if mode == 'nearest' or (h != hw[0] and w != hw[1])]
    return ok[-1]


def ppm_cases():
    out = []
    for n, (hw, sizes) in enumerate(PPM_GEOMETRIES):
        last = len(sizes) - 1
        for mode in PPM_MODES:
            out.append(Case(f"ppm-{hw[0]}x{hw[1]}-{'-'.join(f'{a}x{b}' for a, b in sizes)}-{mode}", 'ppm',
                            _ppm_make(hw, sizes, 960 + n), lambda inp, s=sizes, m=mode: ppm_composition(inp, s, m),
                            _ppm_tol(sizes, mode), ('x', f'ys{_resized_branch(hw, sizes, mode)}', 'g_out', f'gps{last}'),
                            _ppm_places, _ppm_kernel,
                            hw=hw, sizes=sizes, mode=mode))
    return out


# ------------------------------------------------------------------------------ MLP decoders
# (channels, factors, (H, W)): the exact tier's branches at 8 x 16 (the vector route of every dtype), the same channels
# at 8 x 12 (a width off the half vector; the factors that divide it), the sibling file's element-route width
MLD_SHAPES = ((MC.EXACT_CHANNELS, MC.EXACT_FACTORS, (8, 16)), (MC.EXACT_CHANNELS, (4, 4, 2, 1), (8, 12)),
              MC.ELEMENT_CASES[0])


def mld_need(channels):
    """the backward call's wanted branches: the middle one unwanted where there are four"""
    return (True, False, True, True) if len(channels) == 4 else None


def _mld_places(name, t, dtype):
    H, W = t.shape[2:]
    plane = (t.shape[1] + (t.shape[1] > 1)) * H * W                 # image 1, channel 1 (0 of a single one)
    mid = plane + (W if H > 1 else 0) + min(vec(dtype), W) - 1      # row 1: the last pixel of its first 16-byte vector
    return sorted({0, t.numel() - 1, mid})


def _mld_make(channels, factors, hw, seed):
    def make(dtype):
        ys, g_out = RM.make_inputs(MC.GPU_B, channels, factors, hw, seed, dtype)
        out = {'g_out': g_out}
        out.update({f'ys{i}': y for i, y in enumerate(ys)})
        return out
    return make


def mld_composition(inp, n, mode, hw, need):
    ys = [inp[f'ys{i}'].clone().requires_grad_(True) for i in range(n)]
    cat = RM.torch_upcat(ys, mode, size=hw)
    out = {'cat': cat.detach()}
    for i, g in enumerate(_grads(cat, ys, inp['g_out'])):
        if need is None or need[i]:
            out[f'gys{i}'] = g
    return out, {}


def _mld_tol(n, mode, hw, need):
    def tol(c, dtype):
        b = RM.bounds([c[f'ys{i}'] for i in range(n)], mode, c['g_out'], dtype, size=hw)
        out = {'cat': float(b['cat'].max())}
        out.update({f'gys{i}': float(b['gys'][i].max()) for i in range(n) if need is None or need[i]})
        return out
    return tol


def mld_cases():
    out = []
    for k, (channels, factors, hw) in enumerate(MLD_SHAPES):
        n, need = len(channels), mld_need(channels)
        for mode in PPM_MODES:
            shapes = [(hw[0] // f, hw[1] // f) for f in factors]
            maps = tuple(f'ys{i}' for i in sorted({0, _resized_branch(hw, shapes, mode)})) + ('g_out',)
            out.append(Case(f"mld-{'.'.join(map(str, channels))}-{hw[0]}x{hw[1]}-{mode}", 'mld',
                            _mld_make(channels, factors, hw, 980 + k),
                            lambda inp, n=n, m=mode, hw=hw, need=need: mld_composition(inp, n, m, hw, need),
                            _mld_tol(n, mode, hw, need), maps, _mld_places,
                            lambda key: 'mlpdec_upsample_concat' + ('' if key == 'cat' else '_backward'),
                            mode=mode, hw=hw, need=need, n=n))
    return out


# ------------------------------------------------------------------------------ learned upsampling
UP_B, UP_C, UP_SIZES = 2, 13, ((9, 8), (9, 7))                     # the vector route, the one-pixel route


def _up_places(name, t, dtype):
    """both outer corners (every padding tap in play) and an interior pixel of image 1, channel 6"""
    H, W = t.shape[2:]
    return [0, t.numel() - 1, (t.shape[1] + 6) * H * W + (H // 2) * W + W // 2]


def _up_make(h, w, seed):
    def make(dtype):
        gen = torch.Generator().manual_seed(seed)
        return {'x': torch.randn((UP_B, UP_C, h, w), generator=gen).to(dtype),
                'gy': torch.randn((UP_B, UP_C, 2 * h, 2 * w), generator=gen).to(dtype),
                'weight': torch.randn((UP_C, 1, 3, 3), generator=gen) * 0.25, 'bias': torch.randn((UP_C,), generator=gen)}
    return make


def up_composition(inp, zeropad):
    x, wt, b = (inp[k].clone().requires_grad_(True) for k in ('x', 'weight', 'bias'))
    y = RU.torch_formulation(x, wt, b, zeropad)
    g = _grads(y, [x, wt, b], inp['gy'])
    return {'y': y.detach(), 'gx': g[0], 'gw': g[1], 'gb': g[2]}, {}


def _up_tol(zeropad):
    def tol(c, dtype):
        b = RU.bounds(c['x'], c['weight'], c['bias'], c['gy'], zeropad, dtype)
        return {k: float(b[k].max()) for k in ('y', 'gx', 'gw', 'gb')}
    return tol


def up_cases():
    out = []
    for k, (h, w) in enumerate(UP_SIZES):
        for zeropad in (False, True):
            out.append(Case(f"up-{h}x{w}-{'zeropad' if zeropad else 'replicate'}", 'up', _up_make(h, w, 990 + k),
                            lambda inp, z=zeropad: up_composition(inp, z), _up_tol(zeropad), ('x', 'gy'), _up_places,
                            lambda key: 'upsample2x_dw3x3' if key == 'y' else 'upsample2x_dw3x3_backward',
                            zeropad=zeropad, hw=(h, w)))
    return out


def all_cases():
    return block_cases() + sefuse_cases() + lnt_cases() + ppm_cases() + mld_cases() + up_cases()
