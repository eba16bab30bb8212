"""TEST INFRASTRUCTURE — never imported by the product path.

A float64 restatement of the fused batch-norm tail (csrc/block_tail.hip, include/nmsa.h nmsa_bntail_*) and
of the three residual blocks of model/block.py, forward and backward, TOGETHER WITH a bound on the error of
every output.

How the bounds are derived.  Every quantity is an `E`: a float64 value `v` and a non-negative bound `e` on
the absolute error of the float32 computation of it.  Every operation of the restatement is one operation
of the documented float32 arithmetic and propagates the bound to first order with the exact partial
derivatives taken at absolute values (a running error analysis), and adds ONE rounding, U = 2^-24 relative
to its own result:
    a + b: ea + eb + U |a + b|                a * b: |a| eb + |b| ea + ea eb + U |a b|
    a / b: (ea + |a / b| eb) / (|b| - eb) + U |a / b|       sqrt(a): ea / (2 sqrt(a - ea)) + U sqrt(a)
A fused multiply-add of the kernels counts as its two operations (one rounding more than it makes).
A sum of n terms costs `depth` roundings on the sum of the absolute terms, depth = the longest chain of
additions a term goes through.  In the kernels (include/nmsa.h, "Summation order"): at most 8 chunks per
lane, 3 pairwise levels, 6 wave levels inside a unit = 17, then ceil(U / 64) units per lane and 6 levels
between units, each ONE addition for the backward sums (`sum_depth`) and FOUR roundings on the mean for a
merge by Chan's formula (`stats_depth`).  The statistics are stated as mean = sum(x) / M and
var = sum((x - mean)^2) / M with that depth; Chan's merge computes the same two quantities and its cross
term d^2 na nb / n carries the error of the unit means, which the term 2 |x - mean| e(mean) of the
restated square carries too.  A variance from E[x^2] - E[x]^2 has the error U E[x^2], which lies OUTSIDE this
bound as soon as the mean is large against the deviation.
ReLU is 1-Lipschitz (e passes through); SiLU is 1.1-Lipschitz and SiLU' 0.5-Lipschitz, and their own
evaluation (expf within 2 ulp, a division, one to four products) costs SILU_K = 8 roundings of the largest
intermediate.  The ReLU gate of the backward pass is taken from the VALUE of the output (0 where y <= 0, so a NaN y passes
gy as a NaN z passes the forward, both as ATen does): a bound through a
gate holds where the gate cannot flip, which the tests that chain forward and backward assert on their
inputs (`block_reference`, 'margins'); the per-kernel backward tests hand y in as an input.
A half output is rounded once more, by half an ulp: 2^-8 relative (bfloat16, 8 significand bits) or 2^-11
(float16, 11 bits, plus half its subnormal spacing, 2^-25).
Convolutions (torch, not a kernel of this library) are bilinear: with K = 2 * fan-in + 8 roundings on the
convolution of the absolute values; the factor 2 leaves room for transform-based algorithms of the device
library, whose intermediate sums are longer than the direct form's.
The reference's own float32 (the fixture) uses other formulations of the same quantities (a fused scale
and shift in batch_norm, cascaded sums); tests/test_block_host.py holds it to these bounds BEFORE any kernel
is, which is the condition that ties the bounds to the reference.
"""
import math

import torch
import torch.nn.functional as F

from .. import _lib as L

U = 2.0 ** -24
SILU_K = 8.0
SEGMENT = L.NMSA_BNTAIL_SEGMENT
# unit roundoff 2^-p of a format with p significand bits: bfloat16 p = 8, float16 p = 11 (float32: p = 24, U above)
HALF_U = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def units(B: int, hw: int) -> int:
    return B * (-(-hw // SEGMENT))


def sum_depth(B: int, hw: int) -> float:
    return 17.0 + math.ceil(units(B, hw) / 64) + 6


def stats_depth(B: int, hw: int) -> float:
    return 17.0 + 4.0 * (math.ceil(units(B, hw) / 64) + 6)


class E:
    """a float64 value with a bound on the absolute error of its float32 computation"""

    def __init__(self, v, e=None):
        self.v = v.double() if torch.is_tensor(v) else torch.tensor(float(v), dtype=torch.float64)
        self.e = torch.zeros_like(self.v) if e is None else e.double().expand_as(self.v)

    @staticmethod
    def of(x):
        return x if isinstance(x, E) else E(x)

    def _done(self, v, e, roundings=1.0):
        return E(v, e + roundings * U * v.abs())

    def __add__(self, o):
        o = E.of(o)
        return self._done(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = E.of(o)
        return self._done(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = E.of(o)
        return self._done(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e)

    def __truediv__(self, o):
        o = E.of(o)
        v = self.v / o.v
        room = (o.v.abs() - o.e).clamp_min(1e-300)
        return self._done(v, (self.e + v.abs() * o.e) / room)

    def sqrt(self):
        v = self.v.sqrt()
        return self._done(v, self.e / (2.0 * (self.v - self.e).clamp_min(1e-300).sqrt()))

    def exact(self, fn):
        """an operation without a rounding (a view, a broadcast, a selection)"""
        return E(fn(self.v), fn(self.e))

    def sum(self, dims, depth):
        return E(self.v.sum(dims), self.e.sum(dims) + depth * U * self.v.abs().sum(dims))

    def zero_where(self, mask):
        """0 where `mask`, self elsewhere (a selection, not a product: inf and NaN under the mask give 0)"""
        return E(torch.where(mask, torch.zeros_like(self.v), self.v), torch.where(mask, torch.zeros_like(self.e), self.e))

    def rounded(self, dtype):
        h = HALF_U[dtype]
        return E(self.v, self.e + h * self.v.abs() + (2.0 ** -25 if dtype == torch.float16 else 0.0))


def bc(t: E) -> E:
    """a per-channel vector against a [B, C, H, W] map"""
    return t.exact(lambda a: a.reshape(1, -1, 1, 1))


def silu(z: E) -> E:
    v = z.v * torch.sigmoid(z.v)
    return E(v, 1.1 * z.e + SILU_K * U * (v.abs() + z.v.abs()))


def silu_grad(z: E) -> E:
    s = torch.sigmoid(z.v)
    v = s * (1.0 + z.v * (1.0 - s))
    return E(v, 0.5 * z.e + SILU_K * U * (1.0 + v.abs()))


def act_forward(z: E, act: str) -> E:
    if act == 'relu':
        return z.zero_where(z.v <= 0)                               # torch.relu: a NaN z passes
    return silu(z) if act == 'silu' else z


def act_backward(gy: E, z: E, y: E, act: str) -> E:
    if act == 'relu':
        return gy.zero_where(y.v <= 0)                              # ATen's threshold backward: a NaN y passes gy
    return gy * silu_grad(z) if act == 'silu' else gy


# ------------------------------------------------------------------------------ the tail
def tail_forward(x, gamma, beta, running_mean, running_var, eps, momentum, training, act, identity=None,
                 scale=None, dtype=torch.float32):
    """dict of E: mean, var (biased), invstd, z, y (rounded to `dtype`), running_mean, running_var (after the
    step).  x [B, C, H, W], identity alike or None, scale [B, C] or None; all E or tensors (exact)."""
    x, gamma, beta = E.of(x), E.of(gamma), E.of(beta)
    B, C, H, W = x.v.shape
    M = B * H * W
    out = {}
    if training:
        depth = stats_depth(B, H * W)
        mean = x.sum((0, 2, 3), depth) / float(M)
        d = x - bc(mean)
        m2 = (d * d).sum((0, 2, 3), depth)
        var = m2 / float(M)
        keep = 1.0 - momentum
        out['running_mean'] = E.of(running_mean) * keep + mean * momentum
        out['running_var'] = E.of(running_var) * keep + (m2 / float(M - 1)) * momentum
    else:
        mean, var = E.of(running_mean), E.of(running_var)
        d = x - bc(mean)
        out['running_mean'], out['running_var'] = mean, var
    invstd = E(1.0) / (var + eps).sqrt()
    xh = d * bc(invstd)
    z = xh * bc(gamma) + bc(beta)
    if scale is not None:
        z = z * E.of(scale).exact(lambda a: a.reshape(B, C, 1, 1))
    if identity is not None:
        z = z + E.of(identity)
    out.update(mean=mean, var=var, invstd=invstd, z=z, xh=xh, y=act_forward(z, act).rounded(dtype))
    return out


def tail_backward(gy, x, gamma, beta, mean, invstd, training, act, y=None, identity=None, scale=None,
                  dtype=torch.float32):
    """dict of E: gx, gid (rounded to `dtype`), dgamma, dbeta.  `y` (the gate under 'relu') and mean, invstd are
    inputs: E from `tail_forward` when a test chains the passes, tensors when it hands them to the kernels."""
    gy, x, gamma, beta, mean, invstd = (E.of(t) for t in (gy, x, gamma, beta, mean, invstd))
    B, C, H, W = x.v.shape
    M = float(B * H * W)
    depth = sum_depth(B, H * W)
    xh = (x - bc(mean)) * bc(invstd)
    z = None
    if act == 'silu':
        z = xh * bc(gamma) + bc(beta)
        if scale is not None:
            z = z * E.of(scale).exact(lambda a: a.reshape(B, C, 1, 1))
        if identity is not None:
            z = z + E.of(identity)
    gz = act_backward(gy, z, None if y is None else E.of(y), act)
    gu = gz if scale is None else gz * E.of(scale).exact(lambda a: a.reshape(B, C, 1, 1))
    dbeta = gu.sum((0, 2, 3), depth)
    dgamma = (gu * xh).sum((0, 2, 3), depth)
    k = gamma * invstd
    if training:
        gx = bc(k) * ((gu - bc(dbeta / M)) - xh * bc(dgamma / M))
    else:
        gx = bc(k) * gu
    return dict(gx=gx.rounded(dtype), gid=gz.rounded(dtype), dgamma=dgamma, dbeta=dbeta)


def worst_ratio(got, ref: E, extra=None) -> float:
    """max |got - ref| / bound (0 / 0 counts as 0)"""
    diff = (got.detach().double().cpu() - ref.v).abs()
    bound = ref.e if extra is None else ref.e + extra
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / bound.clamp_min(1e-300))
    return float(ratio.max()) if ratio.numel() else 0.0


def merge_partials64(part, B, hw):
    """(mean, var) float64 [C] of the [C, U, 2] unit partials of `ops.bntail_stats`, merged exactly"""
    part = part.double().cpu()
    nseg = -(-hw // SEGMENT)
    n = torch.tensor([min(SEGMENT, hw - (u % nseg) * SEGMENT) for u in range(B * nseg)], dtype=torch.float64)
    total = n.sum()
    mean = (part[:, :, 0] * n).sum(1) / total
    m2 = (part[:, :, 1] + n * (part[:, :, 0] - mean[:, None]) ** 2).sum(1)
    return mean, m2 / total


# ------------------------------------------------------------------------------ inputs of the GPU tier
def make_tail_inputs(B, C, hw, seed, dtype=torch.float32, identity=True, scale=True):
    """seeded inputs of a segment, rounded to `dtype`: x with a per-channel offset and spread, the identity, the
    upstream gradient, a Dropout2d scale of p = 0.25 (0 or 4/3 rounded to dtype), gamma, beta and running
    statistics in float32"""
    gen = torch.Generator().manual_seed(seed)
    shape = (B, C) + tuple(hw)
    off = torch.randn((1, C, 1, 1), generator=gen)
    spread = 0.5 + torch.rand((1, C, 1, 1), generator=gen)
    out = {'x': (off + spread * torch.randn(shape, generator=gen)).to(dtype),
           'identity': torch.randn(shape, generator=gen).to(dtype) if identity else None,
           'gy': torch.randn(shape, generator=gen).to(dtype),
           'scale': ((torch.rand((B, C), generator=gen) < 0.75).float() / 0.75).to(dtype) if scale else None,
           'gamma': 0.5 + torch.rand((C,), generator=gen), 'beta': 0.5 * torch.randn((C,), generator=gen),
           'running_mean': torch.randn((C,), generator=gen), 'running_var': 0.5 + torch.rand((C,), generator=gen)}
    return out


# ------------------------------------------------------------------------------ the whole blocks
def conv_fan_in(weight) -> int:
    return int(weight.shape[1] * weight.shape[2] * weight.shape[3])


def bilinear(fn, a: E, b: E, K: float) -> E:
    v = fn(a.v, b.v)
    aa, ab = a.v.abs(), b.v.abs()
    return E(v, fn(aa, b.e) + fn(a.e, ab) + fn(a.e, b.e) + K * U * fn(aa, ab))


class Conv:
    """a convolution of a block, forward and backward, as bilinear operations on E"""

    def __init__(self, weight, bias, stride, padding, dilation):
        self.w, self.b = E.of(weight), None if bias is None else E.of(bias)
        self.kw = dict(stride=stride, padding=padding, dilation=dilation)
        self.K = 2.0 * conv_fan_in(weight) + 8.0

    def forward(self, x: E) -> E:
        self.x = x
        out = bilinear(lambda a, b: F.conv2d(a, b, **self.kw), x, self.w, self.K)
        return out if self.b is None else out + bc(self.b)

    def backward(self, g: E):
        """-> (gx, gweight, gbias)"""
        xs, ws = self.x.v.shape, self.w.v.shape
        K_in = 2.0 * ws[0] * ws[2] * ws[3] + 8.0
        K_w = 2.0 * g.v.shape[0] * g.v.shape[2] * g.v.shape[3] + 8.0
        gx = bilinear(lambda a, b: torch.nn.grad.conv2d_input(xs, b, a, **self.kw), g, self.w, K_in)
        gw = bilinear(lambda a, b: torch.nn.grad.conv2d_weight(a, ws, b, **self.kw), self.x, g, K_w)
        n = g.v.shape[0] * g.v.shape[2] * g.v.shape[3]
        return gx, gw, None if self.b is None else g.sum((0, 2, 3), float(n))


def _conv_of(state, name, stride=1, padding=0, dilation=1):
    return Conv(state[f'{name}.weight'], state.get(f'{name}.bias'), stride, padding, dilation)


def _conv_of_like(c: Conv) -> Conv:
    return Conv(c.w.v, None if c.b is None else c.b.v, c.kw['stride'], c.kw['padding'], c.kw['dilation'])


class Tail:
    """a batch-norm tail of a block on E, forward and backward; `act` may be 'none' (the downsample branch)"""

    def __init__(self, state, name, act, training, eps=1e-5, momentum=0.1):
        self.name, self.act, self.training, self.eps, self.momentum = name, act, training, eps, momentum
        self.p = {k: state[f'{name}.{k}'] for k in ('weight', 'bias', 'running_mean', 'running_var')}

    def forward(self, x: E, identity=None, scale=None) -> E:
        self.x, self.identity, self.scale = x, identity, scale
        self.f = tail_forward(x, self.p['weight'], self.p['bias'], self.p['running_mean'], self.p['running_var'],
                              self.eps, self.momentum, self.training, self.act, identity, scale)
        return self.f['y']

    def backward(self, g: E):
        return tail_backward(g, self.x, self.p['weight'], self.p['bias'], self.f['mean'], self.f['invstd'],
                             self.training, self.act, self.f['y'], self.identity, self.scale)


def block_reference(kind, state, x, gy, act, training, stride=1, dilation=1, scale=None):
    """The float64 restatement of a whole block with its bounds.  `state`: the block's state dict (float32
    tensors; a `downsample.conv.weight` key means a 1x1 ConvNormAct without activation on the identity
    path); `scale`: the Dropout2d scale [B, C] of a training NonBottleneck1D or None.
    -> dict of E: 'y', 'gx', 'grad/<parameter key>', 'state/<running statistic key>' (after the step), and
    'margins': [(name, min |z| / (64 * the segment's own bound of z), min |z| / the accumulated bound of z)] of
    every ReLU the block holds; both must exceed 1."""
    x, gy = E.of(x), E.of(gy)
    convs, tails, margins = {}, {}, []
    has_ds = 'downsample.conv.weight' in state

    def conv(name, inp, **kw):
        convs[name] = _conv_of(state, name, **kw)
        return convs[name].forward(inp)

    def tail(name, a, inp, identity=None, sc=None):
        tails[name] = Tail(state, name, a, training)
        y = tails[name].forward(inp, identity, sc)
        if a == 'relu':
            own = Tail(state, name, a, training)
            own.forward(E(inp.v), None if identity is None else E(identity.v), sc)
            margin(name, tails[name].f['z'], own.f['z'])
        return y

    def margin(name, z, z_own):
        """how far a ReLU's argument stays from 0: against 64 times the bound of the segment's own forward
        arithmetic (its input taken as exact), and against the bound accumulated from the block's input
        (above it the gate cannot flip, which the bounds behind the gate rest on)"""
        margins.append((name, float((z.v.abs() / (64.0 * z_own.e).clamp_min(1e-300)).min()),
                        float((z.v.abs() / z.e.clamp_min(1e-300)).min())))

    def plain_act(name, cv, z):
        if act == 'relu':
            margin(name, z, _conv_of_like(convs[cv]).forward(E(convs[cv].x.v)))
        return act_forward(z, act)

    def identity_path():
        if not has_ds:
            return x
        return tail('downsample.norm', 'none', conv('downsample.conv', x, stride=stride))

    if kind == 'basicblock':
        t = tail('norm1', act, conv('conv1', x, stride=stride, padding=1))
        y = tail('norm2', act, conv('conv2', t, padding=1), identity_path())
        order = [('norm2', 'conv2'), ('norm1', 'conv1')]
    elif kind == 'bottleneck':
        t = tail('norm1', act, conv('conv1', x))
        t = tail('norm2', act, conv('conv2', t, stride=stride, padding=dilation, dilation=dilation))
        y = tail('norm3', act, conv('conv3', t), identity_path())
        order = [('norm3', 'conv3'), ('norm2', 'conv2'), ('norm1', 'conv1')]
    else:
        z11 = conv('conv1_1', x, stride=(stride, 1), padding=(1, 0))
        a11 = plain_act('act1_1', 'conv1_1', z11)
        t = tail('norm1', act, conv('conv1_2', a11, stride=(1, stride), padding=(0, 1)))
        z21 = conv('conv2_1', t, padding=(dilation, 0), dilation=(dilation, 1))
        a21 = plain_act('act2_1', 'conv2_1', z21)
        y = tail('norm2', act, conv('conv2_2', a21, padding=(0, dilation), dilation=(1, dilation)), identity_path(),
                 scale)
        order = None
    out = {'y': y, 'margins': margins}
    grads = {}

    def back_tail(name, g):
        r = tails[name].backward(g)
        grads[f'{name}.weight'], grads[f'{name}.bias'] = r['dgamma'], r['dbeta']
        return r

    def back_conv(name, g):
        gx, gw, gb = convs[name].backward(g)
        grads[f'{name}.weight'] = gw
        if gb is not None:
            grads[f'{name}.bias'] = gb
        return gx

    if order is not None:
        r = back_tail(order[0][0], gy)
        gid = r['gid']
        g = back_conv(order[0][1], r['gx'])
        for norm, cv in order[1:]:
            g = back_conv(cv, back_tail(norm, g)['gx'])
    else:
        r = back_tail('norm2', gy)
        gid = r['gid']
        g = back_conv('conv2_2', r['gx'])
        g = back_conv('conv2_1', act_backward(g, z21, a21, act))
        g = back_conv('conv1_2', back_tail('norm1', g)['gx'])
        g = back_conv('conv1_1', act_backward(g, z11, a11, act))
    if has_ds:
        gid = back_conv('downsample.conv', back_tail('downsample.norm', gid)['gx'])
    out['gx'] = g + gid
    for key, val in grads.items():
        out[f'grad/{key}'] = val
    for name, t in tails.items():
        out[f'state/{name}.running_mean'] = t.f['running_mean']
        out[f'state/{name}.running_var'] = t.f['running_var']
    return out
