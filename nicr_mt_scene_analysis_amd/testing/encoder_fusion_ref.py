"""TEST / BENCHMARK INFRASTRUCTURE — never imported by the product path.

The SE-weighted add of the encoder RGB-D fusion (squeeze, excitation, weighted add) and all of its
gradients written out in float64 on the CPU, one function per kernel and `reference64` for the chain;
the torch formulation the fallback comparison and the benchmark use; and the error bounds the tests
hold the kernels (and torch's own float32) to.

Conventions.  Per-modality quantities are stacked, rgb first: s, w, gw, gz2, gs [2, B, C]; z1, h, gz1
[2, B, R], R = C // 16.  `params` = (params_rgb, params_depth), each (W1 [R, C] or [R, C, 1, 1], b1 [R],
W2 [C, R] or [C, R, 1, 1], b2 [C]).  `act` is 'relu' or 'silu'.

Bounds.  They hold for a float32 evaluation under the arithmetic contract of include/nmsa.h
(nmsa_sefuse_*): every sum in ANY order (gamma_n = n u / (1 - n u) for n roundings in a row, u = 2^-24),
every product, quotient and sum rounded once, one rounding of a map to its dtype.  Each per-kernel
bound takes the errors of the kernel's inputs; `bounds` chains them through the whole module.
The one constant that does not follow from the contract is the error of the device's `expf` inside
the sigmoid and SiLU.  Its source: no documented ulp figure of the device library is relied on;
`sigmoid_roundoff` measures what torch's own float32 sigmoid needs on the CPU against float64 over
the very pre-activations of the call, in units of u relative to the result, and DOUBLES it; it is
never taken below 3 (the three roundings of 1 / (1 + expf(-z)) with a correctly rounded expf).
Nothing here was tuned to a kernel."""
import torch
import torch.nn.functional as F

from .context_ref import _d
from .context_ref import _with_rounding
from .context_ref import gamma
from .context_ref import worst_ratio       # noqa: F401  (the tests take it from here)

U = 2.0 ** -24
DEFECTS = ('mean', 'no_gs', 'sig_grad')


def params64(params):
    """((W1 [R, C], b1, W2 [C, R], b2) float64 on the CPU) per modality"""
    out = []
    for W1, b1, W2, b2 in params:
        W1, W2 = _d(W1), _d(W2)
        out.append((W1.reshape(W1.shape[0], W1.shape[1]), _d(b1), W2.reshape(W2.shape[0], W2.shape[1]), _d(b2)))
    return tuple(out)


def _sig(z):
    return 1.0 / (1.0 + torch.exp(-z))


def _act(z, act):
    return z.clamp_min(0.0) if act == 'relu' else z * _sig(z)


def _act_grad(z, act):
    if act == 'relu':
        return 1.0 - (z <= 0).double()                              # ATen's threshold backward: 1 at a NaN z
    sg = _sig(z)
    return sg * (1.0 + z * (1.0 - sg))


def sigmoid_roundoff(*pre_activations) -> float:
    """K: the float32 sigmoid is within K u |sigmoid| of the true one (see the module docstring)"""
    worst = 0.0
    for z in pre_activations:
        z32 = _d(z).float()
        exact = _sig(z32.double())
        err = (torch.sigmoid(z32).double() - exact).abs() / (U * exact)
        worst = max(worst, float(err.max())) if err.numel() else worst
    return max(2.0 * worst, 3.0)


# ------------------------------------------------------------------------------ the six kernels
def squeeze64(x_rgb, x_depth, defect=None):
    x = torch.stack((_d(x_rgb), _d(x_depth)))
    n = x.shape[-1] * x.shape[-2]
    return x.sum((-1, -2)) / (n - 1 if defect == 'mean' else n)


def squeeze_bound(x_rgb, x_depth):
    """n - 1 additions and the division: gamma_(n+1) mean|x|"""
    x = torch.stack((_d(x_rgb), _d(x_depth))).abs()
    n = x.shape[-1] * x.shape[-2]
    return gamma(n + 1) * x.sum((-1, -2)) / n


def excite64(s, params, act):
    """dict z1, h [2, B, R], z2, w [2, B, C]"""
    s64, z1, h, z2 = _d(s), [], [], []
    for m, (W1, b1, W2, b2) in enumerate(params64(params)):
        z1.append(s64[m] @ W1.t() + b1)
        h.append(_act(z1[-1], act))
        z2.append(h[-1] @ W2.t() + b2)
    z1, h, z2 = torch.stack(z1), torch.stack(h), torch.stack(z2)
    return {'z1': z1, 'h': h, 'z2': z2, 'w': _sig(z2)}


def excite_bound(s, params, act, Es=None):
    """z1: sum|W1| Es + gamma_(C+2) (sum|W1 s| + |b1|)    (C products, C - 1 additions, the bias)
    h:  relu Ez1;  silu 1.1 Ez1 + (K + 1) u |h|            (|silu'| <= 1.1; the sigmoid, the product)
    z2: sum|W2| Eh + gamma_(R+2) (sum|W2 h| + |b2|)
    w:  w (1 - w) exp(Ez2) Ez2 + K u w                      (the mean value theorem; the sigmoid)
    -> dict z1, h, w (bounds) and K"""
    r = excite64(s, params, act)
    s64 = _d(s)
    Es = torch.zeros_like(s64) if Es is None else Es
    K = sigmoid_roundoff(r['z2'], r['z1']) if act == 'silu' else sigmoid_roundoff(r['z2'])
    Ez1, Eh, Ew = [], [], []
    for m, (W1, b1, W2, b2) in enumerate(params64(params)):
        C, R = W1.shape[1], W1.shape[0]
        Ez1.append(Es[m] @ W1.abs().t() + gamma(C + 2) * (s64[m].abs() @ W1.abs().t() + b1.abs()))
        Eh.append(Ez1[-1] if act == 'relu' else 1.1 * Ez1[-1] + (K + 1) * U * r['h'][m].abs())
        Ez2 = Eh[-1] @ W2.abs().t() + gamma(R + 2) * (r['h'][m].abs() @ W2.abs().t() + b2.abs())
        w = r['w'][m]
        Ew.append(w * (1 - w) * torch.exp(Ez2) * Ez2 + K * U * w)
    return {'z1': torch.stack(Ez1), 'h': torch.stack(Eh), 'w': torch.stack(Ew), 'K': K}


def scale_add64(x_rgb, x_depth, w):
    w64 = _d(w)
    return _d(x_rgb) * w64[0][:, :, None, None] + _d(x_depth) * w64[1][:, :, None, None]


def scale_add_bound(x_rgb, x_depth, w, Ew=None, dtype=torch.float32):
    """|x_rgb| Ew_rgb + |x_depth| Ew_depth + gamma_2 (|x_rgb w_rgb| + |x_depth w_depth|) and the
    rounding to `dtype` (each term passes its product and the sum)"""
    w64 = _d(w)
    Ew = torch.zeros_like(w64) if Ew is None else Ew
    ar, ad = _d(x_rgb).abs(), _d(x_depth).abs()
    e = (ar * Ew[0][:, :, None, None] + ad * Ew[1][:, :, None, None]
         + gamma(2) * (ar * w64[0].abs()[:, :, None, None] + ad * w64[1].abs()[:, :, None, None]))
    return _with_rounding(scale_add64(x_rgb, x_depth, w), e, dtype)


def weight_grad64(gy, x_rgb, x_depth):
    g = _d(gy)
    return torch.stack(((g * _d(x_rgb)).sum((-1, -2)), (g * _d(x_depth)).sum((-1, -2))))


def weight_grad_bound(gy, x_rgb, x_depth):
    """n products and n - 1 additions: gamma_(n+1) sum|gy x|"""
    g = _d(gy).abs()
    n = g.shape[-1] * g.shape[-2]
    return gamma(n + 1) * torch.stack(((g * _d(x_rgb).abs()).sum((-1, -2)), (g * _d(x_depth).abs()).sum((-1, -2))))


def excite_backward64(gw, w, z1, params, act, defect=None):
    """dict gz2, gs [2, B, C], gz1, h, gh [2, B, R]"""
    gw64, w64, z64 = _d(gw), _d(w), _d(z1)
    gz2 = gw64 * w64 if defect == 'sig_grad' else gw64 * w64 * (1.0 - w64)
    gh, gs = [], []
    for m, (W1, b1, W2, b2) in enumerate(params64(params)):
        gh.append(gz2[m] @ W2)
    gh = torch.stack(gh)
    # ReLU: ATen's threshold backward selects (0 at z <= 0 whatever gh is), SiLU multiplies
    gz1 = torch.where(z64 <= 0, torch.zeros_like(gh), gh) if act == 'relu' else gh * _act_grad(z64, act)
    for m, (W1, b1, W2, b2) in enumerate(params64(params)):
        gs.append(gz1[m] @ W1)
    return {'gz2': gz2, 'gh': gh, 'gz1': gz1, 'gs': torch.stack(gs), 'h': _act(z64, act)}


def excite_backward_bound(gw, w, z1, params, act, Egw=None, Ew=None, Ez1=None, K=None):
    """gz2: w (1 - w) Egw + |gw| |1 - 2 w| Ew + |gw| Ew^2 + gamma_3 |gz2|     (1 - w and two products)
    gh:  sum|W2| Egz2 + gamma_(C+1) sum|W2 gz2|
    gz1: |act'| Egh + (|gh| + Egh) Ea + u |gz1|, Ea the error of act'(z1):
         relu: 1 where |z1| <= Ez1 (the step may fall on the other side), else 0
         silu: 0.5 Ez1 + sg |z| (K sg + 2 (1 - sg)) u + (K + 2) u |act'|    (|silu''| <= 0.5, then the
               roundings of sg (1 + z (1 - sg)))
    gs:  sum|W1| Egz1 + gamma_(R+1) sum|W1 gz1|
    h:   as in `excite_bound`
    -> dict gz2, gz1, gs, h"""
    r = excite_backward64(gw, w, z1, params, act)
    gw64, w64, z64 = _d(gw), _d(w), _d(z1)
    zero = torch.zeros_like
    Egw, Ew, Ez1 = (zero(gw64) if Egw is None else Egw, zero(w64) if Ew is None else Ew,
                    zero(z64) if Ez1 is None else Ez1)
    K = (sigmoid_roundoff(z64) if act == 'silu' else 3.0) if K is None else K
    Egz2 = (w64 * (1 - w64) * Egw + gw64.abs() * (1 - 2 * w64).abs() * Ew + gw64.abs() * Ew * Ew
            + gamma(3) * r['gz2'].abs())
    da = _act_grad(z64, act).abs()
    if act == 'relu':
        Ea = (z64.abs() <= Ez1).double() * (Ez1 > 0)
        Eh = Ez1
    else:
        sg = _sig(z64)
        Ea = 0.5 * Ez1 + sg * z64.abs() * (K * sg + 2 * (1 - sg)) * U + (K + 2) * U * da
        Eh = 1.1 * Ez1 + (K + 1) * U * r['h'].abs()
    Egz1, Egs = [], []
    for m, (W1, b1, W2, b2) in enumerate(params64(params)):
        C, R = W1.shape[1], W1.shape[0]
        Egh = Egz2[m] @ W2.abs() + gamma(C + 1) * (r['gz2'][m].abs() @ W2.abs())
        Egz1.append(da[m] * Egh + (r['gh'][m].abs() + Egh) * Ea[m] + U * r['gz1'][m].abs())
        Egs.append(Egz1[-1] @ W1.abs() + gamma(R + 1) * (r['gz1'][m].abs() @ W1.abs()))
    return {'gz2': Egz2, 'gz1': torch.stack(Egz1), 'gs': torch.stack(Egs), 'h': Eh}


def apply64(gy, w, gs, defect=None):
    """(gx_rgb, gx_depth) float64"""
    g, w64, gs64 = _d(gy), _d(w), _d(gs)
    n = g.shape[-1] * g.shape[-2]
    if defect == 'no_gs':
        gs64 = torch.zeros_like(gs64)
    return tuple(g * w64[m][:, :, None, None] + gs64[m][:, :, None, None] / n for m in range(2))


def apply_bound(gy, w, gs, Ew=None, Egs=None, dtype=torch.float32):
    """|gy| Ew + Egs / n + gamma_2 (|gy w| + |gs| / n) and the rounding to `dtype`"""
    g, w64, gs64 = _d(gy).abs(), _d(w), _d(gs)
    n = g.shape[-1] * g.shape[-2]
    Ew = torch.zeros_like(w64) if Ew is None else Ew
    Egs = torch.zeros_like(gs64) if Egs is None else Egs
    ref = apply64(gy, w, gs)
    out = []
    for m in range(2):
        e = (g * Ew[m][:, :, None, None] + Egs[m][:, :, None, None] / n
             + gamma(2) * (g * w64[m].abs()[:, :, None, None] + gs64[m].abs()[:, :, None, None] / n))
        out.append(_with_rounding(ref[m], e, dtype))
    return tuple(out)


PARAM_GRADS = ('gW1', 'gb1', 'gW2', 'gb2')


def param_grads64(gz2, gz1, s, h):
    """dict gW1 [2, R, C], gb1 [2, R], gW2 [2, C, R], gb2 [2, C]"""
    gz2, gz1, s, h = _d(gz2), _d(gz1), _d(s), _d(h)
    return {'gW1': gz1.transpose(1, 2) @ s, 'gb1': gz1.sum(1), 'gW2': gz2.transpose(1, 2) @ h, 'gb2': gz2.sum(1)}


def param_grads_bound(gz2, gz1, s, h, Egz2, Egz1, Es, Eh):
    """a sum over the B images of products a b: sum (Ea |b| + |a| Eb + Ea Eb) + gamma_(B+1) sum|a b|;
    the bias gradients: sum Ea + gamma_B sum|a|"""
    gz2, gz1, s, h = _d(gz2).abs(), _d(gz1).abs(), _d(s).abs(), _d(h).abs()
    B = s.shape[1]

    def prod(a, Ea, b, Eb):
        at, Eat = a.transpose(1, 2), Ea.transpose(1, 2)
        return Eat @ b + at @ Eb + Eat @ Eb + gamma(B + 1) * (at @ b)
    return {'gW1': prod(gz1, Egz1, s, Es), 'gb1': Egz1.sum(1) + gamma(B) * gz1.sum(1),
            'gW2': prod(gz2, Egz2, h, Eh), 'gb2': Egz2.sum(1) + gamma(B) * gz2.sum(1)}


# ------------------------------------------------------------------------------ the chain
def reference64(x_rgb, x_depth, params, act, gy=None, defect=None):
    """every forward and (with gy) backward quantity in float64 from the given, already dtype-rounded
    tensors -> dict s, z1, h, w, y; gw, gz2, gz1, gs, gx_rgb, gx_depth, gW1, gb1, gW2, gb2 (stacked per
    modality).  `defect`: one of DEFECTS, a deliberately wrong restatement."""
    out = {'s': squeeze64(x_rgb, x_depth, defect)}
    out.update(excite64(out['s'], params, act))
    out['y'] = scale_add64(x_rgb, x_depth, out['w'])
    if gy is not None:
        out['gw'] = weight_grad64(gy, x_rgb, x_depth)
        out.update(excite_backward64(out['gw'], out['w'], out['z1'], params, act, defect))
        out['gx_rgb'], out['gx_depth'] = apply64(gy, out['w'], out['gs'], defect)
        out.update(param_grads64(out['gz2'], out['gz1'], out['s'], out['h']))
    return out


def bounds(x_rgb, x_depth, params, act, gy=None, dtype=torch.float32):
    """the per-kernel bounds chained through the module -> dict like reference64's (without z2, gh)"""
    ref = reference64(x_rgb, x_depth, params, act, gy)
    out = {'s': squeeze_bound(x_rgb, x_depth)}
    ex = excite_bound(ref['s'], params, act, out['s'])
    out.update(z1=ex['z1'], h=ex['h'], w=ex['w'])
    out['y'] = scale_add_bound(x_rgb, x_depth, ref['w'], out['w'], dtype)
    if gy is not None:
        out['gw'] = weight_grad_bound(gy, x_rgb, x_depth)
        eb = excite_backward_bound(ref['gw'], ref['w'], ref['z1'], params, act, out['gw'], out['w'], out['z1'], ex['K'])
        out.update(gz2=eb['gz2'], gz1=eb['gz1'], gs=eb['gs'])
        out['gx_rgb'], out['gx_depth'] = apply_bound(gy, ref['w'], ref['gs'], out['w'], out['gs'], dtype)
        out.update(param_grads_bound(ref['gz2'], ref['gz1'], ref['s'], ref['h'], out['gz2'], out['gz1'], out['s'],
                                     out['h']))
    return out


# ------------------------------------------------------------------------------ torch formulation
def torch_formulation(x_rgb, x_depth, params, act):
    """the reference's op sequence: per modality adaptive_avg_pool2d, conv 1x1, activation, conv 1x1,
    sigmoid, broadcast multiply; then the add"""
    fn = F.relu if act == 'relu' else F.silu
    parts = []
    for x, (W1, b1, W2, b2) in zip((x_rgb, x_depth), params):
        W1 = W1.reshape(W1.shape[0], W1.shape[1], 1, 1)
        W2 = W2.reshape(W2.shape[0], W2.shape[1], 1, 1)
        wgt = torch.sigmoid(F.conv2d(fn(F.conv2d(F.adaptive_avg_pool2d(x, 1), W1, b1)), W2, b2))
        parts.append(x * wgt)
    return parts[0] + parts[1]


def make_params(C, seed, dtype=torch.float32):
    """seeded (params_rgb, params_depth) with the scale of a default-initialised 1x1 convolution; the
    hidden bias is positive, so that most hidden units are active under ReLU and gs is not all zero"""
    gen = torch.Generator().manual_seed(seed)
    R = C // 16
    out = []
    for _ in range(2):
        W1 = torch.randn((R, C), generator=gen) / C ** 0.5 * 2
        b1 = 0.25 + torch.randn((R,), generator=gen).abs() * 0.5
        W2 = torch.randn((C, R), generator=gen) / R ** 0.5
        b2 = torch.randn((C,), generator=gen) * 0.5
        out.append(tuple(t.to(dtype) for t in (W1, b1, W2, b2)))
    return tuple(out)


def make_inputs(B, C, hw, seed, dtype=torch.float32, integer=False):
    """seeded x_rgb, x_depth, gy [B, C, H, W] rounded to `dtype`: N(0.3, 1) (a mean away from 0, as
    feature maps behind an activation have), or integers in -8..8 with `integer`"""
    gen = torch.Generator().manual_seed(seed)
    shape = (B, C) + tuple(hw)

    def draw(off):
        if integer:
            return torch.randint(-8, 9, shape, generator=gen).to(dtype)
        return (off + torch.randn(shape, generator=gen, dtype=torch.float64)).to(dtype)
    return draw(0.3), draw(0.3), draw(0.0)
