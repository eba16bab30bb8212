"""TEST / BENCHMARK INFRASTRUCTURE — never imported by the product path.

The Swin encoder-decoder fusion (LayerNorm over C, NHWC -> NCHW, optional addition) and its gradients
written out in float64, the torch formulation the benchmark compares against, the one-pass-variance
control, and the error bounds the tests hold the kernels (and torch's own float32) to."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24          # unit roundoff of float32


def torch_formulation(x, gamma, beta, eps, x_dec=None, contiguous=True):
    """layer_norm -> permute -> add (with x_dec) / contiguous (without): what the reference runs, the
    copy being the one a convolution's NCHW path takes"""
    y = F.layer_norm(x, (x.shape[-1],), gamma, beta, eps).permute(0, 3, 1, 2)
    if x_dec is not None:
        return torch.add(y, x_dec)
    return y.contiguous() if contiguous else y


def reference64(x, gamma, beta, eps, add=None, gy=None):
    """float64 on the CPU from the given (already dtype-rounded) tensors.  x [B, ..., C]; add, gy
    [B, C, ...].  -> dict: y [B, C, ...]; with gy also gx (x's shape), ggamma, gbeta [C]; and the
    row quantities the bounds need (mean, rstd, xh as [B, P(, C)])."""
    x64 = x.detach().double().cpu()
    B, C = x64.shape[0], x64.shape[-1]
    spatial = tuple(x64.shape[1:-1])
    r = x64.reshape(B, -1, C)
    g64, b64 = gamma.detach().double().cpu(), beta.detach().double().cpu()
    mean = r.mean(-1, keepdim=True)
    var = ((r - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (r - mean) * rstd
    n = xh * g64 + b64
    y = n.transpose(1, 2)
    out = {'mean': mean[..., 0], 'rstd': rstd[..., 0], 'xh': xh, 'n': n}
    if add is not None:
        y = y + add.detach().double().cpu().reshape(B, C, -1)
    out['y'] = y.reshape((B, C) + spatial).contiguous()
    if gy is not None:
        g = gy.detach().double().cpu().reshape(B, C, -1).transpose(1, 2)       # [B, P, C]
        a = g * g64
        A1, A2 = a.mean(-1, keepdim=True), (a * xh).mean(-1, keepdim=True)
        out.update(gy_rows=g, a=a, A1=A1, A2=A2)
        out['gx'] = (rstd * (a - A1 - xh * A2)).reshape(x64.shape)
        out['ggamma'] = (g * xh).sum((0, 1))
        out['gbeta'] = g.sum((0, 1))
    return out


def one_pass_variance_f32(x, gamma, beta, eps, gy=None):
    """the control: float32 with var = E[x^2] - mean^2 -> (y, gx) float32, gx None without gy"""
    r = x.detach().float().cpu()
    mean = r.mean(-1, keepdim=True)
    var = (r * r).mean(-1, keepdim=True) - mean * mean
    rstd = 1.0 / torch.sqrt(var.clamp_min(0) + eps)
    xh = (r - mean) * rstd
    y = (xh * gamma.float().cpu() + beta.float().cpu()).movedim(-1, 1).contiguous()
    gx = None
    if gy is not None:
        a = gy.detach().float().cpu().movedim(1, -1) * gamma.float().cpu()
        gx = rstd * (a - a.mean(-1, keepdim=True) - xh * (a * xh).mean(-1, keepdim=True))
    return y, gx


def _out_rounding(expected64, dtype):
    """one rounding to nearest of the output: u |e| with u = 2^-8 (bfloat16) / 2^-11 (float16), and
    never below half the format's smallest step (float16 subnormals); 0 for float32"""
    if dtype == torch.float32:
        return torch.zeros_like(expected64)
    u, floor = (2.0 ** -8, 2.0 ** -134) if dtype == torch.bfloat16 else (2.0 ** -11, 2.0 ** -25)
    return (u * expected64.abs()).clamp_min(floor)


def bounds(x, gamma, beta, eps, add=None, gy=None, dtype_y=torch.float32, dtype_x=torch.float32):
    """Error bounds against `reference64` for a float32 evaluation that follows the arithmetic
    contract of include/nmsa.h (sums over C as trees of depth L = ceil(log2 C) + 2, two-pass variance,
    correctly rounded division and square root), u = 2^-24.  Per row:
      Em  = (L+1) u mean|x|                 error of the mean
      Er  = (L/2+6) u + (rstd Em)^2 / 2     relative error of rstd
      Exh = rstd Em + |xh| Er               error of xh
    y:      |gamma| Exh + u (|xh gamma| + |n|) (+ u |y| with add) + the output rounding;
            n = xh gamma + beta (the two roundings of the scale and the shift, each at the magnitude of
            its own result: `2u|y|` understates them where beta cancels the scaled value)
    gx:     rstd dt + |gx| (Er + 2u) + the output rounding,
            dt = 2u|a| + dA1 + |xh| dA2 + Exh |A2| + 3u (|A1| + |xh A2|),
            dA1 = (L+2) u mean|a|,  dA2 = (L+3) u mean|a xh| + mean(|a| Exh)
    ggamma: (N+2) u sum|gy xh| + sum(|gy| Exh), N = B*P rows (the order-free bound of a sum of N terms)
    gbeta:  (N+2) u sum|gy|
    -> dict of float64 tensors shaped like the results."""
    ref = reference64(x, gamma, beta, eps, add, gy)
    x64 = x.detach().double().cpu()
    B, C = x64.shape[0], x64.shape[-1]
    r = x64.reshape(B, -1, C)
    g64 = gamma.detach().double().cpu().abs()
    L = math.ceil(math.log2(C)) + 2 if C > 1 else 2
    rstd, xh = ref['rstd'][..., None], ref['xh']
    Em = (L + 1) * U * r.abs().mean(-1, keepdim=True)
    Er = (L / 2 + 6) * U + (rstd * Em) ** 2 / 2
    Exh = rstd * Em + xh.abs() * Er
    ey = g64 * Exh + U * ((xh * g64).abs() + ref['n'].abs())
    ey = ey.transpose(1, 2).reshape(ref['y'].shape)
    if add is not None:
        ey = ey + U * ref['y'].abs()
    out = {'y': ey + _out_rounding(ref['y'], dtype_y)}
    if gy is not None:
        a, A1, A2, g = ref['a'], ref['A1'], ref['A2'], ref['gy_rows']
        dA1 = (L + 2) * U * a.abs().mean(-1, keepdim=True)
        dA2 = (L + 3) * U * (a * xh).abs().mean(-1, keepdim=True) + (a.abs() * Exh).mean(-1, keepdim=True)
        dt = 2 * U * a.abs() + dA1 + xh.abs() * dA2 + Exh * A2.abs() + 3 * U * (A1.abs() + (xh * A2).abs())
        gx = ref['gx'].reshape(B, -1, C)
        egx = (rstd * dt + gx.abs() * (Er + 2 * U)).reshape(ref['gx'].shape)
        out['gx'] = egx + _out_rounding(ref['gx'], dtype_x)
        N = r.shape[0] * r.shape[1]
        out['ggamma'] = (N + 2) * U * (g * xh).abs().sum((0, 1)) + (g.abs() * Exh).sum((0, 1))
        out['gbeta'] = (N + 2) * U * g.abs().sum((0, 1))
    return out


def worst_ratio(got, expected64, bound64) -> float:
    """max |got - expected| / bound; a zero bound admits only an exact result"""
    err = (got.detach().double().cpu().reshape(expected64.shape) - expected64).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound64)
    return float(ratio.max())


# the input classes of the bounds: name -> x = offset + scale * N(0, 1); the last is forward only
INPUT_CLASSES = {'normal': (0.0, 1.0), 'small': (0.0, 1e-3), 'offset_neg': (-50.0, 5.0),
                 'offset_pos': (3.0, 0.5), 'offset_1000': (1000.0, 1.0)}
FORWARD_ONLY_CLASSES = ('offset_1000',)


def make_inputs(kind, B, P, C, seed, dtype=torch.float32):
    """seeded x [B, P, C] of an input class (rounded to `dtype`), gamma, beta float32 [C], gy, add
    float32 [B, C, P] (N(0, 1); the caller rounds them to the dtype it tests)"""
    gen = torch.Generator().manual_seed(seed)
    off, scale = INPUT_CLASSES[kind]
    x = (off + scale * torch.randn((B, P, C), generator=gen, dtype=torch.float64)).to(dtype)
    gamma = 1.0 + 0.25 * torch.randn((C,), generator=gen)
    beta = 0.5 * torch.randn((C,), generator=gen)
    gy = torch.randn((B, C, P), generator=gen)
    add = torch.randn((B, C, P), generator=gen)
    return x, gamma, beta, gy, add
