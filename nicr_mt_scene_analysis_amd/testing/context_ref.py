"""TEST / BENCHMARK INFRASTRUCTURE — never imported by the product path.

The four operations of the context module's hot path (all adaptive average pools, their backward,
resize + concatenation, its backward) written out in float64 on the CPU, the torch formulation the
benchmark compares against, three defective restatements, and the error bounds the tests hold the
kernels (and torch's own float32) to.

Every operation is a pair of small matrices per axis: a pool of `out` cells over `n` pixels is the
0/1 membership matrix M [out, n] of ATen's windows with its row sums (the window lengths); a resize
from `n_in` cells to `n_out` pixels is the weight matrix R [n_out, n_in] whose entries come from
ATen's float32 index arithmetic (the weights are float32 numbers, used here as they are: the
reference differs from a kernel only in how the products and sums are rounded)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24          # unit roundoff of float32
f32 = np.float32


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): the relative error of n float32 roundings in a row"""
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------------------ the matrices
def window_matrix(n: int, out: int, end: str = 'ceil') -> torch.Tensor:
    """M [out, n] float64, M[i, k] = 1 where pixel k lies in window i: floor(i n / out) ..
    ceil((i+1) n / out) - 1.  end='floor' is the defective restatement (window ends by floor)."""
    M = torch.zeros((out, n), dtype=torch.float64)
    for i in range(out):
        lo = (i * n) // out
        hi = -((-(i + 1) * n) // out) if end == 'ceil' else max(((i + 1) * n) // out, lo + 1)
        M[i, lo:hi] = 1.0
    return M


def resize_matrix(n_in: int, n_out: int, mode: str, defect: str = None) -> torch.Tensor:
    """R [n_out, n_in] float64: output pixel d = sum_k R[d, k] * cell k, with ATen's float32 index and
    weight arithmetic (scale = float(n_in) / n_out; align_corners=False).  Defects: 'no_half_pixel'
    (bilinear source d * scale), 'round' (nearest by rounding instead of floor)."""
    R = torch.zeros((n_out, n_in), dtype=torch.float64)
    scale = f32(n_in) / f32(n_out)
    for d in range(n_out):
        if mode == 'nearest':
            v = f32(d) * scale
            src = int(np.floor(v + f32(0.5))) if defect == 'round' else int(np.floor(v))
            R[d, min(src, n_in - 1)] = 1.0
            continue
        if defect == 'no_half_pixel':
            s = f32(d) * scale
        else:       # one fused multiply-add: the double product of two floats is exact
            s = f32(float(scale) * float(f32(d) + f32(0.5)) - 0.5)
        s = f32(0.0) if s < 0 else s
        i0 = min(int(s), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        w1 = min(max(f32(s - f32(i0)), f32(0.0)), f32(1.0))
        w0 = f32(f32(1.0) - w1)
        R[d, i0] += float(w0)
        R[d, i1] += float(w1)
    return R


def _d(t):
    return t.detach().double().cpu()


def _pairs(sizes):
    return [(s, s) if isinstance(s, int) else (int(s[0]), int(s[1])) for s in sizes]


# ------------------------------------------------------------------------------ float64 reference
def pool64(x, sizes, end='ceil'):
    """tuple of float64 [B, C, ph, pw]: adaptive average pools of x"""
    x64 = _d(x)
    H, W = x64.shape[2:]
    out = []
    for ph, pw in _pairs(sizes):
        Mh, Mw = window_matrix(H, ph, end), window_matrix(W, pw, end)
        area = Mh.sum(1)[:, None] * Mw.sum(1)[None, :]
        out.append(torch.einsum('ih,bchw,jw->bcij', Mh, x64, Mw) / area)
    return tuple(out)


def pool_backward64(gps, x_shape, sizes, end='ceil'):
    """float64 gx [B, C, H, W] of the pools for the gradients gps (None: not used)"""
    B, C, H, W = x_shape
    gx = torch.zeros((B, C, H, W), dtype=torch.float64)
    for g, (ph, pw) in zip(gps, _pairs(sizes)):
        if g is None:
            continue
        Mh, Mw = window_matrix(H, ph, end), window_matrix(W, pw, end)
        area = Mh.sum(1)[:, None] * Mw.sum(1)[None, :]
        gx += torch.einsum('ih,bcij,jw->bchw', Mh, _d(g) / area, Mw)
    return gx


def upcat64(x, ys, mode, defect=None):
    """float64 [B, C + sum Cr, H, W]: x, then every y resized to x's H x W"""
    x64 = _d(x)
    H, W = x64.shape[2:]
    parts = [x64]
    for y in ys:
        Rh = resize_matrix(y.shape[2], H, mode, defect)
        Rw = resize_matrix(y.shape[3], W, mode, defect)
        parts.append(torch.einsum('hp,bcpq,wq->bchw', Rh, _d(y), Rw))
    return torch.cat(parts, 1)


def upcat_backward64(g_out, n_channels_x, branch_shapes, mode, defect=None):
    """tuple of float64 gradients of the branches for the upstream gradient g_out"""
    g64 = _d(g_out)
    H, W = g64.shape[2:]
    out, c0 = [], int(n_channels_x)
    for (_, cr, ph, pw) in branch_shapes:
        Rh, Rw = resize_matrix(ph, H, mode, defect), resize_matrix(pw, W, mode, defect)
        out.append(torch.einsum('hp,bchw,wq->bcpq', Rh, g64[:, c0:c0 + cr], Rw))
        c0 += cr
    return tuple(out)


def reference64(x, sizes, ys, mode, g_out=None, gps=None):
    """all four operations from the given (already dtype-rounded) tensors -> dict: 'pooled' (tuple),
    'cat'; with g_out 'gys' (tuple); with gps 'gx_pool'"""
    out = {'pooled': pool64(x, sizes), 'cat': upcat64(x, ys, mode)}
    if g_out is not None:
        out['gys'] = upcat_backward64(g_out, x.shape[1], [tuple(y.shape) for y in ys], mode)
    if gps is not None:
        out['gx_pool'] = pool_backward64(gps, tuple(x.shape), sizes)
    return out


# ------------------------------------------------------------------------------ bounds
def _out_rounding(expected64, err64, dtype):
    """one rounding to nearest of a result that is within err of `expected`: u (|e| + err) with
    u = 2^-8 (bfloat16) / 2^-11 (float16), never below half the format's smallest step; 0 for float32"""
    if dtype == torch.float32:
        return torch.zeros_like(expected64)
    u, floor = (2.0 ** -8, 2.0 ** -134) if dtype == torch.bfloat16 else (2.0 ** -11, 2.0 ** -25)
    return (u * (expected64.abs() + err64)).clamp_min(floor)


def _with_rounding(expected64, err64, dtype):
    return err64 + _out_rounding(expected64, err64, dtype)


def bounds(x, sizes, ys, mode, g_out=None, gps=None, dtype=torch.float32):
    """Error bounds against `reference64` for a float32 evaluation in ANY order of summation, then one
    rounding to `dtype`.  With u = 2^-24 and gamma_n = n u / (1 - n u):
      pooled   a window of n pixels: n - 1 additions (n from 0) and one division, or two successive
               divisions by the window's height and width (ATen's evaluation on some devices)
                   gamma_(n+1) * sum|x| / area
      gx_pool  m cells over a pixel (all bins): one or two divisions each, m - 1 additions (m from 0)
                   gamma_(m+1) * sum |gp| / area
      cat      channels of x: 0 (a copy).  nearest: 0 (a copy).  bilinear: each of the four terms
               passes at most 4 roundings (two products, two sums; a product of the two weights
               first in other evaluation orders)
                   gamma_4 * sum_k w_k |y_k|
      gys      a cell read by n output pixels: two products per term and n - 1 additions (n from 0)
                   gamma_(n+2) * sum |g| wy wx        (nearest: the products are exact, gamma_n)
    each plus the rounding of the result to a half dtype.  A zero bound admits only the exact value.
    -> dict like reference64's."""
    ref = reference64(x, sizes, ys, mode, g_out, gps)
    ax = _d(x).abs()
    B, C, H, W = ax.shape
    out = {}
    pooled = []
    for (ph, pw), r in zip(_pairs(sizes), ref['pooled']):
        Mh, Mw = window_matrix(H, ph), window_matrix(W, pw)
        area = Mh.sum(1)[:, None] * Mw.sum(1)[None, :]
        e = gamma(area + 1) * torch.einsum('ih,bchw,jw->bcij', Mh, ax, Mw) / area
        pooled.append(_with_rounding(r, e, dtype))
    out['pooled'] = tuple(pooled)
    parts = [torch.zeros_like(ax)]
    for y in ys:
        Rh, Rw = resize_matrix(y.shape[2], H, mode), resize_matrix(y.shape[3], W, mode)
        s = torch.einsum('hp,bcpq,wq->bchw', Rh, _d(y).abs(), Rw)
        parts.append(s * (gamma(4) if mode == 'bilinear' else 0.0))
    e = torch.cat(parts, 1)
    if mode == 'bilinear':      # only blended values are rounded again; copies are exact in every dtype
        e = torch.cat([parts[0]] + [_with_rounding(ref['cat'][:, C:], e[:, C:], dtype)], 1)
    out['cat'] = e
    if g_out is not None:
        ag = _d(g_out).abs()
        gys, c0 = [], C
        for y, r in zip(ys, ref['gys']):
            cr, ph, pw = y.shape[1:]
            Rh, Rw = resize_matrix(ph, H, mode), resize_matrix(pw, W, mode)
            n = (Rh > 0).sum(0).double()[:, None] * (Rw > 0).sum(0).double()[None, :]     # readers of a cell
            s = torch.einsum('hp,bchw,wq->bcpq', Rh, ag[:, c0:c0 + cr], Rw)
            e = gamma(n + (2 if mode == 'bilinear' else 0)) * s
            gys.append(_with_rounding(r, e, dtype))
            c0 += cr
        out['gys'] = tuple(gys)
    if gps is not None:
        m = torch.zeros((H, W), dtype=torch.float64)
        s = torch.zeros((B, C, H, W), dtype=torch.float64)
        for g, (ph, pw) in zip(gps, _pairs(sizes)):
            if g is None:
                continue
            Mh, Mw = window_matrix(H, ph), window_matrix(W, pw)
            area = Mh.sum(1)[:, None] * Mw.sum(1)[None, :]
            m += Mh.sum(0)[:, None] * Mw.sum(0)[None, :]
            s += torch.einsum('ih,bcij,jw->bchw', Mh, _d(g).abs() / area, Mw)
        out['gx_pool'] = _with_rounding(ref['gx_pool'], gamma(m + 1) * s, dtype)
    return out


def worst_ratio(got, expected64, bound64) -> float:
    """max |got - expected| / bound; a zero bound admits only an exact result"""
    err = (got.detach().double().cpu().reshape(expected64.shape) - expected64).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound64)
    return float(ratio.max())


# ------------------------------------------------------------------------------ torch formulation
def torch_pool(x, sizes):
    return tuple(F.adaptive_avg_pool2d(x, s) for s in _pairs(sizes))


def torch_upcat(x, ys, mode):
    """what the reference runs: n interpolates and one cat"""
    kw = {'mode': 'nearest'} if mode == 'nearest' else {'mode': 'bilinear', 'align_corners': False}
    return torch.cat([x] + [F.interpolate(y, (int(x.shape[2]), int(x.shape[3])), **kw) for y in ys], 1)


def make_inputs(B, C, cr, hw, sizes, seed, dtype=torch.float32, integer=False):
    """seeded x [B, C, H, W], ys (one [B, cr, ph, pw] per size), g_out [B, C + n cr, H, W], gps (one
    [B, C, ph, pw] per size), all rounded to `dtype`; N(0, 1), or integers in -8..8 with `integer`"""
    gen = torch.Generator().manual_seed(seed)
    H, W = hw

    def draw(shape):
        if integer:
            return torch.randint(-8, 9, shape, generator=gen).to(dtype)
        return torch.randn(shape, generator=gen, dtype=torch.float64).to(dtype)

    sz = _pairs(sizes)
    x = draw((B, C, H, W))
    ys = tuple(draw((B, cr, ph, pw)) for ph, pw in sz)
    g_out = draw((B, C + cr * len(sz), H, W))
    gps = tuple(draw((B, C, ph, pw)) for ph, pw in sz)
    return x, ys, g_out, gps


def is_power_of_two_geometry(hw, sizes) -> bool:
    """every window area and resize ratio a power of two (the condition of the exact tier)"""
    return all(n % s == 0 and math.log2(n // s).is_integer() for n, pair in zip(hw, zip(*_pairs(sizes)))
               for s in pair)
