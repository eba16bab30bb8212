"""TEST / BENCHMARK INFRASTRUCTURE — never imported by the product path.

The two operations of the MLP decoders' hot step (every branch resized into the concatenation, and
its backward) written out in float64 on the CPU, the torch composition the benchmark compares
against, and the error bounds the tests hold the kernels (and torch's own float32) to.  A resize is
a pair of weight matrices per axis (`context_ref.resize_matrix`: ATen's float32 index and weight
arithmetic, the weights used as they are)."""
import torch
import torch.nn.functional as F

from .context_ref import _d
from .context_ref import _with_rounding
from .context_ref import gamma
from .context_ref import resize_matrix
from .context_ref import worst_ratio       # noqa: F401  (the tests take it from here)


def out_size(shapes, size=None):
    """(H, W): `size`, by default the largest map"""
    if size is not None:
        return int(size[0]), int(size[1])
    return max(int(s[2]) for s in shapes), max(int(s[3]) for s in shapes)


# ------------------------------------------------------------------------------ float64 reference
def upcat64(ys, mode, defect=None, size=None):
    """float64 [B, sum c_i, H, W]: every y resized to H x W (`out_size`)"""
    H, W = out_size([y.shape for y in ys], size)
    parts = []
    for y in ys:
        Rh = resize_matrix(y.shape[2], H, mode, defect)
        Rw = resize_matrix(y.shape[3], W, mode, defect)
        parts.append(torch.einsum('hp,bcpq,wq->bchw', Rh, _d(y), Rw))
    return torch.cat(parts, 1)


def upcat_backward64(g_out, branch_shapes, mode, defect=None):
    """tuple of float64 gradients of the branches for the upstream gradient g_out"""
    g64 = _d(g_out)
    H, W = g64.shape[2:]
    out, c0 = [], 0
    for (_, c, h, w) in branch_shapes:
        Rh, Rw = resize_matrix(h, H, mode, defect), resize_matrix(w, W, mode, defect)
        out.append(torch.einsum('hp,bchw,wq->bcpq', Rh, g64[:, c0:c0 + c], Rw))
        c0 += c
    return tuple(out)


def reference64(ys, mode, g_out=None, size=None):
    """both operations from the given (already dtype-rounded) tensors -> dict 'cat', with g_out 'gys'"""
    out = {'cat': upcat64(ys, mode, size=size)}
    if g_out is not None:
        out['gys'] = upcat_backward64(g_out, [tuple(y.shape) for y in ys], mode)
    return out


# ------------------------------------------------------------------------------ bounds
def bounds(ys, mode, g_out=None, dtype=torch.float32, size=None):
    """Error bounds against `reference64` for a float32 evaluation in ANY order of summation, then one
    rounding to `dtype` (the reasoning of `context_ref.bounds`).  With u = 2^-24, gamma_n = n u / (1 - n u):
      cat   nearest, or a branch that already has the output size: 0 (a copy).  bilinear: each of the
            four terms passes at most 4 roundings (two products, two sums; a product of the two
            weights first in other evaluation orders)
                gamma_4 * sum_k w_k |y_k|
      gys   a cell read by n output pixels: two products per term and n - 1 additions (n from 0)
                gamma_(n+2) * sum |g| wy wx        (nearest: the products are exact, gamma_n)
    each plus the rounding of the result to a half dtype where a value is computed (not copied).  A zero
    bound admits only the exact value.  -> dict like reference64's."""
    ref = reference64(ys, mode, g_out, size)
    H, W = out_size([y.shape for y in ys], size)
    parts, c0 = [], 0
    for y in ys:
        c = y.shape[1]
        copied = mode == 'nearest' or (y.shape[2], y.shape[3]) == (H, W)
        Rh, Rw = resize_matrix(y.shape[2], H, mode), resize_matrix(y.shape[3], W, mode)
        s = torch.einsum('hp,bcpq,wq->bchw', Rh, _d(y).abs(), Rw)
        parts.append(torch.zeros_like(s) if copied else _with_rounding(ref['cat'][:, c0:c0 + c], gamma(4) * s, dtype))
        c0 += c
    out = {'cat': torch.cat(parts, 1)}
    if g_out is not None:
        ag = _d(g_out).abs()
        gys, c0 = [], 0
        for y, r in zip(ys, ref['gys']):
            c, h, w = y.shape[1:]
            if (h, w) == (H, W):                            # the view of g_out
                gys.append(torch.zeros_like(r))
                c0 += c
                continue
            Rh, Rw = resize_matrix(h, H, mode), resize_matrix(w, W, mode)
            n = (Rh > 0).sum(0).double()[:, None] * (Rw > 0).sum(0).double()[None, :]     # readers of a cell
            s = torch.einsum('hp,bchw,wq->bcpq', Rh, ag[:, c0:c0 + c], Rw)
            gys.append(_with_rounding(r, gamma(n + (2 if mode == 'bilinear' else 0)) * s, dtype))
            c0 += c
        out['gys'] = tuple(gys)
    return out


# ------------------------------------------------------------------------------ torch composition
def torch_upcat(ys, mode, size=None):
    """what the reference runs: one interpolate per branch and one cat"""
    H, W = out_size([y.shape for y in ys], size)
    kw = {'mode': 'nearest'} if mode == 'nearest' else {'mode': 'bilinear', 'align_corners': False}
    return torch.cat([F.interpolate(y, scale_factor=H // int(y.shape[2]), **kw) for y in ys], 1)


def make_inputs(B, channels, factors, hw, seed, dtype=torch.float32, integer=False):
    """seeded ys (one [B, c_i, H / f_i, W / f_i] per branch) and g_out [B, sum c_i, H, W], rounded to
    `dtype`; N(0, 1), or integers in -8..8 with `integer`"""
    gen = torch.Generator().manual_seed(seed)
    H, W = hw

    def draw(shape):
        if integer:
            return torch.randint(-8, 9, shape, generator=gen).to(dtype)
        return torch.randn(shape, generator=gen, dtype=torch.float64).to(dtype)

    ys = tuple(draw((B, c, H // f, W // f)) for c, f in zip(channels, factors))
    return ys, draw((B, sum(channels), H, W))
