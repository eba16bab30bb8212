"""TEST / BENCHMARK INFRASTRUCTURE — never imported by the product path.

The fused step of the dense decoders, `Upsampling(mode)(x) + skip`, in float64 on the CPU, the torch
composition the benchmark compares against, and the error bounds the tests hold the kernel (and torch's own
float32) to.  Nearest and bilinear are a pair of weight matrices per axis (`context_ref.resize_matrix`: ATen's
float32 index and weight arithmetic, the weights used as they are), the learned modes the formulation of
`upsampling_ref`."""
import torch
import torch.nn.functional as F

from . import upsampling_ref as UR
from .context_ref import _d
from .context_ref import gamma
from .context_ref import resize_matrix
from .context_ref import worst_ratio       # noqa: F401  (the tests take it from here)

U = UR.U
MODES = ('nearest', 'bilinear', 'learned-3x3', 'learned-3x3-zeropad')
# the shapes of the bounds tier (tests/test_up_add.py; tests/test_up_add_host.py holds torch's float32 to the same
# bounds on the same inputs): the vector route of every dtype with a tile border, and an odd width with two of them
BOUNDS_SHAPES = ((2, 3, 9, 12), (2, 3, 17, 7))


def bounds_seed(shape) -> int:
    return 500 + sum(shape)


def is_learned(mode: str) -> bool:
    return mode.startswith('learned-3x3')


def up64(x, mode, weight=None, bias=None, defect=None):
    """float64 u = up(x) [B, C, 2h, 2w] from the given (already dtype-rounded) tensors.  `defect`: a defective
    restatement for the tests of the bounds ('no_half_pixel': bilinear source d * scale, `resize_matrix`'s)"""
    x64 = _d(x)
    if is_learned(mode):
        return UR.torch_formulation(x64, _d(weight), None if bias is None else _d(bias), mode.endswith('zeropad'))
    h, w = x64.shape[2:]
    Rh, Rw = resize_matrix(h, 2 * h, mode, defect), resize_matrix(w, 2 * w, mode, defect)
    return torch.einsum('hp,bcpq,wq->bchw', Rh, x64, Rw)


def reference64(x, skip, mode, weight=None, bias=None, defect=None):
    """float64 y = up(x) + skip"""
    return up64(x, mode, weight, bias, defect) + _d(skip)


def bounds(x, skip, mode, weight=None, bias=None, dtype=torch.float32):
    """The error bound of y against `reference64` for float32 arithmetic and one rounding to `dtype`
    (u = 2^-24, gamma_n = n u / (1 - n u), r = half an ulp of `dtype` at the expected value, 0 for float32):
      nearest    one addition:                                       u |y| + r
      bilinear   each of the four terms passes at most 4 roundings (two products, two sums), the addition
                 of the skip is a fifth:                             gamma_5 (sum_k w_k |x_k| + |skip|) + r
      learned    12 u M for u (`upsampling_ref.bounds`: M the formula on |x|, |W|, |b|), the addition of the
                 skip one more rounding of everything:               13 u (M + |skip|) + r"""
    y64 = reference64(x, skip, mode, weight, bias)
    r = UR.half_ulp(y64, dtype)
    a_skip = _d(skip).abs()
    if mode == 'nearest':
        return U * y64.abs() + r
    if mode == 'bilinear':
        return gamma(5) * (up64(_d(x).abs(), mode) + a_skip) + r
    M = up64(_d(x).abs(), mode, _d(weight).abs(), None if bias is None else _d(bias).abs())
    return 13 * U * (M + a_skip) + r


def torch_up(x, mode, weight=None, bias=None):
    """u of the reference's `Upsampling` as torch ops, in x's dtype on x's device"""
    if is_learned(mode):
        return UR.torch_formulation(x, weight.to(x.dtype), None if bias is None else bias.to(x.dtype),
                                    mode.endswith('zeropad'))
    return F.interpolate(x, scale_factor=2., mode=mode, align_corners=False if mode == 'bilinear' else None)


def torch_up_add(x, skip, mode, weight=None, bias=None):
    """what the reference runs: the upsampling, then `torch.add(skip, u)` (two passes, two roundings)"""
    return torch.add(skip, torch_up(x, mode, weight, bias))


def make_inputs(shape, dtype, seed, integer=False, bias=True):
    """seeded (x [B, C, h, w], skip and gy [B, C, 2h, 2w] rounded to `dtype`, weight [C, 1, 3, 3], bias [C] or
    None): N(0, 1) with 0.25 N(0, 1) weights, or, with `integer`, integers in -8..8 and k/16 weights and bias
    (every product and every sum of the four modes is then exact in float32)"""
    B, C, h, w = shape
    gen = torch.Generator().manual_seed(seed)
    if integer:
        x = torch.randint(-8, 9, (B, C, h, w), generator=gen).to(dtype)
        skip = torch.randint(-8, 9, (B, C, 2 * h, 2 * w), generator=gen).to(dtype)
        gy = torch.randint(-8, 9, (B, C, 2 * h, 2 * w), generator=gen).to(dtype)
        wt = torch.randint(-8, 9, (C, 1, 3, 3), generator=gen).float() / 16
        b = torch.randint(-8, 9, (C,), generator=gen).float() / 16
    else:
        x = torch.randn((B, C, h, w), generator=gen).to(dtype)
        skip = torch.randn((B, C, 2 * h, 2 * w), generator=gen).to(dtype)
        gy = torch.randn((B, C, 2 * h, 2 * w), generator=gen).to(dtype)
        wt = torch.randn((C, 1, 3, 3), generator=gen) * 0.25
        b = torch.randn((C,), generator=gen)
    return x, skip, gy, wt, (b if bias else None)
