"""The 3x3 / stride 2 / padding 1 max pool of include/nmsa.h (nmsa_maxpool3x3s2_*) restated in torch on the
CPU, for the tests: the selection rule spelled out position by position, the one-byte window code, the
conversion between ATen's flat indices and codes, and the backward pass as a gather with float32 sums in the
stated order.  Nothing here calls `max_pool2d`; tests/test_maxpool_ref.py holds it to ATen's CPU float32
`max_pool2d(return_indices=True)` and its autograd, exactly, before any kernel is held to it."""
from typing import Dict, List, Tuple

import torch

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


def out_hw(H: int, W: int) -> Tuple[int, int]:
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def _grids(H: int, W: int):
    Ho, Wo = out_hw(H, W)
    oy = torch.arange(Ho).reshape(Ho, 1).expand(Ho, Wo)
    ox = torch.arange(Wo).reshape(1, Wo).expand(Ho, Wo)
    return oy, ox


def forward(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(y, code) of x [B, C, H, W] (any float dtype; compared as float32, which is exact for the halves): the
    window positions inside the map in row-major order, starting at the first, the choice replaced when
    `val > max or isnan(val)`.  y is gathered from x, so it carries the selected element's bits."""
    B, C, H, W = x.shape
    Ho, Wo = out_hw(H, W)
    xf = x.float().reshape(B * C, H * W)
    oy, ox = _grids(H, W)
    best = torch.zeros((B * C, Ho, Wo))
    pos = torch.zeros((Ho, Wo), dtype=torch.int64).expand(B * C, Ho, Wo).clone()
    code = torch.zeros((B * C, Ho, Wo), dtype=torch.uint8)
    started = torch.zeros((Ho, Wo), dtype=torch.bool)
    for k in range(9):
        r, c = 2 * oy - 1 + k // 3, 2 * ox - 1 + k % 3
        valid = (r >= 0) & (r < H) & (c >= 0) & (c < W)
        flat = (r.clamp(0, H - 1) * W + c.clamp(0, W - 1))
        val = xf[:, flat.reshape(-1)].reshape(B * C, Ho, Wo)
        take = valid & (~started | (val > best) | torch.isnan(val))
        best = torch.where(take, val, best)
        pos = torch.where(take, flat.expand_as(pos), pos)
        code = torch.where(take, torch.full_like(code, k), code)
        started = started | valid
    assert bool(started.all())
    y = x.reshape(B * C, H * W).gather(1, pos.reshape(B * C, -1)).reshape(B, C, Ho, Wo)
    return y, code.reshape(B, C, Ho, Wo)


def code_to_index(code: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """ATen's int64 indices (r * W + c inside the plane) of codes [.., Ho, Wo]"""
    oy, ox = _grids(H, W)
    k = code.long()
    return (2 * oy - 1 + k // 3) * W + (2 * ox - 1 + k % 3)


def index_to_code(index: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """the codes of ATen's indices [.., Ho, Wo]; asserts every index lies in its window"""
    oy, ox = _grids(H, W)
    dr, dc = index // W - (2 * oy - 1), index % W - (2 * ox - 1)
    assert bool(((dr >= 0) & (dr < 3) & (dc >= 0) & (dc < 3)).all())
    return (3 * dr + dc).to(torch.uint8)


def backward_f32(gy: torch.Tensor, code: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """gx [B, C, H, W] in float32: for every input pixel the gy (upcast to float32) of the windows whose code
    points at it, added from 0 in the order oy ascending, then ox ascending.  Round once (`.to(dtype)`) for a
    half result."""
    B, C, Ho, Wo = gy.shape
    assert (Ho, Wo) == out_hw(H, W) and code.shape == gy.shape
    g = gy.float()
    index = code_to_index(code, H, W)
    inside = code <= 8
    gx = torch.zeros((B, C, H, W))
    r = torch.arange(H).reshape(H, 1).expand(H, W)
    c = torch.arange(W).reshape(1, W).expand(H, W)
    # the windows covering (r, c): oy in {(r - 1) // 2 + 0, + 1} that hold r, ox alike; ascending
    for dy in (0, 1):
        oy = (r + 1) // 2 - 1 + dy
        oky = (oy >= 0) & (oy < Ho) & (2 * oy - 1 <= r) & (r <= 2 * oy + 1)
        for dx in (0, 1):
            ox = (c + 1) // 2 - 1 + dx
            okx = (ox >= 0) & (ox < Wo) & (2 * ox - 1 <= c) & (c <= 2 * ox + 1)
            o = (oy.clamp(0, Ho - 1) * Wo + ox.clamp(0, Wo - 1)).reshape(-1)
            hit = (index.reshape(B, C, -1)[:, :, o].reshape(B, C, H, W) == r * W + c) & oky & okx
            hit = hit & inside.reshape(B, C, -1)[:, :, o].reshape(B, C, H, W)
            add = g.reshape(B, C, -1)[:, :, o].reshape(B, C, H, W)
            gx = torch.where(hit, gx + add, gx)
    return gx


def special_maps() -> Dict[str, torch.Tensor]:
    """float32 [1, 2, 7, 9] maps that pin the selection rule: a constant, a post-ReLU map (more than half
    zeros), mixed signed zeros, an all -inf window, one NaN, two NaNs in one window, both infinities"""
    gen = torch.Generator().manual_seed(1234)
    shape = (1, 2, 7, 9)
    nan, inf = float('nan'), float('inf')
    base = torch.randn(shape, generator=gen)
    relu = torch.relu(torch.randn(shape, generator=gen) - 0.3)
    assert float((relu == 0).float().mean()) >= 0.5
    zeros = torch.where(torch.rand(shape, generator=gen) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
    ninf = base.clone()
    ninf[0, 0, 0:4, 0:4] = -inf                         # the windows of (0, 0), (0, 1), (1, 0), (1, 1) hold nothing else
    ninf[0, 1, 3:, 5:] = -inf
    one_nan = base.clone()
    one_nan[0, 0, 3, 3] = nan                           # odd row and column: four windows
    one_nan[0, 1, 0, 0] = nan
    two_nans = base.clone()
    two_nans[0, 0, 2, 2] = nan
    two_nans[0, 0, 3, 3] = nan                          # window (1, 1) holds both, (2, 2) only the second
    two_nans[0, 1, 4, 1] = nan
    two_nans[0, 1, 4, 2] = nan
    infs = base.clone()
    infs[0, 0, 1, 1] = inf
    infs[0, 0, 1, 2] = inf                              # a tie of +inf: the first stays
    infs[0, 0, 5, 5] = -inf
    infs[0, 1, 6, 8] = inf
    infs[0, 1, 2, 4] = -inf
    return {'constant': torch.full(shape, 1.5), 'zero': torch.zeros(shape), 'relu': relu, 'signed_zeros': zeros,
            'all_neg_inf': ninf, 'one_nan': one_nan, 'two_nans': two_nans, 'infinities': infs}


def representable(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """x rounded to `dtype`, as float32: inputs every dtype holds exactly"""
    return x.to(dtype).float()


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """bit equality, NaN payloads and signed zeros included"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    view = torch.int32 if a.dtype == F32 else torch.int16
    return bool(torch.equal(a.contiguous().view(view), b.contiguous().view(view)))


def sizes() -> List[int]:
    return [1, 2, 3, 7, 8, 9]
