"""TEST / BENCHMARK INFRASTRUCTURE — never imported by the product path.

The reference's learned upsampling written out as torch ops (model/upsampling.py:85-96:
`interpolate` -> `ReplicationPad2d` -> depthwise `conv2d`, and the zero-pad form), the oracle of
tests/test_upsampling.py and the baseline of tools/bench_upsampling.py, plus the error bounds the
tests derive from it."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24          # unit roundoff of float32


def torch_formulation(x, weight, bias, zeropad: bool):
    """nearest x2, pad, depthwise 3x3 — in x's dtype, on x's device"""
    up = F.interpolate(x, scale_factor=2., mode='nearest')
    if zeropad:
        return F.conv2d(up, weight, bias, padding=1, groups=x.shape[1])
    return F.conv2d(F.pad(up, (1, 1, 1, 1), mode='replicate'), weight, bias, groups=x.shape[1])


def unfold_formulation(x, weight, bias, zeropad: bool):
    """the same sum written as nine shifted views (`unfold`) and one einsum: what `torch_formulation`
    computes, without a grouped convolution — that one takes seconds per call on the CPU at tens of
    thousands of channels.  tests/test_upsampling_host.py holds the two equal."""
    up = F.interpolate(x, scale_factor=2., mode='nearest')
    up = F.pad(up, (1, 1, 1, 1), mode='constant' if zeropad else 'replicate')
    taps = up.unfold(2, 3, 1).unfold(3, 3, 1)                    # [B, C, 2h, 2w, 3, 3]
    y = torch.einsum('bcyxij,cij->bcyx', taps, weight[:, 0])
    return y if bias is None else y + bias[None, :, None, None]


def reference64(x, weight, bias, gy, zeropad: bool, formulation=None):
    """(y, gx, gW, gb) of the formulation in float64 on the CPU, from the given (already
    dtype-rounded) tensors; gb is None without a bias"""
    x64 = x.detach().double().cpu().requires_grad_(True)
    w64 = weight.detach().double().cpu().requires_grad_(True)
    b64 = None if bias is None else bias.detach().double().cpu().requires_grad_(True)
    y = (formulation or torch_formulation)(x64, w64, b64, zeropad)
    y.backward(gy.detach().double().cpu())
    return y.detach(), x64.grad, w64.grad, None if b64 is None else b64.grad


def half_ulp(expected64, dtype):
    """r of the bounds: 0 for float32, half an ulp of `dtype` at the expected value otherwise (the
    spacing of the format at |expected|, the smallest subnormal step below the normal range)"""
    if dtype == torch.float32:
        return torch.zeros_like(expected64)
    fi = torch.finfo(dtype)
    mant = 7 if dtype == torch.bfloat16 else 10
    e = torch.floor(torch.log2(expected64.abs().clamp_min(fi.tiny)))
    return 0.5 * torch.exp2(e - mant)


def bounds(x, weight, bias, gy, zeropad: bool, dtype):
    """The derived error bounds of y, gx, gW, gb against `reference64` (u = 2^-24):
      y   12 u M + r      M: the formula in float64 on |x|, |W|, |b| (9 products, their sums, the
                          bias, one pre-added weight pair)
      gx  40 u M_gx + r   M_gx: the float64 input gradient of the abs-valued formula (at most 36
                          products per pixel)
      gW, gb  (N + 2) u M, N = B * 4hw: the order-free worst case of a sum of N terms
    r = half an ulp of the output dtype at the expected value (0 for float32)."""
    y64, gx64, _, _ = reference64(x, weight, bias, gy, zeropad)
    ya, gxa, gwa, gba = reference64(x.abs(), weight.abs(), None if bias is None else bias.abs(), gy.abs(), zeropad)
    B, _, h, w = x.shape
    n = B * 4 * h * w
    return {'y': 12 * U * ya + half_ulp(y64, dtype), 'gx': 40 * U * gxa + half_ulp(gx64, dtype),
            'gw': (n + 2) * U * gwa,
            'gb': (n + 2) * U * (gba if gba is not None else gy.detach().double().cpu().abs().sum((0, 2, 3)))}
