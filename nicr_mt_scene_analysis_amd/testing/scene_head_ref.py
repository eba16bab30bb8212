"""TEST / BENCHMARK INFRASTRUCTURE — never imported by the product path.

The scene head of include/nmsa.h (nmsa_scene_head_*) restated in torch on the CPU: every sum in the kernels'
order, in float32.  A fused multiply-add is done in float64, as testing/context_ref.py does it: the double
product of two floats is exact, the sum is rounded to double and then to float (a double rounding that differs
from the single one only when the double sum lands on a float32 tie).  Lanes that own no element keep their
sum (no zero is added for them: a -0.0 stays a -0.0).

Also the seeded cases of the fixture tests/golden/scene_decoder.npz (`SCENE_HEAD_CASES`), the shapes of the
GPU tests (`SCENE_HEAD_SHAPES`) and the torch composition the module falls back to."""
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

WAVE = 64
F32 = torch.float32

# the decoder inputs of the fixture: `features` is the shape of the context module's first context feature
# (None: no context features, the map `cm_output` itself is pooled)
SCENE_HEAD_CASES: Dict[str, dict] = {
    'ppm_1x1': dict(cm_output=(3, 48, 5, 7), features=(3, 32, 1, 1), n_classes=10, seed=7101),
    'appm_2x3': dict(cm_output=(3, 40, 6, 9), features=(3, 24, 2, 3), n_classes=17, seed=7102),
    'no_context': dict(cm_output=(4, 36, 7, 5), features=None, n_classes=45, seed=7103),
}

# (B, C, H, W, K) of the GPU tests: the smallest call; H W == 1; odd everything (element route); the vector route
# for both element sizes; C past two waves' worth of lanes and K past the wave count; H W = 259, past one pass of
# a wave; three images at H W == 1 with a wide K
SCENE_HEAD_SHAPES = ((1, 1, 1, 1, 1), (2, 3, 1, 1, 2), (2, 5, 3, 5, 3), (2, 64, 2, 4, 10), (1, 130, 4, 5, 17),
                     (2, 66, 7, 37, 45), (3, 8, 1, 1, 45))


def case_inputs(name: str) -> Dict[str, Optional[np.ndarray]]:
    """the seeded float32 inputs of a fixture case: cm_output, feature (or None), a second context feature that
    must not be read, weight [K, C], bias [K] and the upstream gradient g [B, K]"""
    case = SCENE_HEAD_CASES[name]
    rng = np.random.default_rng(case['seed'])
    cm_output = rng.standard_normal(case['cm_output']).astype(np.float32)
    feature = other = None
    if case['features'] is not None:
        feature = rng.standard_normal(case['features']).astype(np.float32)
        other = rng.standard_normal(case['features'][:2] + (2, 2)).astype(np.float32)
    C = (case['features'] or case['cm_output'])[1]
    B, K = case['cm_output'][0], case['n_classes']
    weight = (rng.standard_normal((K, C)) / np.sqrt(C)).astype(np.float32)
    bias = (0.1 * rng.standard_normal((K,))).astype(np.float32)
    g = rng.standard_normal((B, K)).astype(np.float32)
    return dict(cm_output=cm_output, feature=feature, other=other, weight=weight, bias=bias, g=g)


def case_arrays(inp) -> Tuple[np.ndarray, ...]:
    """the arrays of a case in the order their digest is taken"""
    return tuple(inp[k] for k in ('cm_output', 'feature', 'other', 'weight', 'bias', 'g') if inp[k] is not None)


def decoder_input(inp, requires_grad: bool = False, dtype=torch.float32, device='cpu'):
    """((cm_output, features), the map the decoder pools) as tensors"""
    def t(a):
        return torch.from_numpy(a).to(device=device, dtype=dtype).requires_grad_(requires_grad)
    cm_output = t(inp['cm_output'])
    if inp['feature'] is None:
        return (cm_output, ()), cm_output
    feature = t(inp['feature'])
    return (cm_output, (feature, t(inp['other']))), feature


def torch_composition(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """the reference's formulation, what the module's fallback runs"""
    return F.linear(torch.flatten(F.adaptive_avg_pool2d(x, 1), 1), weight, bias)


# ------------------------------------------------------------------------------ the kernels' arithmetic
def fma(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    return (a.double() * b.double() + c.double()).float()


def halves(v: torch.Tensor) -> torch.Tensor:
    """[.., 64] lane sums combined by halves: v[l] += v[l + o], o = 32 .. 1; the value of lane 0"""
    v = v.clone()
    o = WAVE // 2
    while o:
        v[..., :o] = v[..., :o] + v[..., o:2 * o]
        o //= 2
    return v[..., 0]


def chunk(dtype: torch.dtype) -> int:
    return 4 if dtype == F32 else 8


def pool(x: torch.Tensor) -> torch.Tensor:
    """pooled float32 [B, C] of x [B, C, H, W] (float32, or a half that is converted exactly)"""
    B, C, H, W = x.shape
    HW = H * W
    xf = x.detach().float().cpu().reshape(B * C, HW)
    if HW == 1:
        return xf.reshape(B, C)
    V = chunk(x.dtype)
    lanes = torch.arange(WAVE)
    acc = torch.zeros((B * C, WAVE))
    n_chunks = -(-HW // V)
    for j0 in range(0, n_chunks, WAVE):                     # chunk j0 + l belongs to lane l
        for e in range(V):
            i = (j0 + lanes) * V + e
            ok = ((j0 + lanes) < n_chunks) & (i < HW)
            acc = torch.where(ok, acc + xf[:, i.clamp(max=HW - 1)], acc)
    return (halves(acc) / torch.tensor(float(HW), dtype=F32)).reshape(B, C)


def linear(pooled: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """float32 [B, K] before the one rounding to the output dtype"""
    B, C = pooled.shape
    K = weight.shape[0]
    lanes = torch.arange(WAVE)
    acc = torch.zeros((B, K, WAVE))
    for c0 in range(0, C, WAVE):
        c = c0 + lanes
        ok = c < C
        cc = c.clamp(max=C - 1)
        acc = torch.where(ok, fma(weight[None, :, cc], pooled[:, None, cc], acc), acc)
    out = halves(acc)
    return out if bias is None else out + bias[None, :]


def forward(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], out_dtype=None):
    """(logits in `out_dtype` (x's when None), pooled float32) as nmsa_scene_head_fwd computes them"""
    pooled = pool(x)
    w = weight.detach().float().cpu()
    b = None if bias is None else bias.detach().float().cpu()
    return linear(pooled, w, b).to(x.dtype if out_dtype is None else out_dtype), pooled


def backward(g: torch.Tensor, pooled: torch.Tensor, weight: torch.Tensor, x_shape, x_dtype):
    """(gx in x_dtype, gweight, gbias) as nmsa_scene_head_bwd computes them"""
    B, C, H, W = x_shape
    gf = g.detach().float().cpu()
    w = weight.detach().float().cpu()
    p = pooled.detach().float().cpu()
    K = w.shape[0]
    gs = torch.zeros((B, C))
    for k in range(K):
        gs = fma(gf[:, k, None], w[None, k, :], gs)
    if H * W > 1:
        gs = gs / torch.tensor(float(H * W), dtype=F32)
    gx = gs.to(x_dtype).reshape(B, C, 1, 1).expand(B, C, H, W).contiguous()
    gw = torch.zeros((K, C))
    gb = torch.zeros((K,))
    for b in range(B):
        gw = fma(gf[b, :, None], p[None, b, :], gw)
        gb = gb + gf[b]
    return gx, gw, gb


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """bit equality, NaN payloads and signed zeros included"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    view = torch.int32 if a.dtype == F32 else torch.int16
    return bool(torch.equal(a.contiguous().cpu().view(view), b.contiguous().cpu().view(view)))
