"""GPU tier of the Swin encoder-decoder fusion (csrc/ln_transpose.hip, ops.ln_nhwc_to_nchw*,
model.encoder_decoder_fusion).

Oracle: LayerNorm over C, NHWC -> NCHW and the addition, with their gradients, written out in
float64 on the CPU from the same, already dtype-rounded inputs (`testing.fusion_ref.reference64`),
the error bounds of `testing.fusion_ref.bounds` (tests/test_fusion_host.py holds torch's own float32
to them), and the recorded results of the reference's module in tests/golden/encoder_decoder_fusion.npz.

Launch geometry the shapes are picked from (csrc/ln_transpose.hip): a workgroup of 256 lanes owns a
tile of 32 consecutive pixels of one image with all C channels; the statistics of a pixel are taken
by one wave, a lane holding the channels (k*64 + lane)*V .. +V of slot k, V = 4 (float32 x) / 8
(half x) on both routes, at most 32 values (C <= 2048); the transposition goes through LDS in chunks
of 128 channels, a wave working on 4 pixels x 16 groups of V channels at a time.  So: P around 32 and
64 (one tile, a partial second tile, two tiles), B = 2 (a tile must not run into the next image), C
around 64 and 128 (16V channels, one chunk) and up to 2048.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nicr_mt_scene_analysis_amd import _lib as L
from nicr_mt_scene_analysis_amd import ops
from nicr_mt_scene_analysis_amd.model import encoder_decoder_fusion as edf
from nicr_mt_scene_analysis_amd.testing import fusion_cases as fc
from nicr_mt_scene_analysis_amd.testing import fusion_ref as R

import _golden

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
PAIRS = ((F32, F32), (BF16, BF16), (BF16, F32), (F16, F16), (F16, F32))      # (dtype_x, dtype_y)
PAIR_IDS = ['f32-f32', 'bf16-bf16', 'bf16-f32', 'f16-f16', 'f16-f32']
VECTOR, ELEMENT = L.NMSA_LNT_ROUTE_VECTOR, L.NMSA_LNT_ROUTE_ELEMENT
VEC = {F32: 4, BF16: 8, F16: 8}
TILE = 32                                   # pixels of a tile
EXACT_CS = (2, 6, 62, 64, 66, 96, 192, 384, 768, 1536, 2048)
EXACT_PS = (1, 2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE)
POW2_CS = (2, 64, 128, 256, 512, 1024, 2048)
POISON = 12288.0                            # exact in bfloat16 and float16


# ------------------------------------------------------------------------------ helpers
def exact_inputs(B, P, C, dx, dy, seed):
    """rows s_bp * sigma (sigma: +1 / -1 in equal counts, s_bp a power of two in 1/4 .. 4), gamma and
    beta k/16, add and gy integers in -8..8: with eps = 0 the mean is 0, the variance s^2, rstd 1/s
    and xh = sigma, and every product and partial sum, in any order, is exact in float32"""
    assert C % 2 == 0 and B * P * 8 < 1 << 24
    gen = torch.Generator().manual_seed(seed)
    sigma = torch.ones(C)
    sigma[torch.randperm(C, generator=gen)[:C // 2]] = -1.0
    s = torch.exp2(torch.randint(-2, 3, (B, P, 1), generator=gen).float())
    x = (s * sigma).to(dx)
    gamma = torch.randint(-8, 9, (C,), generator=gen).float() / 16
    beta = torch.randint(-8, 9, (C,), generator=gen).float() / 16
    add = torch.randint(-8, 9, (B, C, P), generator=gen).to(dy)
    gy = torch.randint(-8, 9, (B, C, P), generator=gen).to(dy)
    return x, gamma, beta, add, gy


def dev(*tensors):
    return tuple(None if t is None else t.to(DEV) for t in tensors)


def off_by_one(t):
    """the same values on the device, one element into a larger buffer: off 16 bytes, on the element"""
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=DEV)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def run_op(x, gamma, beta, eps, add, gy, dy, element=False, need=(True, True, True)):
    """forward with saved statistics, then backward -> (y, gx, ggamma, gbeta, route)"""
    xd, gd, bd, ad, gyd = dev(x, gamma, beta, add, gy)
    if element:
        xd = off_by_one(xd)
    y, mean, rstd = ops.ln_nhwc_to_nchw(xd, gd, bd, eps, add=ad, out_dtype=dy, save_stats=True)
    gx, gg, gb = ops.ln_nhwc_to_nchw_backward(gyd, xd, gd, mean, rstd, *need)
    return y, gx, gg, gb, ops.ln_nhwc_to_nchw_route(xd, y)


def expected_route(P, C, dx, dy, element=False):
    return VECTOR if (not element and C % VEC[dx] == 0 and P % VEC[dy] == 0) else ELEMENT


def check_exact(B, P, C, dx, dy, with_add, element=False, seed=0):
    x, gamma, beta, add, gy = exact_inputs(B, P, C, dx, dy, seed)
    add = add if with_add else None
    ref = R.reference64(x, gamma, beta, 0.0, add, gy)
    y, gx, gg, gb, route = run_op(x, gamma, beta, 0.0, add, gy, dy, element)
    tag = (B, P, C, dx, dy, with_add, element)
    assert route == expected_route(P, C, dx, dy, element), tag
    assert y.dtype == dy and gx.dtype == dx and gg.dtype == gb.dtype == F32
    assert torch.equal(y.cpu(), ref['y'].to(dy)), tag            # the exact value, cast once
    assert torch.equal(gg.cpu().double(), ref['ggamma']), tag
    assert torch.equal(gb.cpu().double(), ref['gbeta']), tag
    if C & (C - 1) == 0:                                         # mean_c(a) is exact: a division by 2^k
        assert torch.equal(gx.cpu(), ref['gx'].to(dx)), tag
    return route


def check_bounds(x, gamma, beta, eps, add, gy, dx, dy, element=False, backward=True, tag=None):
    """the kernels — and torch's own float32 on the CPU, from the same inputs — against `bounds`"""
    ref = R.reference64(x, gamma, beta, eps, add, gy)
    y, gx, gg, gb, route = run_op(x, gamma, beta, eps, add, gy, dy, element)
    assert route == expected_route(x.shape[1], x.shape[2], dx, dy, element), tag
    bd = R.bounds(x, gamma, beta, eps, add, gy, dtype_y=dy, dtype_x=dx)
    bd32 = R.bounds(x, gamma, beta, eps, add, gy)
    xr, gr, br = (t.float().clone().requires_grad_(True) for t in (x, gamma, beta))
    yt = F.layer_norm(xr, (x.shape[-1],), gr, br, eps).permute(0, 2, 1)
    yt = yt if add is None else yt + add.float()
    yt.backward(gy.float())
    results = {'y': (y, yt)}
    if backward:
        results.update(gx=(gx, xr.grad), ggamma=(gg, gr.grad), gbeta=(gb, br.grad))
    for key, (got, torch32) in results.items():
        ours, theirs = R.worst_ratio(got, ref[key], bd[key]), R.worst_ratio(torch32, ref[key], bd32[key])
        print(tag, key, 'kernel %.3f torch-f32 %.3f of the bound' % (ours, theirs))
        assert theirs <= 1.0, (tag, key, 'torch float32', theirs)
        assert ours <= 1.0, (tag, key, ours)


# ------------------------------------------------------------------------------ a. exact
@pytest.mark.parametrize('pair', PAIRS, ids=PAIR_IDS)
def test_exact_forward_and_backward(pair):
    """every even C of the list x every P around the tile span, with and without `add`; where the
    shape takes the vector route, once more on the element route (x one element off 16 bytes).
    y, ggamma and gbeta are exact for every C, gx for the powers of two"""
    dx, dy = pair
    routes = set()
    for C in EXACT_CS:
        for P in EXACT_PS:
            for with_add in (False, True):
                route = check_exact(2, P, C, dx, dy, with_add, seed=C + P)
                routes.add(route)
                if route == VECTOR:
                    routes.add(check_exact(2, P, C, dx, dy, with_add, element=True, seed=C + P + 1))
    assert routes == {VECTOR, ELEMENT}


@pytest.mark.parametrize('pair', PAIRS, ids=PAIR_IDS)
def test_exact_backward_powers_of_two_and_partial_vector_tiles(pair):
    """gx bit for bit at every power of two; P = 40 and 72 are vector-route shapes whose last tile is
    partial (8 of 32 pixels)"""
    dx, dy = pair
    for C in POW2_CS:
        for P in (3, 40, 72):
            for element in (False, True):
                check_exact(2, P, C, dx, dy, True, element=element, seed=3 * C + P)


@pytest.mark.parametrize('pair', PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize('shape', ((2, 15 * 20, 768), (1, 30 * 40, 384)), ids=['15x20x768', '30x40x384'])
def test_exact_real_shapes(pair, shape):
    """15*20 = 300 pixels are a multiple of 4 but not of 8: with a half y that shape is an
    element-route shape, every other combination here takes the vector route"""
    vector = shape[1] % VEC[pair[1]] == 0
    assert vector or (shape[1] == 300 and pair[1] != F32)
    for with_add in (False, True):
        assert check_exact(*shape, *pair, with_add, seed=9) == (VECTOR if vector else ELEMENT)
    check_exact(*shape, *pair, True, element=True, seed=10)


def test_each_gradient_can_be_skipped():
    for dx, dy in ((F32, F32), (BF16, F32)):
        for P, C, element in ((40, 128, False), (33, 66, False), (40, 128, True)):
            x, gamma, beta, add, gy = exact_inputs(2, P, C, dx, dy, seed=P)
            full = run_op(x, gamma, beta, 0.0, None, gy, dy, element)[1:4]
            for skip in range(3):
                need = tuple(i != skip for i in range(3))
                got = run_op(x, gamma, beta, 0.0, None, gy, dy, element, need)[1:4]
                for i in range(3):
                    assert (got[i] is None) == (i == skip)
                    assert i == skip or torch.equal(got[i], full[i]), (dx, P, C, element, skip, i)
            only_gx = run_op(x, gamma, beta, 0.0, None, gy, dy, element, (True, False, False))[1:4]
            assert torch.equal(only_gx[0], full[0]) and only_gx[1] is None and only_gx[2] is None
            nothing = run_op(x, gamma, beta, 0.0, None, gy, dy, element, (False, False, False))[1:4]
            assert nothing == (None, None, None)


@pytest.mark.parametrize('pair', PAIRS, ids=PAIR_IDS)
def test_one_channel(pair):
    """C = 1: x - mean = 0, so y = beta (+ add) exactly and gx is exactly 0"""
    dx, dy = pair
    gen = torch.Generator().manual_seed(4)
    for P in (1, 5, 32, 67):
        x = torch.randn((2, P, 1), generator=gen).to(dx)
        gamma, beta = torch.tensor([1.75]), torch.tensor([-0.625])
        add = torch.randint(-8, 9, (2, 1, P), generator=gen).to(dy)
        gy = torch.randn((2, 1, P), generator=gen).to(dy)
        for a in (None, add):
            y, gx, gg, gb, route = run_op(x, gamma, beta, 1e-5, a, gy, dy)
            want = torch.full((2, 1, P), -0.625, dtype=torch.float64) + (0 if a is None else a.double())
            assert route == ELEMENT and torch.equal(y.cpu(), want.to(dy))
            assert torch.equal(gx.cpu(), torch.zeros((2, P, 1), dtype=dx))
            assert torch.equal(gg.cpu(), torch.zeros(1))
            # gbeta = sum gy: float32 sums of 2P terms in another order than the float64 one
            want_gb = gy.double().sum()
            assert abs(float(gb.cpu()[0]) - float(want_gb)) <= (2 * P + 2) * R.U * float(gy.double().abs().sum())


# ------------------------------------------------------------------------------ b. bounds
@pytest.mark.parametrize('C', (3, 7, 63, 65, 97, 2047))
def test_odd_channel_counts_within_bounds(C):
    """the element route: no C here is a multiple of a vector.  The four input classes, and for the
    forward also 1000 + N(0,1) (where the gx bound does not hold for torch's float32 either)"""
    for P in (1, 5, 67):
        for kind in R.INPUT_CLASSES:
            x, gamma, beta, gy, add = R.make_inputs(kind, 2, P, C, seed=C + P)
            check_bounds(x, gamma, beta, 1e-5, add, gy, F32, F32,
                         backward=kind not in R.FORWARD_ONLY_CLASSES, tag=(C, P, kind))


@pytest.mark.parametrize('pair', PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize('shape', ((2, 67, 96), (2, 300, 768)), ids=['67x96', '300x768'])
def test_rounding_on_normal_inputs(pair, shape):
    dx, dy = pair
    x, gamma, beta, gy, add = R.make_inputs('normal', *shape, seed=21, dtype=dx)
    gy, add = gy.to(dy), add.to(dy)
    check_bounds(x, gamma, beta, 1e-5, add, gy, dx, dy, tag=(shape, dx, dy, 'add'))
    check_bounds(x, gamma, beta, 1e-5, None, gy, dx, dy, tag=(shape, dx, dy, 'select'))


# ------------------------------------------------------------------------------ c. pointers
def _code(t):
    return L.float_dtype_code(t)


def _poisoned(n, dtype, lead):
    """a device buffer full of POISON and its window of n elements, `lead` elements in"""
    buf = torch.full((n + 64,), POISON, dtype=dtype, device=DEV)
    return buf, buf[lead:lead + n]


def _intact(buf, lead, n):
    return bool((buf[:lead] == POISON).all()) and bool((buf[lead + n:] == POISON).all())


@pytest.mark.parametrize('pair', PAIRS, ids=PAIR_IDS)
def test_offset_pointers_and_poison(pair):
    """y, gx, mean and rstd one element into poisoned buffers: the element route, the values of the
    vector route, nothing written in front of or behind any of them"""
    dx, dy = pair
    B, P, C = 2, 40, 136                    # a partial second tile, a partial second chunk
    x, gamma, beta, gy, add = R.make_inputs('normal', B, P, C, seed=31, dtype=dx)
    gy, add = gy.to(dy), add.to(dy)
    xd, gd, bd, gyd, ad = dev(x, gamma, beta, gy, add)
    y0, mean0, rstd0 = ops.ln_nhwc_to_nchw(xd, gd, bd, 1e-5, add=ad, out_dtype=dy, save_stats=True)
    gx0, gg0, gb0 = ops.ln_nhwc_to_nchw_backward(gyd, xd, gd, mean0, rstd0)
    assert ops.ln_nhwc_to_nchw_route(xd, y0) == VECTOR and ops.ln_nhwc_to_nchw_route(gx0, gyd) == VECTOR
    n, rows = B * P * C, B * P
    for lead in (1, 17):
        ybuf, y = _poisoned(n, dy, lead)
        gxbuf, gx = _poisoned(n, dx, lead)
        y, gx = y.view(B, C, P), gx.view(B, P, C)
        mbuf, mean = _poisoned(rows, F32, lead)
        rbuf, rstd = _poisoned(rows, F32, lead)
        gg, gb = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        ws = torch.empty(L.lib().nmsa_ln_nhwc_nchw_bwd_workspace_bytes(B, P, C) // 4, device=DEV)
        assert ops.ln_nhwc_to_nchw_route(xd, y) == ELEMENT and ops.ln_nhwc_to_nchw_route(gx, gyd) == ELEMENT
        stream = L.stream_ptr(DEV)
        L.check(L.lib().nmsa_ln_nhwc_nchw_fwd(L.ptr(xd), _code(xd), L.ptr(gd), L.ptr(bd), 1e-5, L.ptr(ad), B, P, C,
                                              L.ptr(y), _code(y), L.ptr(mean), L.ptr(rstd), stream), 'fwd')
        L.check(L.lib().nmsa_ln_nhwc_nchw_bwd(L.ptr(gyd), _code(gyd), L.ptr(xd), _code(xd), L.ptr(gd), L.ptr(mean),
                                              L.ptr(rstd), B, P, C, L.ptr(gx), L.ptr(gg), L.ptr(gb), L.ptr(ws),
                                              ws.numel() * 4, stream), 'bwd')
        torch.cuda.synchronize()
        assert torch.equal(y, y0) and torch.equal(gx, gx0)
        assert torch.equal(mean, mean0) and torch.equal(rstd, rstd0)
        assert torch.equal(gg, gg0) and torch.equal(gb, gb0)
        for buf, cnt in ((ybuf, n), (gxbuf, n), (mbuf, rows), (rbuf, rows)):
            assert _intact(buf, lead, cnt), lead


def test_non_contiguous_inputs():
    gen = torch.Generator().manual_seed(8)
    B, H, W, C = 2, 5, 8, 64
    wide = torch.randn((B, H, W, C + 8), generator=gen).to(DEV)
    gwide = torch.randn((B, C, H, W + 3), generator=gen).to(DEV)
    awide = torch.randn((B, C, H + 1, W), generator=gen).to(DEV)
    gamma, beta = dev(torch.randn(C, generator=gen), torch.randn(C, generator=gen))
    x, gy, add = wide[..., 4:4 + C], gwide[..., 1:1 + W], awide[:, :, 1:]
    assert not x.is_contiguous() and not gy.is_contiguous() and not add.is_contiguous()
    y, mean, rstd = ops.ln_nhwc_to_nchw(x, gamma, beta, 1e-5, add=add, save_stats=True)
    y2, mean2, rstd2 = ops.ln_nhwc_to_nchw(x.contiguous(), gamma, beta, 1e-5, add=add.contiguous(), save_stats=True)
    assert y.shape == (B, C, H, W) and y.is_contiguous()
    assert torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
    got = ops.ln_nhwc_to_nchw_backward(gy, x, gamma, mean, rstd)
    want = ops.ln_nhwc_to_nchw_backward(gy.contiguous(), x.contiguous(), gamma, mean, rstd)
    assert got[0].shape == x.shape
    for a, e in zip(got, want):
        assert torch.equal(a, e)


# ------------------------------------------------------------------------------ d. determinism, streams, graph
def test_backward_twice_side_stream_and_graph():
    B, P, C = 2, 300, 768
    gen = torch.Generator().manual_seed(12)

    def draw():
        return dev(torch.randn((B, P, C), generator=gen).bfloat16(), torch.randn((B, C, P), generator=gen),
                   torch.randn((B, C, P), generator=gen))
    gamma, beta = dev(1 + 0.25 * torch.randn(C, generator=gen), torch.randn(C, generator=gen))

    def step(x, gy, add):
        y, mean, rstd = ops.ln_nhwc_to_nchw(x, gamma, beta, 1e-5, add=add, out_dtype=F32, save_stats=True)
        return (y,) + tuple(ops.ln_nhwc_to_nchw_backward(gy, x, gamma, mean, rstd))

    x, gy, add = draw()
    first, second = step(x, gy, add), step(x, gy, add)
    torch.cuda.synchronize()
    for a, e in zip(first, second):
        assert torch.equal(a, e)                                 # no atomics: the same bytes
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = step(x, gy, add)
    side.synchronize()
    for a, e in zip(on_side, first):
        assert torch.equal(a, e)
    # one chain on one stream: capture after the eager warm-up above, replay with new contents
    sx, sgy, sadd = x.clone(), gy.clone(), add.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(sx, sgy, sadd)
    for _ in range(2):
        nx, ngy, nadd = draw()
        sx.copy_(nx), sgy.copy_(ngy), sadd.copy_(nadd)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(nx, ngy, nadd)
        for a, e in zip(captured, eager):
            assert torch.equal(a, e)


# ------------------------------------------------------------------------------ e. module
@pytest.fixture(scope='module')
def golden():
    return _golden.load('encoder_decoder_fusion')


def build(name, device=DEV):
    fusion, n_enc, n_dec, _, _ = fc.FUSION_CASES[name]
    inp = fc.make_fusion_inputs(name)
    module = edf.get_encoder_decoder_fusion_class(fusion)(n_channels_encoder=n_enc, n_channels_decoder=n_dec)
    params = dict(module.named_parameters())
    with torch.no_grad():
        for key, value in inp['params'].items():
            params[key].copy_(torch.from_numpy(value))
    return module.to(device), inp


def run_module(module, inp, key):
    x_enc = torch.from_numpy(inp['x_enc']).to(DEV).requires_grad_(True)
    x_dec = torch.from_numpy(inp['x_dec']).to(DEV).requires_grad_(True)
    gy = torch.from_numpy(inp['gy']).to(DEV)
    y = module({key: x_enc}, x_dec)
    y.backward(gy)
    return y, x_enc, x_dec, gy


@pytest.mark.parametrize('name', [n for n in fc.FUSION_CASES if n.startswith('swin_ln') and n.endswith('_eq')])
def test_module_equal_channels_against_the_recorded_reference(golden, name):
    """the module's results lie within `bounds` of the float64 value; the recorded results are the
    reference's float32, itself within one bound of that value, so the two differ by at most twice
    the bound"""
    module, inp = build(name)
    p = _golden.jload(golden[f'{name}__params'])
    y, x_enc, x_dec, gy = run_module(module, inp, p['key'])
    is_add = 'add' in p['fusion']
    x, add = torch.from_numpy(inp['x_enc']), torch.from_numpy(inp['x_dec']) if is_add else None
    gamma, beta = (torch.from_numpy(inp['params'][k]) for k in ('ln.weight', 'ln.bias'))
    bd = R.bounds(x, gamma, beta, module.ln.eps, add, torch.from_numpy(inp['gy']))
    ref = R.reference64(x, gamma, beta, module.ln.eps, add, torch.from_numpy(inp['gy']))
    assert y.is_contiguous() and y.dtype == F32
    for got, key in ((y, 'y'), (x_enc.grad, 'gx'), (module.ln.weight.grad, 'ggamma'), (module.ln.bias.grad, 'gbeta')):
        assert R.worst_ratio(got, ref[key], bd[key]) <= 1.0, (name, key)
    for got, want, bound in ((y, golden[f'{name}__y'], bd['y']), (x_enc.grad, golden[f'{name}__gx_enc'], bd['gx']),
                             (module.ln.weight.grad, golden[f'{name}__g__ln.weight'], bd['ggamma']),
                             (module.ln.bias.grad, golden[f'{name}__g__ln.bias'], bd['gbeta'])):
        err = (got.detach().double().cpu() - torch.from_numpy(want).double()).abs()
        assert bool((err <= 2 * bound.reshape(err.shape)).all()), (name, float((err / bound.reshape(err.shape)).max()))
    if is_add:
        assert torch.equal(x_dec.grad, gy)                       # the upstream gradient itself
        assert torch.equal(x_dec.grad.cpu(), torch.from_numpy(golden[f'{name}__gx_dec']))
    else:
        assert x_dec.grad is None and 'gx_dec' not in p['grads']


@pytest.mark.parametrize('name', [n for n in fc.FUSION_CASES if n.startswith('swin_ln') and n.endswith('_ne')])
def test_module_unequal_channels_against_the_recorded_reference(golden, name):
    """kernel, then the 1x1 ConvNormAct and the fuse operation in torch.  The LayerNorm error (a few
    1e-7 relative) passes through 8-12 weights of size 0.3 and a batch normalization over 30-60
    samples (1/std about 1 to 3): 1e-5 of the largest magnitude at most; 1e-4 leaves a decade for the
    device's own convolution and batch-norm arithmetic against the CPU's"""
    module, inp = build(name)
    p = _golden.jload(golden[f'{name}__params'])
    y, x_enc, x_dec, gy = run_module(module, inp, p['key'])

    # every tensor against its own largest recorded magnitude.  The gradient of ln.bias is the one
    # exception: it is a sum that cancels to zero in exact arithmetic (the batch normalization removes a
    # per-channel shift), both sides hold rounding noise of the terms' size there, so its scale is that
    # of the same sum without the cancellation, the gradient of ln.weight
    def close(got, want, scale=None):
        scale = float(np.abs(want).max()) if scale is None else scale
        return bool(((got.detach().cpu() - torch.from_numpy(want)).abs() <= 1e-4 * scale).all())
    assert close(y, golden[f'{name}__y']) and close(x_enc.grad, golden[f'{name}__gx_enc'])
    for key, param in module.named_parameters():
        scale = float(np.abs(golden[f'{name}__g__ln.weight']).max()) if key == 'ln.bias' else None
        assert close(param.grad, golden[f'{name}__g__{key}'], scale), key
    if 'add' in p['fusion']:
        assert torch.equal(x_dec.grad.cpu(), torch.from_numpy(golden[f'{name}__gx_dec']))
    else:
        assert x_dec.grad is None


def test_module_loads_a_reference_shaped_state_dict(golden):
    recorded = _golden.jload(golden['state'])
    gen = torch.Generator().manual_seed(2)
    for name in ('swin-ln-add', 'swin-ln-select-rgb'):
        for n_enc, n_dec in fc.FUSION_STATE_CHANNELS:
            state = {k: (torch.zeros(s, dtype=torch.int64) if k.endswith('num_batches_tracked')
                         else torch.rand(s, generator=gen)) for k, s in recorded[name][f'{n_enc}_{n_dec}'].items()}
            m = edf.get_encoder_decoder_fusion_class(name)(n_channels_encoder=n_enc, n_channels_decoder=n_dec)
            m.load_state_dict(state, strict=True)
            m = m.to(DEV).eval()
            x = torch.randn((2, 3, 4, n_enc), generator=gen).to(DEV)
            x_dec = torch.randn((2, n_dec, 3, 4), generator=gen).to(DEV)
            with torch.no_grad():
                got = m({'rgb': x}, x_dec)
                ln = F.layer_norm(x, (n_enc,), m.ln.weight, m.ln.bias, m.ln.eps).permute(0, 3, 1, 2)
                want = m._fuse_operation(m.layer(ln), x_dec)
            assert got.shape == (2, n_dec, 3, 4)
            assert torch.allclose(got, want, rtol=1e-5, atol=1e-5)


def test_module_sgd_step_moves_the_layer_norm_parameters_like_torch():
    lr = 0.1
    name = 'swin_ln_add_eq'
    ours, inp = build(name)
    theirs, _ = build(name, device='cpu')
    theirs = theirs.double()
    run_module(ours, inp, 'enc')
    x = torch.from_numpy(inp['x_enc']).double()
    y = F.layer_norm(x, (x.shape[-1],), theirs.ln.weight, theirs.ln.bias, theirs.ln.eps).permute(0, 3, 1, 2)
    (y + torch.from_numpy(inp['x_dec']).double()).backward(torch.from_numpy(inp['gy']).double())
    before = {k: v.detach().clone() for k, v in ours.ln.named_parameters()}
    for m in (ours, theirs):
        torch.optim.SGD(m.ln.parameters(), lr=lr).step()
    gamma, beta = (torch.from_numpy(inp['params'][k]) for k in ('ln.weight', 'ln.bias'))
    bd = R.bounds(torch.from_numpy(inp['x_enc']), gamma, beta, ours.ln.eps, torch.from_numpy(inp['x_dec']),
                  torch.from_numpy(inp['gy']))
    for key, bound in (('weight', bd['ggamma']), ('bias', bd['gbeta'])):
        got, want = getattr(ours.ln, key).detach().double().cpu(), getattr(theirs.ln, key).detach()
        assert not torch.equal(getattr(ours.ln, key).detach(), before[key])
        # lr * the gradient's bound, and the rounding of the float32 update itself
        assert bool(((got - want).abs() <= lr * bound + 2 * R.U * want.abs()).all()), key


def test_module_autocast_and_half():
    gen = torch.Generator().manual_seed(6)
    B, H, W, C = 2, 6, 8, 96
    x32 = torch.randn((B, H, W, C), generator=gen)
    x = x32.bfloat16().to(DEV).requires_grad_(True)
    x_dec = torch.randn((B, C, H, W), generator=gen).to(DEV).requires_grad_(True)
    gy = torch.randn((B, C, H, W), generator=gen)
    m = edf.get_encoder_decoder_fusion_class('swin-ln-add')(n_channels_encoder=C, n_channels_decoder=C).to(DEV)
    with torch.no_grad():
        m.ln.weight.copy_(1 + 0.25 * torch.randn(C, generator=gen))
        m.ln.bias.copy_(torch.randn(C, generator=gen))
    with torch.autocast('cuda', dtype=torch.bfloat16):
        y = m({'enc': x}, x_dec)
    y.backward(gy.to(DEV))
    assert y.dtype == F32 and m.ln.weight.dtype == F32 and m.ln.weight.grad.dtype == F32 and x.grad.dtype == BF16
    args = (x.detach().cpu(), m.ln.weight.detach().cpu(), m.ln.bias.detach().cpu(), m.ln.eps, x_dec.detach().cpu(), gy)
    ref, bd = R.reference64(*args), R.bounds(*args, dtype_y=F32, dtype_x=BF16)
    for got, key in ((y, 'y'), (x.grad, 'gx'), (m.ln.weight.grad, 'ggamma'), (m.ln.bias.grad, 'gbeta')):
        assert R.worst_ratio(got, ref[key], bd[key]) <= 1.0, key
    assert torch.equal(x_dec.grad, gy.to(DEV))
    # outside autocast the output has the input's dtype; a half decoder tensor is added by the kernel
    y16 = m({'enc': x.detach()}, x_dec.detach().bfloat16())
    assert y16.dtype == BF16
    # module.half(): float16 parameters are cast for the kernel and get float16 gradients
    h = edf.get_encoder_decoder_fusion_class('swin-ln-select')(n_channels_encoder=C, n_channels_decoder=C)
    h = h.to(DEV).half()
    xh = x32.half().to(DEV).requires_grad_(True)
    yh = h({'enc': xh}, None)
    yh.backward(gy.half().to(DEV))
    assert yh.dtype == F16 and h.ln.weight.grad.dtype == F16 and xh.grad.dtype == F16
    args = (xh.detach().cpu(), h.ln.weight.detach().float().cpu(), h.ln.bias.detach().float().cpu(), h.ln.eps, None,
            gy.half())
    ref, bd = R.reference64(*args), R.bounds(*args, dtype_y=F16, dtype_x=F16)
    assert R.worst_ratio(yh, ref['y'], bd['y']) <= 1.0 and R.worst_ratio(xh.grad, ref['gx'], bd['gx']) <= 1.0


def test_no_gradient_means_no_statistics_and_inference_works():
    m = edf.get_encoder_decoder_fusion_class('swin-ln-select')(n_channels_encoder=8, n_channels_decoder=8).to(DEV)
    x = torch.randn(1, 3, 4, 8, device=DEV)
    with torch.no_grad():
        y = m({'enc': x}, None)
    assert y.shape == (1, 8, 3, 4) and not y.requires_grad
    want = F.layer_norm(x, (8,), m.ln.weight, m.ln.bias, m.ln.eps).permute(0, 3, 1, 2)
    assert torch.allclose(y, want, rtol=1e-5, atol=1e-6)
