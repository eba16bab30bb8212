"""GPU tier of the learned upsampling (csrc/upsampling.hip, ops.upsample2x_dw3x3*, model.upsampling).

Oracle: the reference's formulation as torch ops (interpolate -> pad -> depthwise conv2d),
evaluated on the CPU in float64 from the same, already dtype-rounded inputs
(`testing.upsampling_ref.reference64`), plus the recorded results of the reference's own module in
tests/golden/upsampling.npz.

Launch geometry the shapes are picked from (csrc/upsampling.hip): a lane owns a run of 2 (f32) or
4 (half) input pixels on the vector route and 1 on the one-pixel route; a wave spans 64 runs
(128 / 256 / 64 pixels), a workgroup of 256 lanes 512 / 1024 / 256 pixels of a row; a lane walks a
tile of 8 input rows; a plane's (tile, run) units are split into chunks of 256.
"""
import itertools

import numpy as np
import pytest
import torch

from nicr_mt_scene_analysis_amd import _lib as L
from nicr_mt_scene_analysis_amd import ops
from nicr_mt_scene_analysis_amd.model import upsampling as up
from nicr_mt_scene_analysis_amd.testing import synthetic as syn
from nicr_mt_scene_analysis_amd.testing import upsampling_ref as R

import _golden

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
MODES = (False, True)                       # zeropad
VECTOR, PIXEL = L.NMSA_UP_ROUTE_VECTOR, L.NMSA_UP_ROUTE_PIXEL
RUN = {torch.float32: 2, torch.bfloat16: 4, torch.float16: 4}


# ------------------------------------------------------------------------------ helpers
def grid_inputs(B, C, h, w, dtype, seed, bias=True):
    """integers in -8..8 for x and gy, k/16 with k in -8..8 for W and b: with B*4hw <= 2^18 per
    channel every product and every partial sum, in any order, is exact in float32"""
    assert B * 4 * h * w <= 1 << 18
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-8, 9, (B, C, h, w), generator=gen).to(dtype)
    gy = torch.randint(-8, 9, (B, C, 2 * h, 2 * w), generator=gen).to(dtype)
    wt = torch.randint(-8, 9, (C, 1, 3, 3), generator=gen).float() / 16
    b = torch.randint(-8, 9, (C,), generator=gen).float() / 16 if bias else None
    return x, gy, wt, b


def normal_inputs(B, C, h, w, dtype, seed, bias=True):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((B, C, h, w), generator=gen).to(dtype)
    gy = torch.randn((B, C, 2 * h, 2 * w), generator=gen).to(dtype)
    wt = torch.randn((C, 1, 3, 3), generator=gen) * 0.25
    b = torch.randn((C,), generator=gen) if bias else None
    return x, gy, wt, b


def dev(*tensors):
    return tuple(None if t is None else t.to(DEV) for t in tensors)


def run_op(x, gy, wt, b, zeropad, **need):
    xd, gyd, wd, bd = dev(x, gy, wt, b)
    y = ops.upsample2x_dw3x3(xd, wd, bd, zeropad)
    gx, gw, gb = ops.upsample2x_dw3x3_backward(gyd, xd, wd, zeropad, **need)
    routes = (ops.upsample2x_dw3x3_route(xd, y), ops.upsample2x_dw3x3_route(xd, gyd))
    return y, gx, gw, gb, routes


def check_exact(B, C, h, w, dtype, zeropad, seed=0, bias=True, formulation=None):
    x, gy, wt, b = grid_inputs(B, C, h, w, dtype, seed, bias)
    y64, gx64, gw64, gb64 = R.reference64(x, wt, b, gy, zeropad, formulation)
    y, gx, gw, gb, routes = run_op(x, gy, wt, b, zeropad)
    tag = (B, C, h, w, dtype, zeropad)
    assert y.dtype == dtype and gx.dtype == dtype and gw.dtype == gb.dtype == torch.float32
    assert torch.equal(y.cpu(), y64.to(dtype)), tag          # the exact value, cast once
    assert torch.equal(gx.cpu(), gx64.to(dtype)), tag
    assert torch.equal(gw.cpu().double(), gw64), tag
    assert torch.equal(gb.cpu().double(), gy.double().sum((0, 2, 3))), tag
    if bias:
        assert torch.equal(gb.cpu().double(), gb64), tag
    assert routes[0] == routes[1] == (VECTOR if w % RUN[dtype] == 0 else PIXEL), tag
    return routes[0]


# ------------------------------------------------------------------------------ a. exact, integer grid
@pytest.mark.parametrize('zeropad', MODES)
@pytest.mark.parametrize('dtype', DTYPES)
def test_exact_smallest_maps(dtype, zeropad):
    """h, w in {1, 2, 3}: every pixel is a border pixel, at h = 1 / w = 1 of both sides at once"""
    for h, w in itertools.product((1, 2, 3), repeat=2):
        check_exact(2, 3, h, w, dtype, zeropad, seed=10 * h + w)


@pytest.mark.parametrize('zeropad', MODES)
@pytest.mark.parametrize('dtype', DTYPES)
def test_exact_width_edges(dtype, zeropad):
    """w one below, at and above: the lane run (2 for f32, 4 for half), a wave's span (64 runs: 128
    / 256 pixels on the vector route, 64 pixels on the one-pixel route that the odd widths take), a
    workgroup's row span (256 runs: 512 / 1024 pixels, 256 on the one-pixel route); the nearest
    widths that stay on the vector route (w +- run) ride along.  h = 3 keeps two tile-less borders
    and an interior row."""
    run = RUN[dtype]
    widths = {run - 1, run, run + 1, 2 * run, 63, 64, 65, 255, 256, 257}
    for span in (64 * run, 256 * run):
        widths |= {span - run, span - 1, span, span + 1, span + run}
    routes = {check_exact(1, 2, 3, w, dtype, zeropad, seed=w) for w in sorted(widths)}
    assert routes == {VECTOR, PIXEL}


@pytest.mark.parametrize('zeropad', MODES)
@pytest.mark.parametrize('dtype', DTYPES)
def test_exact_height_edges(dtype, zeropad):
    """h one below, at and above the tile height (8) and twice it; w = 8 is the vector route of
    every dtype, w = 7 the one-pixel route; 40 and 33 columns with h = 17 put a tile border and a
    chunk border (256 units) inside one plane"""
    for h, w in itertools.product((7, 8, 9, 15, 16, 17), (8, 7)):
        check_exact(2, 2, h, w, dtype, zeropad, seed=h)
    for h, w in ((17, 40 * RUN[dtype]), (17, 129)):
        check_exact(1, 3, h, w, dtype, zeropad, seed=w)


@pytest.mark.parametrize('zeropad', MODES)
def test_exact_plane_counts(zeropad):
    """B*C in {1, 3, 70001}: one plane, a batch of three of one channel (the reducer walks n), and
    more planes than a grid's y / z dimension holds (h = 1, w = 2; the grid-stride loop runs)"""
    check_exact(1, 1, 5, 6, torch.float32, zeropad)
    check_exact(3, 1, 5, 6, torch.float32, zeropad)
    check_exact(1, 3, 5, 6, torch.bfloat16, zeropad)
    check_exact(1, 70001, 1, 2, torch.float32, zeropad, formulation=R.unfold_formulation)
    check_exact(7, 10001, 1, 2, torch.float32, zeropad, formulation=R.unfold_formulation)


@pytest.mark.parametrize('zeropad', MODES)
@pytest.mark.parametrize('dtype', DTYPES)
def test_exact_without_bias(dtype, zeropad):
    for h, w in ((3, 4), (9, 5)):
        check_exact(2, 3, h, w, dtype, zeropad, bias=False)


@pytest.mark.parametrize('zeropad', MODES)
@pytest.mark.parametrize('dtype', (torch.float32, torch.bfloat16))
def test_each_gradient_can_be_skipped(dtype, zeropad):
    for w in (8, 7):
        x, gy, wt, b = grid_inputs(2, 3, 9, w, dtype, seed=5)
        full = run_op(x, gy, wt, b, zeropad)
        for skip in ('need_gx', 'need_gweight', 'need_gbias'):
            got = run_op(x, gy, wt, b, zeropad, **{skip: False})
            for name, a, e in zip(('need_gx', 'need_gweight', 'need_gbias'), got[1:4], full[1:4]):
                assert (a is None) if name == skip else torch.equal(a, e), (skip, name)
        none = run_op(x, gy, wt, b, zeropad, need_gx=False, need_gweight=False, need_gbias=False)
        assert none[1:4] == (None, None, None) and torch.equal(none[0], full[0])


@pytest.mark.parametrize('zeropad', MODES)
@pytest.mark.parametrize('dtype', DTYPES)
def test_both_routes_and_an_offset_output_with_poison(dtype, zeropad):
    """the same even-width call on the vector route and, with y one element into a larger
    allocation (off 16 bytes), on the one-pixel route: the same values, and the poison in front of
    and behind y's range is intact"""
    B, C, h, w = 2, 3, 9, 16
    x, gy, wt, b = grid_inputs(B, C, h, w, dtype, seed=21)
    y64 = R.reference64(x, wt, b, gy, zeropad)[0]
    xd, wd, bd = dev(x, wt, b)
    y = ops.upsample2x_dw3x3(xd, wd, bd, zeropad)
    assert ops.upsample2x_dw3x3_route(xd, y) == VECTOR
    n = y.numel()
    buf = torch.full((n + 64,), 1024.0, dtype=dtype, device=DEV)
    view = buf[1:1 + n].view(y.shape)
    assert ops.upsample2x_dw3x3_route(xd, view) == PIXEL
    out = ops.upsample2x_dw3x3(xd, wd, bd, zeropad, out=view)
    assert out.data_ptr() == view.data_ptr() == buf.data_ptr() + buf.element_size()
    assert torch.equal(view, y) and torch.equal(y.cpu(), y64.to(dtype))
    assert buf[0].item() == 1024.0 and bool((buf[1 + n:] == 1024.0).all())
    # an input one element into its allocation: the backward call's one-pixel route
    xbuf = torch.zeros((x.numel() + 8,), dtype=dtype, device=DEV)
    xoff = xbuf[1:1 + x.numel()].view(x.shape).copy_(xd)
    gyd = gy.to(DEV)
    assert ops.upsample2x_dw3x3_route(xoff, gyd) == PIXEL and ops.upsample2x_dw3x3_route(xd, gyd) == VECTOR
    for a, e in zip(ops.upsample2x_dw3x3_backward(gyd, xoff, wd, zeropad), ops.upsample2x_dw3x3_backward(gyd, xd, wd, zeropad)):
        assert torch.equal(a, e)
    assert torch.equal(ops.upsample2x_dw3x3(xoff, wd, bd, zeropad), y)


# ------------------------------------------------------------------------------ b. beyond 2^31 elements
def test_more_than_two_to_the_31_output_elements():
    """bf16 [1, 2049, 512, 512], replicate: 2049 * 4 * 512 * 512 = 2^31 + 2^20 output elements, so
    the last planes lie behind a 32-bit element offset.  The first and the last four planes hold
    grid values and equal torch's float64 result on the GPU for those eight planes alone; every
    other plane holds one constant x and one constant gy, for which the exact results are
    y = b + x * sum(W) everywhere and gx = gy * (the channel's response to gy = 1, which depends
    on the pixel's border class only: top / interior / bottom times left / interior / right)."""
    C, h, w, dtype = 2049, 512, 512, torch.bfloat16
    gen = torch.Generator().manual_seed(31)
    wt = (torch.randint(-8, 9, (C, 1, 3, 3), generator=gen).float() / 16).to(DEV)
    b = (torch.randint(-8, 9, (C,), generator=gen).float() / 16).to(DEV)
    cx = torch.randint(-8, 9, (C,), generator=gen).to(DEV)
    cg = torch.randint(-8, 9, (C,), generator=gen).to(DEV)
    edge = torch.tensor([0, 1, 2, 3, C - 4, C - 3, C - 2, C - 1], device=DEV)
    x = cx.to(dtype)[None, :, None, None].expand(1, C, h, w).contiguous()
    gy = cg.to(dtype)[None, :, None, None].expand(1, C, 2 * h, 2 * w).contiguous()
    torch.manual_seed(32)
    x[0, edge] = torch.randint(-8, 9, (8, h, w), device=DEV).to(dtype)
    gy[0, edge] = torch.randint(-8, 9, (8, 2 * h, 2 * w), device=DEV).to(dtype)
    assert gy.numel() > 1 << 31

    y = ops.upsample2x_dw3x3(x, wt, b, False)
    gx, gw, gb = ops.upsample2x_dw3x3_backward(gy, x, wt, False)

    # the eight grid planes against torch on the GPU, float64
    x8 = x[:, edge].double().requires_grad_(True)
    y8 = R.torch_formulation(x8, wt[edge].double(), b[edge].double(), False)
    y8.backward(gy[:, edge].double())
    assert torch.equal(y[:, edge], y8.detach().to(dtype))
    assert torch.equal(gx[:, edge], x8.grad.to(dtype))
    del x8, y8

    mid = slice(4, C - 4)
    want_y = (b.double() + cx.double() * wt.double().sum((1, 2, 3))).to(dtype)
    assert bool((y[0, mid] == want_y[mid, None, None]).all())
    # response of every channel to gy = 1 on a 3x3 map: its nine border classes
    ones = torch.ones((1, C, 3, 3), dtype=torch.float64, device=DEV, requires_grad=True)
    R.torch_formulation(ones, wt.double(), None, False).sum().backward()
    klass = torch.ones(h, dtype=torch.long, device=DEV)
    klass[0], klass[-1] = 0, 2
    want_gx = (ones.grad[0][:, klass][:, :, klass] * cg.double()[:, None, None]).to(dtype)
    assert bool((gx[0, mid] == want_gx[mid]).all())
    assert torch.equal(gb.double()[mid], cg.double()[mid] * (4 * h * w))
    assert bool(torch.isfinite(gw).all())
    del x, gy, y, gx, gw, gb, want_gx
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------ c. rounding, real values
def assert_within(got, want64, bound, what):
    err = (got.detach().double().cpu() - want64).abs()
    worst = float((err - bound).max())
    print(f'{what}: max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e}, worst margin {worst:.3e}')
    assert bool((err <= bound).all()), what


@pytest.mark.parametrize('zeropad', MODES)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', ((2, 3, 9, 12), (2, 3, 17, 7)))
def test_rounding_bounds_on_normal_inputs(shape, dtype, zeropad):
    """accumulation is float32 and a half output is rounded once: the derived bounds of
    `upsampling_ref.bounds` (12 u M + r forward, 40 u M_gx + r for gx, (N + 2) u M for gW and gb),
    which the reference's own float32 CPU result has to meet on the same inputs as well"""
    x, gy, wt, b = normal_inputs(*shape, dtype, seed=sum(shape))
    want = dict(zip(('y', 'gx', 'gw', 'gb'), R.reference64(x, wt, b, gy, zeropad)))
    bound = R.bounds(x, wt, b, gy, zeropad, dtype)
    x32 = x.float().requires_grad_(True)
    w32, b32 = wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y32 = R.torch_formulation(x32, w32, b32, zeropad)
    y32.backward(gy.float())
    for k, t in (('y', y32), ('gx', x32.grad), ('gw', w32.grad), ('gb', b32.grad)):
        assert_within(t, want[k], bound[k], f'reference f32 {k}')        # else the bound is wrong
    y, gx, gw, gb, _ = run_op(x, gy, wt, b, zeropad)
    assert y.dtype == dtype and gx.dtype == dtype
    for k, t in (('y', y), ('gx', gx), ('gw', gw), ('gb', gb)):
        assert_within(t, want[k], bound[k], f'kernel {dtype} {k}')


# ------------------------------------------------------------------------------ d. fixture, module, training
def module_for(name):
    mode, use_bias, _, shape, _ = syn.UPSAMPLING_CASES[name]
    inp = syn.make_upsampling_inputs(name)
    m = up.Upsampling(mode, n_channels=shape[1], use_bias=use_bias)
    with torch.no_grad():
        if inp['weight'] is not None:
            m.conv.weight.copy_(torch.from_numpy(inp['weight']))
        if inp['bias'] is not None:
            m.conv.bias.copy_(torch.from_numpy(inp['bias']))
    return m.to(DEV), inp, mode == 'learned-3x3-zeropad'


@pytest.mark.parametrize('name', list(syn.UPSAMPLING_CASES))
def test_module_against_the_recorded_reference_module(name):
    g = _golden.load('upsampling')
    m, inp, zeropad = module_for(name)
    assert _golden.jload(g[f'{name}__params'])['digest'] == syn.upsampling_input_digest(inp)
    x = torch.from_numpy(inp['x']).to(DEV).requires_grad_(True)
    y = m(x)
    y.backward(torch.from_numpy(inp['gy']).to(DEV))
    bound = R.bounds(torch.from_numpy(inp['x']), m.conv.weight.detach().cpu(),
                     None if m.conv.bias is None else m.conv.bias.detach().cpu(),
                     torch.from_numpy(inp['gy']), zeropad, torch.float32)
    assert_within(y, torch.from_numpy(g[f'{name}__y']).double(), bound['y'], 'y')
    assert_within(x.grad, torch.from_numpy(g[f'{name}__gx']).double(), bound['gx'], 'gx')
    assert_within(m.conv.weight.grad, torch.from_numpy(g[f'{name}__gw']).double(), bound['gw'], 'gw')
    if m.conv.bias is not None:
        assert_within(m.conv.bias.grad, torch.from_numpy(g[f'{name}__gb']).double(), bound['gb'], 'gb')
    else:
        assert f'{name}__gb' not in g.files


def test_a_reference_shaped_state_dict_loads():
    gen = torch.Generator().manual_seed(4)
    state = {'conv.weight': torch.randn((6, 1, 3, 3), generator=gen), 'conv.bias': torch.randn((6,), generator=gen)}
    for mode in ('learned-3x3', 'learned-3x3-zeropad'):
        m = up.Upsampling(mode, n_channels=6).to(DEV)
        m.load_state_dict(state, strict=True)
        x = torch.randn((1, 6, 4, 8), generator=gen)
        want = R.reference64(x, state['conv.weight'], state['conv.bias'], torch.zeros(1, 6, 8, 16), 'zeropad' in mode)[0]
        bound = R.bounds(x, state['conv.weight'], state['conv.bias'], torch.zeros(1, 6, 8, 16), 'zeropad' in mode,
                         torch.float32)
        with torch.no_grad():
            assert_within(m(x.to(DEV)), want, bound['y'], mode)
    m = up.Upsampling('learned-3x3', n_channels=6, use_bias=False)
    with pytest.raises(RuntimeError):
        m.load_state_dict(state, strict=True)                   # the reference's keys, nothing more


@pytest.mark.parametrize('zeropad', MODES)
def test_an_sgd_step_moves_the_parameters_like_the_torch_formulation(zeropad):
    """training=True, one step of torch.optim.SGD: the parameters end where the torch formulation's
    end, within lr * (the gradient bounds of (c)) plus the update's own rounding (u * |p'| for each
    of the two float32 updates)"""
    lr, shape = 0.1, (2, 3, 9, 12)
    x, gy, wt, b = normal_inputs(*shape, torch.float32, seed=77)
    m = up.Upsampling('learned-3x3-zeropad' if zeropad else 'learned-3x3', n_channels=3).to(DEV).train()
    with torch.no_grad():
        m.conv.weight.copy_(wt)
        m.conv.bias.copy_(b)
    wt_t, b_t = torch.nn.Parameter(wt.to(DEV)), torch.nn.Parameter(b.to(DEV))
    opt_m, opt_t = torch.optim.SGD(m.parameters(), lr=lr), torch.optim.SGD([wt_t, b_t], lr=lr)
    xd, gyd = dev(x, gy)
    (m(xd) * gyd).sum().backward()
    (R.torch_formulation(xd, wt_t, b_t, zeropad) * gyd).sum().backward()
    opt_m.step()
    opt_t.step()
    bound = R.bounds(x, wt, b, gy, zeropad, torch.float32)
    assert m.training and not torch.equal(m.conv.weight.detach().cpu(), wt) and not torch.equal(m.conv.bias.detach().cpu(), b)
    for got, ref, bd in ((m.conv.weight, wt_t, bound['gw']), (m.conv.bias, b_t, bound['gb'])):
        ref64 = ref.detach().double().cpu()
        assert_within(got, ref64, lr * bd + 2 * R.U * ref64.abs(), 'parameter after the step')


# ------------------------------------------------------------------------------ e. autocast
@pytest.mark.parametrize('zeropad', MODES)
def test_autocast_gives_the_autocast_dtype(zeropad):
    x, gy, wt, b = normal_inputs(2, 3, 9, 12, torch.float32, seed=88)
    m = up.Upsampling('learned-3x3-zeropad' if zeropad else 'learned-3x3', n_channels=3).to(DEV)
    with torch.no_grad():
        m.conv.weight.copy_(wt)
        m.conv.bias.copy_(b)
    xd = x.to(DEV).requires_grad_(True)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        y = m(xd)
    assert y.dtype == torch.bfloat16 and m.conv.weight.dtype == torch.float32
    xr = x.bfloat16()
    want = R.reference64(xr, wt, b, gy.bfloat16(), zeropad)
    bound = R.bounds(xr, wt, b, gy.bfloat16(), zeropad, torch.bfloat16)
    assert_within(y, want[0], bound['y'], 'autocast y')
    y.backward(gy.bfloat16().to(DEV))
    assert xd.grad.dtype == torch.float32 and m.conv.weight.grad.dtype == torch.float32
    assert_within(m.conv.weight.grad, want[2], bound['gw'], 'autocast gw')
    assert_within(m.conv.bias.grad, want[3], bound['gb'], 'autocast gb')
    with torch.autocast('cuda', dtype=torch.bfloat16):         # the plain modes: interpolate, dtype kept
        assert up.Upsampling('bilinear', 3)(x.to(DEV)).dtype == torch.float32


# ------------------------------------------------------------------------------ f. determinism, streams, graphs
def test_backward_twice_gives_identical_bytes():
    for dtype, shape in ((torch.float32, (4, 5, 33, 40)), (torch.bfloat16, (3, 4, 17, 37))):
        x, gy, wt, b = dev(*normal_inputs(*shape, dtype, seed=9))
        first = ops.upsample2x_dw3x3_backward(gy, x, wt, False)
        second = ops.upsample2x_dw3x3_backward(gy, x, wt, False)
        for a, e in zip(first, second):
            assert torch.equal(a.view(torch.uint8), e.view(torch.uint8))


def test_side_stream():
    x, gy, wt, b = dev(*normal_inputs(2, 3, 17, 24, torch.float32, seed=12))
    want = (ops.upsample2x_dw3x3(x, wt, b, True),) + ops.upsample2x_dw3x3_backward(gy, x, wt, True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        got = (ops.upsample2x_dw3x3(x, wt, b, True),) + ops.upsample2x_dw3x3_backward(gy, x, wt, True)
    side.synchronize()
    for a, e in zip(got, want):
        assert torch.equal(a, e)


def test_graph_capture_and_replay():
    """forward and backward captured in one torch.cuda.graph after an eager warm-up, replayed twice
    with new input contents: the eager results bit for bit.  The capture is a single chain on one
    stream; nothing about queues is set."""
    shape, dtype = (2, 3, 17, 24), torch.float32
    inputs = [dev(*normal_inputs(*shape, dtype, seed=s)) for s in (1, 2, 3)]
    xs, gys, wt, b = (t.clone() for t in inputs[0])

    def step():
        return (ops.upsample2x_dw3x3(xs, wt, b, False),) + ops.upsample2x_dw3x3_backward(gys, xs, wt, False)

    step()                                                       # eager warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for x, gy, _, _ in inputs[1:]:
        xs.copy_(x)
        gys.copy_(gy)
        graph.replay()
        torch.cuda.synchronize()
        eager = (ops.upsample2x_dw3x3(x, wt, b, False),) + ops.upsample2x_dw3x3_backward(gy, x, wt, False)
        for a, e in zip(outs, eager):
            assert torch.equal(a, e)
    del graph


# ------------------------------------------------------------------------------ g. non-contiguous input
@pytest.mark.parametrize('dtype', (torch.float32, torch.float16))
def test_non_contiguous_inputs(dtype):
    x, gy, wt, b = dev(*normal_inputs(2, 4, 9, 12, dtype, seed=14))
    xcl = x.to(memory_format=torch.channels_last)
    gyt = gy.transpose(2, 3).contiguous().transpose(2, 3)
    assert not xcl.is_contiguous() and not gyt.is_contiguous()
    assert torch.equal(ops.upsample2x_dw3x3(xcl, wt, b, False), ops.upsample2x_dw3x3(x, wt, b, False))
    for a, e in zip(ops.upsample2x_dw3x3_backward(gyt, xcl, wt, False), ops.upsample2x_dw3x3_backward(gy, x, wt, False)):
        assert torch.equal(a, e)
    m = up.Upsampling('learned-3x3', n_channels=4).to(DEV)
    grads = []
    for xi, gi in ((x, gy), (xcl, gyt)):
        m.zero_grad()
        xi = xi.detach().requires_grad_(True)
        m(xi).backward(gi)
        grads.append((xi.grad.contiguous(), m.conv.weight.grad.clone(), m.conv.bias.grad.clone()))
    for a, e in zip(*grads):
        assert torch.equal(a, e)
