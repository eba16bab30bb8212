"""GPU tier of the fused x2 upsampling + skip addition (csrc/up_add.hip, ops.up2x_add).

Oracle: `testing.up_add_ref.reference64`, float64 on the CPU from the same, already dtype-rounded inputs: nearest
and bilinear as ATen's weight matrices, the learned modes as the reference's formulation in torch ops.

Launch geometry the shapes are picked from (csrc/up_add.hip, the one of csrc/upsampling.hip): a lane owns a run
of 2 (f32) or 4 (half) input pixels on the vector route and 1 on the one-pixel route; a wave spans 64 runs (128 / 256
/ 64 pixels), a workgroup of 256 lanes 512 / 1024 / 256 pixels of a row; a lane walks a tile of 8 input rows; a
plane's (tile, run) units are split into chunks of 256; the grid is capped at 8 workgroups per compute unit.
"""
import itertools

import pytest
import torch
import torch.nn.functional as F

from nicr_mt_scene_analysis_amd import _lib as L
from nicr_mt_scene_analysis_amd import ops
from nicr_mt_scene_analysis_amd.testing import up_add_ref as R
from nicr_mt_scene_analysis_amd.testing import upsampling_ref as UR

from _gpu_support import assume_cus     # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
MODES = R.MODES
VECTOR, PIXEL = L.NMSA_UPADD_ROUTE_VECTOR, L.NMSA_UPADD_ROUTE_PIXEL
RUN = {torch.float32: 2, torch.bfloat16: 4, torch.float16: 4}


# ------------------------------------------------------------------------------ helpers
def dev(*tensors):
    return tuple(None if t is None else t.to(DEV) for t in tensors)


def run_op(x, skip, mode, wt, b):
    xd, sd, wd, bd = dev(x, skip, wt, b)
    y = ops.up2x_add(xd, sd, mode, wd, bd)
    return y, ops.up2x_add_route(xd, sd, y)


def check_exact(shape, dtype, mode, seed=0, bias=True):
    """integers in -8..8 for x and skip, k/16 for W and b: every product and every sum of the four modes is exact
    in float32 (the bilinear weights are 1/4 and 3/4), so the result is the float64 value, cast once"""
    x, skip, _, wt, b = R.make_inputs(shape, dtype, seed, integer=True, bias=bias)
    y, route = run_op(x, skip, mode, wt, b)
    tag = (shape, dtype, mode)
    assert y.dtype == dtype and tuple(y.shape) == tuple(skip.shape), tag
    assert torch.equal(y.cpu(), R.reference64(x, skip, mode, wt, b).to(dtype)), tag
    assert route == (VECTOR if shape[3] % RUN[dtype] == 0 else PIXEL), tag
    return route


# ------------------------------------------------------------------------------ a. exact, integer grid
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', DTYPES)
def test_exact_smallest_maps(dtype, mode):
    """h, w in {1, 2, 3}: every pixel is a border pixel, at h = 1 / w = 1 of both sides at once"""
    for h, w in itertools.product((1, 2, 3), repeat=2):
        check_exact((2, 3, h, w), dtype, mode, seed=10 * h + w)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', DTYPES)
def test_exact_width_edges(dtype, mode):
    """w one below, at and above: the lane run (2 for f32, 4 for half), a wave's span (64 runs: 128 / 256 pixels on
    the vector route, 64 pixels on the one-pixel route that the odd widths take), a workgroup's row span (256 runs:
    512 / 1024 pixels, 256 on the one-pixel route); the nearest widths that stay on the vector route (w +- run) ride
    along.  h = 3 keeps both borders and an interior row."""
    run = RUN[dtype]
    widths = {run - 1, run, run + 1, 63, 64, 65, 255, 256, 257}
    for span in (64 * run, 256 * run):
        widths |= {span - run, span - 1, span, span + 1, span + run}
    routes = {check_exact((1, 2, 3, w), dtype, mode, seed=w) for w in sorted(widths)}
    assert routes == {VECTOR, PIXEL}


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', DTYPES)
def test_exact_height_edges(dtype, mode):
    """h one below, at and above the tile height (8) and twice it; w = 8 is the vector route of every dtype, w = 7
    the one-pixel route; 40 runs and 129 columns with h = 17 put a tile border and a chunk border (256 units)
    inside one plane"""
    for h, w in itertools.product((7, 8, 9, 15, 16, 17), (8, 7)):
        check_exact((2, 2, h, w), dtype, mode, seed=h)
    for h, w in ((17, 40 * RUN[dtype]), (17, 129)):
        check_exact((1, 3, h, w), dtype, mode, seed=w)


@pytest.mark.parametrize('mode', MODES)
def test_exact_plane_counts(mode, assume_cus):
    """B*C in {1, 2, 5}, and, with the library told of one compute unit (a grid of 8 workgroups), 9 planes of one
    chunk and 5 planes of two: the grid-stride loop runs a second trip, with another channel in it"""
    check_exact((1, 1, 5, 6), torch.float32, mode)
    check_exact((2, 1, 5, 6), torch.float32, mode)
    check_exact((1, 5, 5, 6), torch.bfloat16, mode)
    assert assume_cus(1) == 1
    check_exact((3, 3, 5, 6), torch.float32, mode, seed=1)
    check_exact((1, 5, 17, 129), torch.float16, mode, seed=2)
    check_exact((3, 3, 9, 8), torch.bfloat16, mode, seed=3)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', DTYPES)
def test_exact_without_bias(dtype, mode):
    for h, w in ((3, 4), (9, 5)):
        check_exact((2, 3, h, w), dtype, mode, bias=False)


# ------------------------------------------------------------------------------ b. nearest: torch's bits
@pytest.mark.parametrize('dtype', DTYPES)
def test_nearest_equals_torch_bit_for_bit(dtype):
    """one IEEE addition of the same two values: float32 inside and one rounding are what torch's half addition
    does as well"""
    for shape in R.BOUNDS_SHAPES + ((1, 2, 3, 1024), (2, 2, 8, 65)):
        x, skip, _, _, _ = dev(*R.make_inputs(shape, dtype, seed=sum(shape)))
        want = F.interpolate(x, scale_factor=2, mode='nearest') + skip
        got = ops.up2x_add(x, skip, 'nearest')
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), (shape, dtype)


# ------------------------------------------------------------------------------ c. rounding, real values
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', R.BOUNDS_SHAPES)
def test_rounding_bounds_on_normal_inputs(shape, dtype, mode):
    """float32 inside, one rounding after the addition: the derived bounds of `up_add_ref.bounds`
    (gamma_5 (sum w |x| + |skip|) + r bilinear, 13 u (M + |skip|) + r learned, u |y| + r nearest), which torch's own
    float32 result meets on the same inputs (tests/test_up_add_host.py)"""
    x, skip, _, wt, b = R.make_inputs(shape, dtype, R.bounds_seed(shape))
    want = R.reference64(x, skip, mode, wt, b)
    bound = R.bounds(x, skip, mode, wt, b, dtype)
    y, _ = run_op(x, skip, mode, wt, b)
    worst = R.worst_ratio(y, want, bound)
    print(f'kernel {mode} {dtype} {shape}: worst error / bound {worst:.3f}')
    assert y.dtype == dtype and worst <= 1.0


# ------------------------------------------------------------------------------ d. routes, poison, strides
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', DTYPES)
def test_both_routes_and_an_offset_output_with_poison(dtype, mode):
    """the same even-width call on the vector route and, with y one element into a larger allocation (off 16
    bytes), on the one-pixel route: the same values, and the poison in front of and behind y's range is intact
    before and after"""
    shape = (2, 3, 9, 16)
    x, skip, _, wt, b = R.make_inputs(shape, dtype, seed=21, integer=True)
    want = R.reference64(x, skip, mode, wt, b).to(dtype)
    xd, sd, wd, bd = dev(x, skip, wt, b)
    y = ops.up2x_add(xd, sd, mode, wd, bd)
    assert ops.up2x_add_route(xd, sd, y) == VECTOR
    n = y.numel()
    buf = torch.full((n + 64,), 1024.0, dtype=dtype, device=DEV)
    view = buf[1:1 + n].view(y.shape)
    assert ops.up2x_add_route(xd, sd, view) == PIXEL
    assert buf[0].item() == 1024.0 and bool((buf[1 + n:] == 1024.0).all())
    out = ops.up2x_add(xd, sd, mode, wd, bd, out=view)
    assert out.data_ptr() == view.data_ptr() == buf.data_ptr() + buf.element_size()
    assert torch.equal(view, y) and torch.equal(y.cpu(), want)
    assert buf[0].item() == 1024.0 and bool((buf[1 + n:] == 1024.0).all())
    # inputs one element into their allocations: the one-pixel route as well, the same bits
    for which in ('x', 'skip'):
        t = xd if which == 'x' else sd
        off = torch.zeros((t.numel() + 8,), dtype=dtype, device=DEV)[1:1 + t.numel()].view(t.shape).copy_(t)
        args = (off, sd) if which == 'x' else (xd, off)
        got = ops.up2x_add(*args, mode, wd, bd)
        assert ops.up2x_add_route(*args, got) == PIXEL and torch.equal(got, y), which


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', (torch.float32, torch.float16))
def test_non_contiguous_inputs(dtype, mode):
    x, skip, _, wt, b = dev(*R.make_inputs((2, 4, 9, 12), dtype, seed=14))
    xcl = x.to(memory_format=torch.channels_last)
    st = skip.transpose(2, 3).contiguous().transpose(2, 3)
    assert not xcl.is_contiguous() and not st.is_contiguous()
    want = ops.up2x_add(x, skip, mode, wt, b)
    for a, s in ((xcl, skip), (x, st), (xcl, st)):
        assert torch.equal(ops.up2x_add(a, s, mode, wt, b).view(torch.uint8), want.view(torch.uint8))


def test_the_wrapper_refuses_what_it_should():
    x, skip, _, wt, b = dev(*R.make_inputs((1, 2, 3, 4), torch.float32, 1))
    with pytest.raises(TypeError):
        ops.up2x_add(x.double(), skip.double(), 'nearest')
    with pytest.raises(TypeError):
        ops.up2x_add(x, skip.half(), 'nearest')
    with pytest.raises(TypeError):
        ops.up2x_add(x, skip, 'learned-3x3')                # no weight
    with pytest.raises(TypeError):
        ops.up2x_add(x, skip, 'learned-3x3', wt.half(), b)
    with pytest.raises(ValueError):
        ops.up2x_add(x, skip[..., :-1], 'nearest')
    with pytest.raises(ValueError):
        ops.up2x_add(x[0], skip[0], 'nearest')
    with pytest.raises(L.NmsaError):
        ops.up2x_add(x.cpu(), skip, 'nearest')
    with pytest.raises(L.NmsaError):
        ops.up2x_add(x, skip.cpu(), 'nearest')
    with pytest.raises(L.NmsaError):                        # y overlaps skip: refused by the library's host check
        ops.up2x_add(x, skip, 'nearest', out=skip)
    # weight and bias are ignored in the other two modes
    assert torch.equal(ops.up2x_add(x, skip, 'bilinear', wt, b), ops.up2x_add(x, skip, 'bilinear'))


# ------------------------------------------------------------------------------ e. non-finite values
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', DTYPES)
def test_non_finite_values_land_where_torch_puts_them(dtype, mode):
    """a 5x6 map with an infinity in row 1 and a NaN in the interior, a skip with an infinity at a corner: NaN,
    +inf and -inf sit where the torch composition on the device puts them.  Bilinear: the infinity of row 1 lies
    next to the zero-weight tap of output row 0, which is multiplied (ATen's NaN).  Learned: the kernel multiplies
    PRE-ADDED weight pairs, so with weights of mixed sign an infinity could give inf where the nine separate
    products give inf - inf; the weights here are positive, which leaves one answer, and the composition is
    written as nine shifted views and a sum (`upsampling_ref.unfold_formulation`), not as a library convolution."""
    gen = torch.Generator().manual_seed(5)
    x = torch.randn((1, 2, 5, 6), generator=gen)
    skip = torch.randn((1, 2, 10, 12), generator=gen)
    wt = torch.rand((2, 1, 3, 3), generator=gen) * 0.25 + 0.05
    b = torch.randn((2,), generator=gen)
    x[0, 0, 1, 2], x[0, 1, 1, 0] = float('inf'), float('-inf')
    x[0, 0, 3, 3], x[0, 1, 2, 4] = float('nan'), float('nan')
    skip[0, 0, 0, 0], skip[0, 1, 9, 11] = float('-inf'), float('inf')
    x, skip, wt, b = dev(x.to(dtype), skip.to(dtype), wt, b)
    if R.is_learned(mode):
        u = UR.unfold_formulation(x.float(), wt, b, mode.endswith('zeropad')).to(dtype)
        want = torch.add(skip, u)
    else:
        want = R.torch_up_add(x, skip, mode)
    got = ops.up2x_add(x, skip, mode, wt, b)
    assert bool(torch.isnan(want).any()) and bool(torch.isposinf(want).any()) and bool(torch.isneginf(want).any())
    assert torch.equal(torch.isnan(got), torch.isnan(want)), mode
    assert torch.equal(torch.isposinf(got), torch.isposinf(want)), mode
    assert torch.equal(torch.isneginf(got), torch.isneginf(want)), mode
    if mode == 'bilinear':                                  # the zero-weight tap of output row 0 under the infinity
        assert bool(torch.isnan(got[0, 0, 0, 4:6]).all())


# ------------------------------------------------------------------------------ f. beyond 2^31 elements
@pytest.mark.parametrize('mode', ('bilinear', 'learned-3x3'))
def test_more_than_two_to_the_31_output_elements(mode):
    """float16 [1, 2049, 512, 512]: 2049 * 4 * 512 * 512 = 2^31 + 2^20 output elements, so the last planes lie
    behind a 32-bit element offset.  The first and the last four planes hold grid values and equal torch's float64
    result on the GPU for those eight planes alone; every other plane holds one constant x, for which u is one
    constant per channel (the bilinear weights sum to 1; b + x sum(W) under replication), and a skip that changes
    with row, column and channel: y = u_c + skip, exact in float16, compared on the device in slabs."""
    C, h, w, dtype = 2049, 512, 512, torch.float16
    gen = torch.Generator().manual_seed(31)
    wt = (torch.randint(-8, 9, (C, 1, 3, 3), generator=gen).float() / 16).to(DEV)
    b = (torch.randint(-8, 9, (C,), generator=gen).float() / 16).to(DEV)
    cx = torch.randint(-8, 9, (C,), generator=gen).to(DEV)
    edge = torch.tensor([0, 1, 2, 3, C - 4, C - 3, C - 2, C - 1], device=DEV)
    x = cx.to(dtype)[None, :, None, None].expand(1, C, h, w).contiguous()
    torch.manual_seed(32)
    x[0, edge] = torch.randint(-8, 9, (8, h, w), device=DEV).to(dtype)
    rows = torch.arange(2 * h, device=DEV, dtype=torch.int16)[None, :, None]
    cols = torch.arange(2 * w, device=DEV, dtype=torch.int16)[None, None, :]
    chan = torch.arange(C, device=DEV, dtype=torch.int16)[:, None, None]
    skip = (((rows + 3 * cols + 5 * chan) % 17) - 8).to(dtype)[None]
    assert skip.numel() > 1 << 31 and skip.is_contiguous()

    y = ops.up2x_add(x, skip, mode, wt, b)

    x8, s8 = x[:, edge].double(), skip[:, edge].double()
    want8 = R.torch_up_add(x8, s8, mode, wt[edge].double(), b[edge].double())
    assert torch.equal(y[:, edge], want8.to(dtype))
    del x8, s8, want8
    uc64 = cx.double() if mode == 'bilinear' else b.double() + cx.double() * wt.double().sum((1, 2, 3))
    uc = uc64.to(dtype)
    assert torch.equal(uc.double(), uc64)
    for lo in range(4, C - 4, 256):
        hi = min(lo + 256, C - 4)
        assert torch.equal(y[0, lo:hi], uc[lo:hi, None, None] + skip[0, lo:hi]), (lo, hi)
    del x, skip, y
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------ g. graphs
def test_graph_capture_and_replay():
    """all four modes captured in one torch.cuda.graph after an eager warm-up, replayed three times with new input
    contents: the eager results bit for bit.  The capture is a single chain on the current stream; nothing about
    queues is set."""
    shape, dtype = (2, 3, 17, 24), torch.float32
    inputs = [dev(*R.make_inputs(shape, dtype, seed=s)) for s in (1, 2, 3, 4)]
    xs, ss, _, wt, b = (t.clone() for t in inputs[0])

    def step(x, s):
        return tuple(ops.up2x_add(x, s, mode, wt, b) for mode in MODES)

    step(xs, ss)                                                 # eager warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(xs, ss)
    for x, s, _, _, _ in inputs[1:]:
        xs.copy_(x)
        ss.copy_(s)
        graph.replay()
        torch.cuda.synchronize()
        for a, e in zip(outs, step(x, s)):
            assert torch.equal(a.view(torch.uint8), e.view(torch.uint8))
    del graph
