"""GPU tier: the stem max pool (csrc/maxpool.hip, ops.maxpool3x3s2*, model.pooling.MaxPool2d) against the
restatement of testing/maxpool_ref.py, which tests/test_maxpool_ref.py holds to ATen's CPU float32 pool: y bit
for bit, the codes against ATen's converted CPU indices, gx bit for bit against the float32 ordered gather
rounded once.  The halves are held to that gather on the upcast gy and not to ATen's half backward, which
rounds after every add.  Both routes: the one-pixel route is forced by an odd width and by a storage offset of
one element."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from nicr_mt_scene_analysis_amd import _lib as L
from nicr_mt_scene_analysis_amd import model, ops
from nicr_mt_scene_analysis_amd.model import pooling
from nicr_mt_scene_analysis_amd.testing import maxpool_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = (F32, BF16, F16)
SHAPES = ((1, 1, 1, 1), (1, 1, 2, 2), (1, 2, 3, 3), (2, 3, 7, 9), (2, 3, 8, 8), (1, 2, 9, 16), (2, 2, 6, 24),
          (1, 1, 5, 259), (1, 1, 130, 6))
VECTOR, PIXEL = L.NMSA_MP_ROUTE_VECTOR, L.NMSA_MP_ROUTE_PIXEL
_CASES = {}


def case(shape, dtype):
    """x, gy (of `dtype`, on the CPU) and the expected y, code, gx; computed once, never modified"""
    key = (shape, dtype)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(sum(shape) * 7 + 1)
        x = torch.randn(shape, generator=gen).to(dtype)
        # ties within a window: a quarter of the map on a coarse grid
        coarse = (x.float() * 2).round() / 2
        x = torch.where(torch.rand(shape, generator=gen) < 0.25, coarse, x.float()).to(dtype)
        y, code = R.forward(x)
        idx = F.max_pool2d(x.float(), 3, 2, 1, return_indices=True)[1]
        assert torch.equal(R.index_to_code(idx, *shape[2:]), code)
        gy = torch.randn(y.shape, generator=gen).to(dtype)
        gx = R.backward_f32(gy, code, *shape[2:]).to(dtype)
        _CASES[key] = dict(x=x, gy=gy, y=y, code=code, gx=gx)
    return _CASES[key]


def shifted(t):
    """the same values one element off the allocation's start: element-aligned, off 16 bytes"""
    buf = torch.empty((t.numel() + 16,), dtype=t.dtype, device=DEV)
    out = buf[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 != 0
    return out


def expected_route(shape, dtype, offset):
    return VECTOR if not offset and shape[3] % (4 if dtype == F32 else 8) == 0 else PIXEL


@pytest.mark.parametrize('offset', (False, True), ids=('aligned', 'offset'))
@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_forward_and_backward_bit_equal(shape, dtype, offset):
    c = case(shape, dtype)
    place = shifted if offset else (lambda t: t)
    x, gy = place(c['x'].to(DEV)), place(c['gy'].to(DEV))
    y, code = ops.maxpool3x3s2(x)
    assert ops.maxpool3x3s2_route(x, y, code) == expected_route(shape, dtype, offset)
    gx = ops.maxpool3x3s2_backward(gy, code, shape[2:])
    assert ops.maxpool3x3s2_route(gx, gy, code) == expected_route(shape, dtype, offset)
    assert y.dtype == dtype and code.dtype == torch.uint8 and gx.dtype == dtype and gx.shape == x.shape
    assert torch.equal(code.cpu(), c['code'])
    assert R.same_bits(y.cpu(), c['y'])
    assert R.same_bits(gx.cpu(), c['gx'])
    # two calls give the same bits; the inference call gives the same y
    y2, code2 = ops.maxpool3x3s2(x)
    gx2 = ops.maxpool3x3s2_backward(gy, code2, shape[2:])
    y3, none = ops.maxpool3x3s2(x, need_code=False)
    assert none is None
    assert R.same_bits(y2.cpu(), y.cpu()) and R.same_bits(y3.cpu(), y.cpu()) and R.same_bits(gx2.cpu(), gx.cpu())


def test_both_routes_are_taken_by_the_shapes():
    taken = {(d, expected_route(s, d, False)) for s in SHAPES for d in DTYPES}
    assert taken == {(d, r) for d in DTYPES for r in (VECTOR, PIXEL)}


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('name', sorted(R.special_maps()))
def test_special_value_maps(name, dtype):
    x = R.special_maps()[name].to(dtype)
    want_y, want_code = R.forward(x)
    idx = F.max_pool2d(x.float(), 3, 2, 1, return_indices=True)[1]
    assert torch.equal(R.index_to_code(idx, 7, 9), want_code)
    gy = torch.randn(want_y.shape, generator=torch.Generator().manual_seed(3)).to(dtype)
    # the vector route too: the same map widened to 16 columns by a copy of its first seven
    wide = torch.cat([x, x[..., :7]], dim=3)
    for xin in (x, wide):
        H, W = xin.shape[2:]
        wy, wc = R.forward(xin)
        y, code = ops.maxpool3x3s2(xin.to(DEV))
        g = gy if xin is x else torch.cat([gy, gy[..., :3]], dim=3)
        gx = ops.maxpool3x3s2_backward(g.to(DEV), code, (H, W))
        assert torch.equal(code.cpu(), wc), name
        assert R.same_bits(y.cpu(), wy), name
        assert R.same_bits(gx.cpu(), R.backward_f32(g, wc, H, W).to(dtype)), name


def test_nonfinite_gradients_pass_through_their_own_pixel_only():
    x = torch.randn((1, 1, 8, 8), generator=torch.Generator().manual_seed(9))
    _, code = R.forward(x)
    gy = torch.ones((1, 1, 4, 4))
    gy[0, 0, 1, 1], gy[0, 0, 2, 2] = float('nan'), float('inf')
    gx = ops.maxpool3x3s2_backward(gy.to(DEV), code.to(DEV), (8, 8)).cpu()
    want = R.backward_f32(gy, code, 8, 8)
    assert R.same_bits(gx, want) and int(torch.isnan(gx).sum()) == 1 and int(torch.isinf(gx).sum()) == 1


# ------------------------------------------------------------------------------ the module
def test_module_is_one_node_that_saves_the_code_alone():
    m = model.MaxPool2d(kernel_size=3, stride=2, padding=1)
    assert isinstance(m, nn.MaxPool2d)
    c = case((2, 3, 8, 8), F32)
    x = c['x'].to(DEV).requires_grad_(True)
    y = m(x)
    assert type(y.grad_fn).__name__ == 'MaxPool3x3S2FunctionBackward'
    saved = y.grad_fn.saved_tensors
    assert len(saved) == 1 and saved[0].dtype == torch.uint8 and saved[0].shape == y.shape
    y.backward(c['gy'].to(DEV))
    assert R.same_bits(y.detach().cpu(), c['y']) and R.same_bits(x.grad.cpu(), c['gx'])
    with pytest.raises(RuntimeError):
        x2 = c['x'].to(DEV).requires_grad_(True)
        g, = torch.autograd.grad(m(x2), x2, c['gy'].to(DEV), create_graph=True)
        g.sum().backward()                              # once_differentiable: no double backward


def test_no_grad_call_allocates_no_code(monkeypatch):
    calls = []
    real = ops.maxpool3x3s2
    monkeypatch.setattr(ops, 'maxpool3x3s2', lambda x, need_code=True, out=None: calls.append(need_code) or real(x, need_code, out))
    m = model.MaxPool2d(3, 2, 1)
    x = case((2, 3, 8, 8), BF16)['x'].to(DEV)
    m(x)                                                # x needs no gradient
    with torch.no_grad():
        y = m(x.clone().requires_grad_(True))
    assert not y.requires_grad
    m(x.clone().requires_grad_(True))
    assert calls == [False, False, True]
    big = torch.zeros((2, 3, 64, 64), dtype=BF16, device=DEV)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        out = m(big)
    assert out.numel() * 2 == 12288 and torch.cuda.memory_allocated() - before == 12288        # y alone, no 6144 of code


@pytest.mark.parametrize('what', ('kernel', 'stride', 'padding', 'dilation', 'ceil', 'indices', 'cpu', '3d',
                                  'channels_last', 'strided', 'float64', 'default_stride'))
def test_every_fallback_condition_reaches_nn_maxpool2d(monkeypatch, what):
    def refuse(*a, **k):
        raise AssertionError('the library must not be called on this path')
    monkeypatch.setattr(ops, 'maxpool3x3s2', refuse)
    kw = dict(kernel_size=3, stride=2, padding=1)
    kw.update({'kernel': dict(kernel_size=2, padding=0), 'stride': dict(stride=1), 'padding': dict(padding=0),
               'dilation': dict(dilation=2), 'ceil': dict(ceil_mode=True), 'indices': dict(return_indices=True),
               'default_stride': dict(stride=None)}.get(what, {}))
    m = model.MaxPool2d(**kw)
    x = torch.randn((2, 4, 9, 10), generator=torch.Generator().manual_seed(2))
    x = {'cpu': lambda: x, '3d': lambda: x[0].to(DEV), 'float64': lambda: x.double().to(DEV),
         'channels_last': lambda: x.to(DEV).contiguous(memory_format=torch.channels_last),
         'strided': lambda: x.to(DEV)[:, :, :, ::2]}.get(what, lambda: x.to(DEV))()
    assert not m.takes_hip_path(x)
    got = m(x)
    want = nn.MaxPool2d(**kw)(x)
    if what == 'indices':
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    else:
        assert torch.equal(got, want)


def test_captured_forward_and_backward_replay_on_fresh_contents():
    shape = (2, 3, 9, 16)
    m = model.MaxPool2d(3, 2, 1)
    a, b = case(shape, F16), case((2, 3, 9, 16), BF16)
    x = a['x'].to(DEV).requires_grad_(True)
    gy = a['gy'].to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gx0, = torch.autograd.grad(m(x), x, gy)         # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = m(x)
        gx, = torch.autograd.grad(y, x, gy)
    fresh = b['x'].float().to(F16)                      # other contents in the same dtype
    fy, fcode = R.forward(fresh)
    fgy = b['gy'].float().to(F16)
    with torch.no_grad():
        x.copy_(fresh.to(DEV))
        gy.copy_(fgy.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert R.same_bits(y.detach().cpu(), fy)
    assert R.same_bits(gx.cpu(), R.backward_f32(fgy, fcode, 9, 16).to(F16))
    assert R.same_bits(gx0.cpu(), a['gx'])


@pytest.mark.parametrize('dtype', (BF16, F16), ids=str)
def test_autocast_keeps_the_input_dtype(dtype):
    m = model.MaxPool2d(3, 2, 1)
    for given in (F32, dtype):
        x = case((2, 3, 8, 8), given)['x'].to(DEV).requires_grad_(True)
        with torch.autocast('cuda', dtype=dtype):
            y = m(x)
            want = F.max_pool2d(x.detach(), 3, 2, 1)
        assert y.dtype == given == want.dtype and type(y.grad_fn).__name__ == 'MaxPool3x3S2FunctionBackward'
        assert R.same_bits(y.detach(), want)


def test_ops_refuse_what_the_kernels_do_not_take():
    x = torch.zeros((1, 1, 4, 4), device=DEV)
    with pytest.raises(TypeError):
        ops.maxpool3x3s2(x.double())
    with pytest.raises(TypeError):
        ops.maxpool3x3s2(x.expand(2, 2, 4, 4))
    with pytest.raises(L.NmsaError):
        ops.maxpool3x3s2(x.cpu())
    y, code = ops.maxpool3x3s2(x)
    with pytest.raises(TypeError):
        ops.maxpool3x3s2_backward(y, code.long(), (4, 4))
    with pytest.raises(TypeError):
        ops.maxpool3x3s2_backward(y, code, (5, 5))
    assert pooling.MaxPool3x3S2Function is model.MaxPool3x3S2Function
