"""GPU tier: the scene head (csrc/scene_head.hip, ops.scene_head*, model.decoder.SceneClassificationDecoder)
against the restatement of testing/scene_head_ref.py, which tests/test_scene_decoder_ref.py holds to the
reference's decoder: logits, pooled, gx, gweight and gbias bit for bit.  Half inputs are upcast for the
restatement (exact) and outputs are rounded once.  All three routes: the element route is forced by a plane size
off the chunk and by a storage offset of one element."""
import pytest
import torch

from nicr_mt_scene_analysis_amd import _lib as L
from nicr_mt_scene_analysis_amd import model, ops
from nicr_mt_scene_analysis_amd.model.decoder import scene as scene_module
from nicr_mt_scene_analysis_amd.testing import scene_head_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = (F32, BF16, F16)
SHAPES = R.SCENE_HEAD_SHAPES
UNIT, VECTOR, ELEMENT = L.NMSA_SH_ROUTE_UNIT, L.NMSA_SH_ROUTE_VECTOR, L.NMSA_SH_ROUTE_ELEMENT
_CASES = {}


def case(shape, dtype):
    """x, g (of `dtype`), weight, bias (float32) on the CPU and the expected results; computed once, never
    modified"""
    key = (shape, dtype)
    if key not in _CASES:
        B, C, H, W, K = shape
        gen = torch.Generator().manual_seed(sum(shape) * 11 + 3)
        x = torch.randn((B, C, H, W), generator=gen).to(dtype)
        weight = torch.randn((K, C), generator=gen) / C ** 0.5
        bias = 0.1 * torch.randn((K,), generator=gen)
        g = torch.randn((B, K), generator=gen).to(dtype)
        logits, pooled = R.forward(x, weight, bias)
        gx, gw, gb = R.backward(g, pooled, weight, x.shape, dtype)
        _CASES[key] = dict(x=x, weight=weight, bias=bias, g=g, logits=logits, pooled=pooled, gx=gx, gw=gw, gb=gb)
    return _CASES[key]


def shifted(t):
    """the same values one element off the allocation's start: element-aligned, off 16 bytes"""
    buf = torch.empty((t.numel() + 16,), dtype=t.dtype, device=DEV)
    out = buf[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 != 0
    return out


def expected_route(shape, dtype, offset):
    hw = shape[2] * shape[3]
    if hw == 1:
        return UNIT
    return VECTOR if not offset and hw % (4 if dtype == F32 else 8) == 0 else ELEMENT


@pytest.mark.parametrize('offset', (False, True), ids=('aligned', 'offset'))
@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_forward_and_backward_bit_equal(shape, dtype, offset):
    c = case(shape, dtype)
    K = shape[4]
    place = shifted if offset else (lambda t: t)
    x, g = place(c['x'].to(DEV)), place(c['g'].to(DEV))
    weight, bias = c['weight'].to(DEV), c['bias'].to(DEV)
    aligned = ops.scene_head_route(c['x'].to(DEV), K)
    assert aligned == expected_route(shape, dtype, False)
    route = ops.scene_head_route(x, K)
    assert route == expected_route(shape, dtype, offset)
    if offset and aligned == VECTOR:
        assert route == ELEMENT                                 # the offset pointer flips the route
    logits, pooled = ops.scene_head(x, weight, bias)
    assert logits.dtype == dtype and pooled.dtype == F32
    assert R.same_bits(logits, c['logits']) and R.same_bits(pooled, c['pooled'])
    gx, gw, gb = ops.scene_head_backward(g, pooled, weight, x.shape, dtype)
    assert gx.dtype == dtype and gx.shape == x.shape and gw.dtype == F32 and gb.dtype == F32
    assert R.same_bits(gx, c['gx']) and R.same_bits(gw, c['gw']) and R.same_bits(gb, c['gb'])
    # two calls give the same bits; the inference call gives the same logits
    logits2, pooled2 = ops.scene_head(x, weight, bias)
    gx2, gw2, gb2 = ops.scene_head_backward(g, pooled2, weight, x.shape, dtype)
    logits3, none = ops.scene_head(x, weight, bias, need_pooled=False)
    assert none is None
    for a, b in ((logits2, logits), (pooled2, pooled), (logits3, logits), (gx2, gx), (gw2, gw), (gb2, gb)):
        assert R.same_bits(a, b)
    # gradients that are not wanted leave the others unchanged
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        got = ops.scene_head_backward(g, pooled, weight, x.shape, dtype, need=need)
        for wanted, t, full in zip(need, got, (gx, gw, gb)):
            assert (t is None) if not wanted else R.same_bits(t, full), need
    assert ops.scene_head_backward(g, pooled, weight, x.shape, dtype, need=(False, False, False)) == (None,) * 3


def test_all_routes_are_taken_by_the_shapes():
    taken = {(d, expected_route(s, d, False)) for s in SHAPES for d in DTYPES}
    assert taken == {(d, r) for d in DTYPES for r in (UNIT, VECTOR, ELEMENT)}


@pytest.mark.parametrize('out_dtype', DTYPES, ids=str)
def test_output_dtype_and_missing_bias(out_dtype):
    shape = (2, 66, 7, 37, 45)
    c = case(shape, F32)
    x, weight = c['x'].to(DEV), c['weight'].to(DEV)
    logits, pooled = ops.scene_head(x, weight, None, out_dtype=out_dtype)
    want, _ = R.forward(c['x'], c['weight'], None, out_dtype=out_dtype)
    assert logits.dtype == out_dtype and R.same_bits(logits, want)
    # g in one dtype, gx in another
    g = c['g'].to(out_dtype)
    gx, gw, gb = ops.scene_head_backward(g.to(DEV), pooled, weight, x.shape, BF16)
    wx, ww, wb = R.backward(g, c['pooled'], c['weight'], x.shape, BF16)
    assert R.same_bits(gx, wx) and R.same_bits(gw, ww) and R.same_bits(gb, wb)


@pytest.mark.parametrize('value', (float('nan'), float('inf'), float('-inf')), ids=str)
@pytest.mark.parametrize('shape', ((3, 8, 1, 1, 45), (2, 5, 3, 5, 3), (2, 64, 2, 4, 10)), ids=str)
def test_nonfinite_values_stay_in_their_row_and_columns(shape, value):
    c = case(shape, F32)
    B, C, H, W, K = shape
    b0, c0 = B - 1, C // 2
    x = c['x'].clone()
    x[b0, c0, H - 1, W // 2] = value
    xd, weight, bias, g = x.to(DEV), c['weight'].to(DEV), c['bias'].to(DEV), c['g'].to(DEV)
    logits, pooled = ops.scene_head(xd, weight, bias)
    finite = torch.isfinite(logits).cpu()
    assert not bool(finite[b0].any()) and bool(finite[torch.arange(B) != b0].all())
    rows = torch.arange(B) != b0
    assert R.same_bits(logits.cpu()[rows], c['logits'][rows])
    gx, gw, gb = ops.scene_head_backward(g, pooled, weight, x.shape, F32)
    finite = torch.isfinite(gw).cpu()
    assert not bool(finite[:, c0].any()) and bool(finite[:, torch.arange(C) != c0].all())
    cols = torch.arange(C) != c0
    assert R.same_bits(gw.cpu()[:, cols].contiguous(), c['gw'][:, cols].contiguous())
    # gx and gbias do not depend on x
    assert R.same_bits(gx, c['gx']) and R.same_bits(gb, c['gb'])


def test_autograd_gives_the_ops_gradients_and_saves_pooled_only():
    shape = (2, 66, 7, 37, 45)
    c = case(shape, BF16)
    x = c['x'].to(DEV).requires_grad_(True)
    weight = c['weight'].to(DEV).requires_grad_(True)
    bias = c['bias'].to(DEV).requires_grad_(True)
    out = model.SceneHeadFunction.apply(x, weight, bias, BF16, True)
    saved = out.grad_fn.saved_tensors
    assert len(saved) == 2 and tuple(saved[0].shape) == shape[:2] and saved[0].dtype == F32
    assert saved[1].data_ptr() == weight.data_ptr()
    assert R.same_bits(saved[0], c['pooled'])
    out.backward(c['g'].to(DEV))
    assert R.same_bits(out.detach(), c['logits'])
    assert R.same_bits(x.grad, c['gx']) and R.same_bits(weight.grad, c['gw']) and R.same_bits(bias.grad, c['gb'])
    # a frozen head: only gx is asked for
    asked = []
    real = ops.scene_head_backward
    x2 = c['x'].to(DEV).requires_grad_(True)
    out = model.SceneHeadFunction.apply(x2, weight.detach(), bias.detach(), BF16, True)
    try:
        ops.scene_head_backward = lambda *a, **k: asked.append(k['need']) or real(*a, **k)
        out.backward(c['g'].to(DEV))
    finally:
        ops.scene_head_backward = real
    assert asked == [(True, False, False)] and R.same_bits(x2.grad, c['gx'])


def _decoder(c, shape):
    m = model.SceneClassificationDecoder(n_channels_in=shape[1], n_classes=shape[4])
    m.load_state_dict({'_task_head.weight': c['weight'], '_task_head.bias': c['bias']}, strict=True)
    return m.to(DEV)


@pytest.fixture
def calls(monkeypatch):
    """the `need_pooled` of every ops.scene_head call"""
    seen = []
    real = ops.scene_head

    def scene_head(x, weight, bias, need_pooled=True, out_dtype=None):
        seen.append(need_pooled)
        return real(x, weight, bias, need_pooled=need_pooled, out_dtype=out_dtype)
    monkeypatch.setattr(ops, 'scene_head', scene_head)
    return seen


@pytest.mark.parametrize('with_features', (True, False))
@pytest.mark.parametrize('train', (True, False))
def test_module_train_eval_and_no_grad(calls, train, with_features):
    shape = (2, 64, 2, 4, 10)
    c = case(shape, F32)
    m = _decoder(c, shape).train(train)
    x = c['x'].to(DEV).requires_grad_(True)
    other = torch.full((2, 7, 3, 3), float('nan'), device=DEV)          # never read
    inp = (other, (x, other)) if with_features else (x, ())
    assert m.takes_hip_path(x)
    out, side = m(inp, None, {}, do_postprocessing=False)
    assert side is None and calls == [True] and type(out.grad_fn).__name__ == 'SceneHeadFunctionBackward'
    out.backward(c['g'].to(DEV))
    assert R.same_bits(out.detach(), c['logits']) and R.same_bits(x.grad, c['gx'])
    assert R.same_bits(m._task_head.weight.grad, c['gw']) and R.same_bits(m._task_head.bias.grad, c['gb'])
    with torch.no_grad():
        out2, _ = m(inp, None, {}, do_postprocessing=False)
    assert calls == [True, False] and not out2.requires_grad and R.same_bits(out2, c['logits'])
    # nothing needs a gradient: no pooled vector either
    for p in m.parameters():
        p.requires_grad_(False)
    out3, _ = m((x.detach(), ()), None, {}, do_postprocessing=False)
    assert calls == [True, False, False] and R.same_bits(out3, c['logits'])
    # with the default postprocessing the raw logits are handed on
    post = m((x.detach(), ()), None, {}, do_postprocessing=True)
    assert R.same_bits(post['scene_output'], c['logits'])


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_module_under_autocast_and_with_a_half_cast_weight(calls, dtype):
    shape = (1, 130, 4, 5, 17)
    c = case(shape, dtype)
    m = _decoder(c, shape)
    x = c['x'].to(DEV)
    # outside autocast: x's dtype; inside: the autocast dtype, whatever x's dtype
    out, _ = m((x, ()), None, {}, do_postprocessing=False)
    assert out.dtype == dtype and R.same_bits(out.detach(), c['logits'])
    for auto in (BF16, F16):
        with torch.autocast('cuda', dtype=auto):
            out, _ = m((x, ()), None, {}, do_postprocessing=False)
        want, _ = R.forward(c['x'], c['weight'], c['bias'], out_dtype=auto)
        assert out.dtype == auto and R.same_bits(out.detach(), want)
    # module.half(): the half weights are cast to float32 on the host side
    if dtype != F32:
        m = m.to(dtype)
        out, _ = m((x, ()), None, {}, do_postprocessing=False)
        want, _ = R.forward(c['x'], c['weight'].to(dtype).float(), c['bias'].to(dtype).float())
        assert out.dtype == dtype and R.same_bits(out.detach(), want)
    assert all(calls) and len(calls) == (4 if dtype != F32 else 3)


def test_every_fallback_input_takes_torch(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError('the HIP path was taken')
    C, K = 6, 4
    m = model.SceneClassificationDecoder(C, K).to(DEV)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn((2, C, 4, 4), generator=gen).to(DEV)
    assert m.takes_hip_path(x)
    many_c = L.NMSA_SCENE_HEAD_MAX_CHANNELS + 1
    cases = {
        'float64': (m, x.double()),
        'empty': (m, x[:0]),
        'non-dense': (m, x[:, :, :, ::2]),
        'channels-last': (m, x.contiguous(memory_format=torch.channels_last)),
        'cpu': (model.SceneClassificationDecoder(C, K), x.cpu()),
        'too many channels': (model.SceneClassificationDecoder(many_c, K).to(DEV),
                              torch.randn((1, many_c, 1, 1), generator=gen).to(DEV)),
        'too many classes': (model.SceneClassificationDecoder(C, L.NMSA_SCENE_MAX_CLASSES + 1).to(DEV), x),
    }
    # the measured crossover: a map on the element route above FUSED_MAX_ELEMENT_ROUTE_IMAGE elements per image
    # takes torch; the same size on the vector route, and the element route up to the constant, stay on HIP
    limit = scene_module.FUSED_MAX_ELEMENT_ROUTE_IMAGE
    assert limit == 131072
    wide = model.SceneClassificationDecoder(2048, K).to(DEV)
    large = torch.randn((1, 2048, 5, 13), generator=gen).to(DEV)                # 65 elements per plane
    assert large[0].numel() > limit and ops.scene_head_route(large, K) == ELEMENT
    cases['large element-route map'] = (wide, large)
    assert wide.takes_hip_path(torch.zeros((1, 2048, 8, 9), device=DEV))        # 147456 elements, vector route
    assert wide.takes_hip_path(torch.zeros((2, 2048, 7, 9), device=DEV))        # 129024 elements, element route
    assert not wide.takes_hip_path(shifted(torch.zeros((1, 2048, 8, 9), device=DEV)))
    monkeypatch.setattr(ops, 'scene_head', refuse)
    monkeypatch.setattr(scene_module.SceneHeadFunction, 'apply', refuse)
    for what, (mod, t) in cases.items():
        assert not mod.takes_hip_path(t), what
        if t.dtype == torch.float64:
            mod = model.SceneClassificationDecoder(C, K).to(DEV).double()
        out, side = mod((t, ()), None, {}, do_postprocessing=False)
        want = R.torch_composition(t, mod._task_head.weight, mod._task_head.bias)
        assert side is None and out.shape == want.shape and torch.equal(out, want), what
