"""GPU tier of the MLP decoders (csrc/mlp_decoder.hip, ops.mlpdec_*, model.decoder).

Oracle: the two operations written out in float64 on the CPU from the same, already dtype-rounded
inputs (`testing.mlp_decoder_ref.reference64`), the error bounds of `testing.mlp_decoder_ref.bounds`
(tests/test_mlp_decoder_host.py holds torch's own float32 to them and two defective restatements out
of them), and the recorded results of the reference's decoders in tests/golden/mlp_decoder.npz.

Launch geometry the shapes are picked from (csrc/mlp_decoder.hip).  Forward: the output is a flat
stream; a work item is 256 lanes x VEC consecutive pixels of ONE output plane, VEC = 4 (float32) / 8
(half) on the vector route (W % VEC == 0, every tensor on 16 bytes) and 1 on the element route, so an
item is 1024 / 2048 / 256 pixels.  Backward: a lane owns a source pixel; an item is 256 consecutive
source pixels of one branch's flat [B * c * h * w] array and may span planes.  So: B = 2 (a plane must
not run into the next image), output planes of 8x16 = 128 and 6x8 = 48 pixels (smaller than one
item on every route), 40x48 = 1920 (ends inside the second float32 vector item, inside the first
half one), 48x64 = 3072 (ends inside the second half vector item and the third float32 one); source
planes from 1x1 (factor 16) and 5x6 (eight planes and a part per backward item) to 24x32 (three
items per plane); channel counts (3, 2, 1, 5) and (64, 3) (the plane -> branch search crosses every
boundary); W = 6 and W = 5 (element route only)."""
import pytest
import torch

from nicr_mt_scene_analysis_amd import _lib as L
from nicr_mt_scene_analysis_amd import model
from nicr_mt_scene_analysis_amd import ops
from nicr_mt_scene_analysis_amd.model import decoder as D
from nicr_mt_scene_analysis_amd.model.decoder import mlp_base
from nicr_mt_scene_analysis_amd.testing import mlp_decoder_cases as mc
from nicr_mt_scene_analysis_amd.testing import mlp_decoder_ref as R

import _golden

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = (F32, BF16, F16)
MODES = ('nearest', 'bilinear')
VECTOR, ELEMENT = L.NMSA_MLPDEC_ROUTE_VECTOR, L.NMSA_MLPDEC_ROUTE_ELEMENT
POISON = 12288.0                            # exact in bfloat16 and float16
B = mc.GPU_B


# ------------------------------------------------------------------------------ helpers
def off_by_one(t):
    """the same values on the device, one element into a larger buffer: off 16 bytes, on the element"""
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=DEV)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def run_ops(ys, g_out, mode, hw, shift=(), need=None):
    """both kernels on the device -> dict like reference64's; `shift`: indices of the tensors (branches
    0.., g_out = -1) that are placed one element into a larger buffer"""
    ysd = tuple(off_by_one(y.to(DEV)) if i in shift else y.to(DEV) for i, y in enumerate(ys))
    gd = off_by_one(g_out.to(DEV)) if -1 in shift else g_out.to(DEV)
    return {'cat': ops.mlpdec_upsample_concat(ysd, mode, size=hw),
            'gys': ops.mlpdec_upsample_concat_backward(gd, [tuple(y.shape) for y in ys], mode, need)}


def pairs(got, ref):
    yield 'cat', got['cat'], ref['cat']
    for i, (g, r) in enumerate(zip(got['gys'], ref['gys'])):
        yield f'gys{i}', g, r


def check_bounds(channels, factors, hw, dtype, mode, seed, shift=()):
    ys, g_out = R.make_inputs(B, channels, factors, hw, seed, dtype=dtype)
    ref = R.reference64(ys, mode, g_out, size=hw)
    bd = R.bounds(ys, mode, g_out, dtype=dtype, size=hw)
    got = run_ops(ys, g_out, mode, hw, shift)
    worst = {}
    for (key, g, r), (_, _, b) in zip(pairs(got, ref), pairs(got, bd)):
        assert g.dtype == dtype and tuple(g.shape) == tuple(r.shape), key
        worst[key] = R.worst_ratio(g, r, b)
    print('bounds', channels, factors, hw, dtype, mode, shift, {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, (channels, factors, hw, dtype, mode, worst)
    return got


# ------------------------------------------------------------------------------ exact tier
@pytest.mark.parametrize('hw', mc.EXACT_HW)
def test_exact_on_integer_inputs(hw):
    """integers in -8..8, factors (8, 4, 2, 1): every weight is a multiple of 1/32 and every sum is
    exact in float32 in any order (torch's own float32 is held to the same on the CPU by
    tests/test_mlp_decoder_host.py), so both kernels must give the float64 value, cast once"""
    for dtype in DTYPES:
        for mode in MODES:
            ys, g_out = R.make_inputs(B, mc.EXACT_CHANNELS, mc.EXACT_FACTORS, hw, 0, dtype=dtype, integer=True)
            ref = R.reference64(ys, mode, g_out, size=hw)
            got = run_ops(ys, g_out, mode, hw)
            for key, g, r in pairs(got, ref):
                assert g.dtype == dtype, key
                assert torch.equal(g.cpu(), r.to(dtype)), (key, hw, dtype, mode)


# ------------------------------------------------------------------------------ bounds tier
@pytest.mark.parametrize('channels,factors,sizes', mc.BOUNDS_CASES)
def test_bounds_on_normal_inputs(channels, factors, sizes):
    seed = 100 + sum(len(c[2]) for c in mc.BOUNDS_CASES[:mc.BOUNDS_CASES.index((channels, factors, sizes))])
    for hw in sizes:
        seed += 1
        for dtype in DTYPES:
            for mode in MODES:
                ys, _ = R.make_inputs(B, channels, factors, hw, seed, dtype=dtype)
                want = VECTOR if hw[1] % (4 if dtype == F32 else 8) == 0 else ELEMENT
                yd = tuple(y.to(DEV) for y in ys)
                assert ops.mlpdec_route(yd, torch.empty((B, sum(channels)) + hw, dtype=dtype, device=DEV)) == want
                got = check_bounds(channels, factors, hw, dtype, mode, seed)
                # a branch that already has the output size is copied
                for i, f in enumerate(factors):
                    if f == 1:
                        c0 = sum(channels[:i])
                        assert torch.equal(got['cat'][:, c0:c0 + channels[i]].cpu(), ys[i])


# ------------------------------------------------------------------------------ element route
@pytest.mark.parametrize('channels,factors,hw', mc.ELEMENT_CASES)
def test_element_route_on_widths_off_the_vector(channels, factors, hw):
    seed = 100 + sum(len(c[2]) for c in mc.BOUNDS_CASES) + 1 + mc.ELEMENT_CASES.index((channels, factors, hw))
    for dtype in DTYPES:
        ys, _ = R.make_inputs(B, channels, factors, hw, seed, dtype=dtype)
        out = torch.empty((B, sum(channels)) + hw, dtype=dtype, device=DEV)
        assert ops.mlpdec_route(tuple(y.to(DEV) for y in ys), out) == ELEMENT
        for mode in MODES:
            a = check_bounds(channels, factors, hw, dtype, mode, seed)
            # every tensor one element into a larger buffer: no alignment rule beyond the element
            b = check_bounds(channels, factors, hw, dtype, mode, seed, shift=(-1,) + tuple(range(len(channels))))
            for (key, ta, _), (_, tb, _) in zip(pairs(a, a), pairs(b, b)):
                assert torch.equal(ta, tb), key


def test_element_route_gives_the_bits_of_the_vector_route():
    """aligned shapes, the element route forced by shifting ONE tensor off 16 bytes"""
    channels, factors, hw = (3, 2, 1, 5), (8, 4, 2, 1), (40, 48)
    for dtype in DTYPES:
        for mode in MODES:
            ys, g_out = R.make_inputs(B, channels, factors, hw, 21, dtype=dtype)
            yd = tuple(y.to(DEV) for y in ys)
            out = torch.empty((B, sum(channels)) + hw, dtype=dtype, device=DEV)
            assert ops.mlpdec_route(yd, out) == VECTOR
            a = run_ops(ys, g_out, mode, hw)
            for k in (0, 3):
                moved = tuple(off_by_one(y) if i == k else y for i, y in enumerate(yd))
                assert ops.mlpdec_route(moved, out) == ELEMENT
                assert torch.equal(ops.mlpdec_upsample_concat(moved, mode), a['cat']), (dtype, mode, k)
            b = run_ops(ys, g_out, mode, hw, shift=(-1,))
            for ga, gb in zip(a['gys'], b['gys']):
                assert torch.equal(ga, gb)


# ------------------------------------------------------------------------------ subsets
def test_unwanted_gradients_come_back_none_and_nothing_else_is_skipped():
    channels, factors, hw = (3, 2, 1, 5), (8, 4, 2, 1), (16, 24)
    ys, g_out = R.make_inputs(B, channels, factors, hw, 3)
    shapes = [tuple(y.shape) for y in ys]
    gd = g_out.to(DEV)
    real_empty = torch.empty

    def poisoned(*args, **kwargs):
        return real_empty(*args, **kwargs).fill_(POISON)

    full = ops.mlpdec_upsample_concat_backward(gd, shapes, 'bilinear')
    for need in ((True, False, True, False), (False, True, False, True), (False, False, True, False)):
        torch.empty = poisoned                  # an element the kernel does not write shows
        try:
            part = ops.mlpdec_upsample_concat_backward(gd, shapes, 'bilinear', need=need)
            cat = ops.mlpdec_upsample_concat(tuple(y.to(DEV) for y in ys), 'bilinear')
        finally:
            torch.empty = real_empty
        for n, p, f in zip(need, part, full):
            assert (p is None) == (not n)
            if n:
                assert torch.equal(p, f)
        assert not bool((cat == POISON).any())
    assert ops.mlpdec_upsample_concat_backward(gd, shapes, 'bilinear', need=(False,) * 4) == (None,) * 4
    ref = R.upcat_backward64(g_out, shapes, 'bilinear')
    bd = R.bounds(ys, 'bilinear', g_out)['gys']
    assert max(R.worst_ratio(g, r, b) for g, r, b in zip(full, ref, bd)) <= 1.0
    # the factor-1 gradient is the view of g_out
    assert full[3].data_ptr() == gd[:, 6:].data_ptr() and torch.equal(full[3], gd[:, 6:])


def test_argument_checks_on_the_device():
    y = torch.zeros(2, 3, 4, 8, device=DEV)
    with pytest.raises(TypeError):
        ops.mlpdec_upsample_concat((y.double(),), 'nearest')
    with pytest.raises(TypeError):
        ops.mlpdec_upsample_concat((y, y.half()), 'nearest')            # one dtype per call
    with pytest.raises(TypeError):
        ops.mlpdec_upsample_concat((y, y[:1]), 'nearest')
    with pytest.raises(ValueError):
        ops.mlpdec_upsample_concat((y,) * 5, 'nearest')
    with pytest.raises(ValueError):
        ops.mlpdec_upsample_concat((y,), 'bicubic')
    with pytest.raises(TypeError):
        ops.mlpdec_upsample_concat_backward(torch.zeros(2, 7, 4, 8, device=DEV), ((2, 3, 4, 8),), 'nearest')
    # a permuted branch is made contiguous
    ys, _ = R.make_inputs(B, (3, 2), (2, 1), (8, 8), 1)
    yd = tuple(t.to(DEV) for t in ys)
    yt = yd[0].permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not yt.is_contiguous()
    assert torch.equal(ops.mlpdec_upsample_concat((yt, yd[1]), 'bilinear'), ops.mlpdec_upsample_concat(yd, 'bilinear'))


# ------------------------------------------------------------------------------ the fixture
@pytest.fixture(scope='module')
def golden():
    return _golden.load('mlp_decoder')


CASES = list(mc.MLP_DECODER_CASES)


def build(case, train=False):
    module = mc.build_decoder(D, model.get_encoder_decoder_fusion_class, model.get_upsampling_class, case)
    inp = mc.make_decoder_inputs(case, mc.state_shapes(module), mc.output_shapes(case))
    mc.load_state(module, inp['state'])
    return (module.train() if train else module.eval()).to(DEV), inp


@pytest.mark.parametrize('case', CASES)
def test_kernels_against_the_recorded_intermediates(golden, case):
    """float32 kernels on the recorded branch maps and the recorded gradient of the concatenation:
    within TWICE the bounds of the recorded float32 results (both sides are float32 evaluations within
    one bound of the truth)"""
    c = mc.MLP_DECODER_CASES[case]
    n = len(c['n_channels'])
    embs = tuple(torch.from_numpy(golden[f'{case}__emb{i}']) for i in range(n))
    g_cat = torch.from_numpy(golden[f'{case}__gcat'])
    got = run_ops(embs, g_cat, c['mode'], tuple(g_cat.shape[2:]))
    bd = R.bounds(embs, c['mode'], g_cat)
    worst = {'cat': R.worst_ratio(got['cat'], torch.from_numpy(golden[f'{case}__cat']).double(), 2 * bd['cat'])}
    for i in range(n):
        worst[f'gemb{i}'] = R.worst_ratio(got['gys'][i], torch.from_numpy(golden[f'{case}__gemb{i}']).double(),
                                          2 * bd['gys'][i])
    print('fixture', case, {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, (case, worst)


def run_module(module, inp, fused):
    """outputs and input gradients of the decoder; `fused` False: the torch composition with the same
    parameters on the same device"""
    x = torch.from_numpy(inp['x']).to(DEV).requires_grad_(True)
    skips = mc.skips_to(inp, DEV, requires_grad=True)
    real = mlp_base._fused_mode
    if not fused:
        mlp_base._fused_mode = lambda *a: None
    try:
        outs, side = module((x, ()), skips, {}, do_postprocessing=False)
    finally:
        mlp_base._fused_mode = real
    assert side == ()
    outs = outs if isinstance(outs, tuple) else (outs,)
    torch.autograd.backward(outs, [torch.from_numpy(g).to(DEV) for g in inp['gys']])
    res = {f'out{k}': o.detach().cpu() for k, o in enumerate(outs)}
    res['gx'] = x.grad.cpu()
    for d, s in skips.items():
        res[f'gskip{d}'] = s['rgb'].grad.cpu()
    return res


@pytest.mark.parametrize('case', CASES)
def test_module_against_the_fixture_end_to_end(golden, case):
    """eval mode, float32: the decoder's worst error against every recorded output and gradient must not
    exceed twice that of the torch-composition twin with the same parameters on the same device (two
    float32 evaluations of one formula); where the twin's error is 0 the decoder's must be 0"""
    module, inp = build(case)
    errs = {}
    for who, fused in (('module', True), ('twin', False)):
        res = run_module(module, inp, fused)
        errs[who] = {k: float((v - torch.from_numpy(golden[f'{case}__{k}'])).abs().max()) for k, v in res.items()}
    print('end-to-end', case, errs)
    assert set(errs['module']) >= {'out0', 'gx'}
    for key in errs['module']:
        assert errs['module'][key] <= 2 * errs['twin'][key], (case, key, errs)


# ------------------------------------------------------------------------------ wiring
def count_calls(monkeypatch):
    calls = []
    real = ops.mlpdec_upsample_concat
    monkeypatch.setattr(ops, 'mlpdec_upsample_concat', lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


@pytest.mark.parametrize('case', ('sem_swin_bilinear_4', 'normal_swin_nearest_2', 'ins_select_bilinear_3'))
def test_the_fused_step_is_taken_when_its_conditions_hold(monkeypatch, case):
    calls = count_calls(monkeypatch)
    module, inp = build(case)
    run_module(module, inp, fused=True)
    assert len(calls) == 1
    run_module(module, inp, fused=False)
    assert len(calls) == 1


def test_the_composition_is_taken_for_a_learned_mode_and_an_odd_factor(monkeypatch):
    calls = count_calls(monkeypatch)
    # both branches at factor 2 (the learned upsampling's only factor): 3x5 maps, a 6x10 grid
    case = dict(mc.MLP_DECODER_CASES['emb_select_bilinear_2'], mode='learned-3x3', skip_downs=(8,))
    module = mc.build_decoder(D, model.get_encoder_decoder_fusion_class, model.get_upsampling_class, case)
    inp = mc.make_decoder_inputs(case, mc.state_shapes(module), mc.output_shapes(case))
    mc.load_state(module, inp['state'])
    out, _ = module.to(DEV).eval()((torch.from_numpy(inp['x']).to(DEV), ()), mc.skips_to(inp, DEV), {},
                                  do_postprocessing=False)
    assert tuple(out.shape) == (2, 4, 12, 20) and not calls
    # an odd factor: 3
    up = model.get_upsampling_class('nearest')
    ups = [up(n_channels=2, scale_factor=3), up(n_channels=2, scale_factor=1)]
    ys = [torch.randn(2, 2, 2, 3, device=DEV), torch.randn(2, 2, 6, 9, device=DEV)]
    assert mlp_base._fused_mode(ups, ys) is None
    assert tuple(mlp_base.upsample_concat(ups, ys).shape) == (2, 4, 6, 9) and not calls
    # a fifth branch
    ups = [up(n_channels=2, scale_factor=1) for _ in range(5)]
    assert mlp_base._fused_mode(ups, [ys[1]] * 5) is None
    # and the fused step where everything holds
    ups = [up(n_channels=2, scale_factor=2), up(n_channels=2, scale_factor=1)]
    ys = [torch.randn(2, 2, 3, 4, device=DEV), torch.randn(2, 2, 6, 8, device=DEV)]
    assert mlp_base._fused_mode(ups, ys) == 'nearest'
    assert torch.equal(mlp_base.upsample_concat(ups, ys), torch.cat([u(y) for u, y in zip(ups, ys)], 1))
    assert len(calls) == 1


def test_train_mode_runs_and_every_parameter_gets_a_gradient(golden):
    module, inp = build(mc.MLP_DECODER_TRAIN_CASE, train=True)
    x = torch.from_numpy(inp['x']).to(DEV).requires_grad_(True)
    out, side = module((x, ()), mc.skips_to(inp, DEV), {}, do_postprocessing=False)
    assert side == () and [list(out.shape)] == _golden.jload(golden['train'])['out']
    out.backward(torch.from_numpy(inp['gys'][0]).to(DEV))
    assert x.grad.shape == x.shape and bool(torch.isfinite(x.grad).all())
    assert all(q.grad is not None for q in module.parameters())


@pytest.mark.parametrize('cast', (BF16,))
def test_autocast_keeps_the_reference_dtype(monkeypatch, cast):
    calls = count_calls(monkeypatch)
    module, inp = build('sem_select_nearest_3')
    res, cats = {}, {}
    real = mlp_base._fused_mode
    for fused in (True, False):
        hook = module.fuse.register_forward_pre_hook(lambda _, args, fused=fused: cats.__setitem__(fused, args[0]))
        if not fused:
            monkeypatch.setattr(mlp_base, '_fused_mode', lambda *a: None)
        with torch.autocast('cuda', dtype=cast):
            res[fused], _ = module((torch.from_numpy(inp['x']).to(DEV), ()), mc.skips_to(inp, DEV), {},
                                   do_postprocessing=False)
        monkeypatch.setattr(mlp_base, '_fused_mode', real)
        hook.remove()
    assert len(calls) == 1
    # the concatenation has the dtype torch's own resize gives under autocast (float32 or the half
    # dtype, depending on the build's autocast policy), and so has the output
    assert res[True].dtype == res[False].dtype and cats[True].dtype == cats[False].dtype
    # nearest: the concatenation is a copy of the half branch maps on both paths
    assert torch.equal(cats[True], cats[False])


def test_a_reference_shaped_state_dict_loads_strictly(golden):
    recorded = _golden.jload(golden['state'])
    for name, kwargs in mc.MLP_DECODER_STATE_KWARGS.items():
        case = dict(mc.MLP_DECODER_STATE_PROBE, decoder=name, mode='bilinear', kwargs=kwargs)
        m = mc.build_decoder(D, model.get_encoder_decoder_fusion_class, model.get_upsampling_class, case).to(DEV)
        state = {k: torch.full(s, 0.5) for k, s in recorded[name].items() if not k.endswith('num_batches_tracked')}
        state.update({k: v for k, v in m.state_dict().items() if k.endswith('num_batches_tracked')})
        m.load_state_dict(state, strict=True)
        assert float(m.fuse.conv.weight.sum()) == 0.5 * m.fuse.conv.weight.numel()


# ------------------------------------------------------------------------------ determinism
def test_same_bits_on_every_call_stream_and_graph_replay():
    channels, factors, hw = (3, 2, 1, 5), (8, 4, 2, 1), (40, 48)
    shapes = None
    for dtype in (F32, BF16):
        ys, g_out = R.make_inputs(B, channels, factors, hw, 9, dtype=dtype)
        yd, gd = tuple(y.to(DEV) for y in ys), g_out.to(DEV)
        shapes = [tuple(y.shape) for y in ys]

        def call():
            return (ops.mlpdec_upsample_concat(yd, 'bilinear'),) + \
                ops.mlpdec_upsample_concat_backward(gd, shapes, 'bilinear')[:3]

        first = call()
        torch.cuda.synchronize()
        for a, b in zip(first, call()):
            assert torch.equal(a, b)
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            on_side = call()
        side.synchronize()
        for a, b in zip(first, on_side):
            assert torch.equal(a, b)
        graph = torch.cuda.CUDAGraph()
        warm = torch.cuda.Stream(DEV)
        warm.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(warm):
            call()
        torch.cuda.current_stream(DEV).wait_stream(warm)
        with torch.cuda.graph(graph):
            captured = call()
        for t in captured:
            t.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(first, captured):
            assert torch.equal(a, b)
