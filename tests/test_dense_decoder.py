"""GPU tier of the convolutional dense decoders (model/decoder/dense_base.py and the three decoders over it).

The node: `UpsampleAddFunction`'s gradients against float64 autograd of the composition, inside the bounds the
backward kernels it calls are held to (`upsampling_ref.bounds`, `mlp_decoder_ref.bounds`); the gradient of the skip is
the upstream gradient's storage.

The decoders: every case of tests/golden/dense_decoder.npz (the reference's own decoders, float64 on the CPU) run
twice on the device in float32, fused and with `dense_base._fused_mode` replaced by one that answers None (torch's
own composition on the same device: not code under test).  With d = the largest, over the outputs, side outputs and
input gradients, of max|got - record| / max|record|, the rule is d_fused <= 2 d_plain + r, r = 2^-24 (half an ulp of
float32, relative): the fused step changes one rounding per step and nothing else.  Both distances are printed; the
ones measured on an MI355X are in docs/measurement_log.md.  The cases are tiny (main map 1x2) because the fixture
records every tensor; the kernel's own geometry is the business of tests/test_up_add.py."""
import collections

import numpy as np
import pytest
import torch

from nicr_mt_scene_analysis_amd import model
from nicr_mt_scene_analysis_amd import ops
from nicr_mt_scene_analysis_amd.model import decoder as D
from nicr_mt_scene_analysis_amd.model.decoder import dense_base
from nicr_mt_scene_analysis_amd.testing import dense_decoder_cases as dc
from nicr_mt_scene_analysis_amd.testing import mlp_decoder_ref as MR
from nicr_mt_scene_analysis_amd.testing import network_cases as NC
from nicr_mt_scene_analysis_amd.testing import up_add_ref as R
from nicr_mt_scene_analysis_amd.testing import upsampling_ref as UR

import _golden

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
U = 2.0 ** -24
NODE = 'UpsampleAddFunctionBackward'
CPU_CASES = [k for k, c in dc.DENSE_DECODER_CASES.items() if c['mode'] in ('nearest', 'bilinear')]


@pytest.fixture(scope='module')
def golden():
    return _golden.load('dense_decoder')


def build(case, device=DEV, dtype=torch.float32):
    """the decoder of a case with the case's state (loaded strictly), in the mode of the records, and its inputs"""
    module = dc.build_decoder(D, model.get_encoder_decoder_fusion_class, model.get_upsampling_class,
                              model.get_block_class, case)
    inp = dc.make_decoder_inputs(case, dc.state_shapes(module))
    state = {k: torch.from_numpy(v) for k, v in inp['state'].items()}
    state.update({k: v for k, v in module.state_dict().items() if k.endswith('num_batches_tracked')})
    module.load_state_dict(state, strict=True)              # the reference's keys: the host tier holds the table
    dc.record_mode(module)
    return module.to(device=device, dtype=dtype), inp


def run(module, inp, device=DEV, dtype=torch.float32, nodes=None):
    """forward and backward of a case -> {name: tensor} of the outputs, side outputs and input gradients"""
    module.zero_grad(set_to_none=True)
    x = torch.from_numpy(inp['x']).to(device=device, dtype=dtype).requires_grad_(True)
    skips = {d: {'rgb': s['rgb'].to(device=device, dtype=dtype).requires_grad_(True)}
             for d, s in dc.skips_to(inp).items()}
    outs, sides = module((x, ()), skips, {}, do_postprocessing=False)
    flat = dc.flat_outputs(outs, sides)
    if nodes is not None:
        nodes.update(NC.graph_node_counts(*flat))
    torch.autograd.backward(flat, dc.flat_gradients(inp, dtype, device))
    got = {f'out{k}': o.detach() for k, o in enumerate(flat)}
    got['gx'] = x.grad
    got.update({f'gskip{d}': s['rgb'].grad for d, s in skips.items()})
    return got


def distance(got, golden, case):
    """the largest max|got - record| / max|record| over the recorded float64 quantities, and where"""
    worst, where = 0.0, None
    for name, t in got.items():
        rec = golden[f'{case}__f64_{name}']
        d = float(np.abs(t.double().cpu().numpy() - rec).max() / np.abs(rec).max())
        if d >= worst:
            worst, where = d, name
    return worst, where


def plain(monkeypatch):
    monkeypatch.setattr(dense_base, '_fused_mode', lambda *args: None)


# ------------------------------------------------------------------------------ a. the node
@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('dtype', (torch.float32, torch.bfloat16))
@pytest.mark.parametrize('shape', ((2, 3, 9, 12), (2, 3, 17, 7)))
def test_node_gradients_against_float64_autograd_of_the_composition(shape, dtype, mode):
    x, skip, gy, wt, b = R.make_inputs(shape, dtype, seed=600 + sum(shape))
    learned = R.is_learned(mode)
    xd, sd, gyd = (t.to(DEV).requires_grad_(g) for t, g in ((x, True), (skip, True), (gy, False)))
    wd, bd = (wt.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)) if learned else (None, None)
    y = D.UpsampleAddFunction.apply(xd, sd, wd, bd, mode)
    assert type(y.grad_fn).__name__ == NODE
    saved = [t for t in (getattr(y.grad_fn, 'saved_tensors', ()) or ())]
    assert len(saved) == (2 if learned else 0)              # x and weight, or nothing map-sized
    y.backward(gyd)
    assert R.worst_ratio(y, R.reference64(x, skip, mode, wt, b), R.bounds(x, skip, mode, wt, b, dtype)) <= 1.0
    assert torch.equal(sd.grad, gyd)                        # d(u + skip) / d skip = 1
    if learned:
        zeropad = mode.endswith('zeropad')
        _, gx64, gw64, gb64 = UR.reference64(x, wt, b, gy, zeropad)
        bound = UR.bounds(x, wt, b, gy, zeropad, dtype)
        worst = {'gx': R.worst_ratio(xd.grad, gx64, bound['gx']), 'gw': R.worst_ratio(wd.grad, gw64, bound['gw']),
                 'gb': R.worst_ratio(bd.grad, gb64, bound['gb'])}
    else:
        size = (2 * shape[2], 2 * shape[3])
        gx64 = MR.reference64([x], mode, gy, size=size)['gys'][0]
        bound = MR.bounds([x], mode, gy, dtype=dtype, size=size)['gys'][0]
        worst = {'gx': R.worst_ratio(xd.grad, gx64, bound)}
    print(f'node {mode} {dtype} {shape}: worst error / bound', {k: round(v, 3) for k, v in worst.items()})
    assert xd.grad.dtype == dtype and max(worst.values()) <= 1.0


@pytest.mark.parametrize('mode', ('bilinear', 'learned-3x3'))
def test_the_gradient_of_the_skip_is_the_upstream_gradient_itself(mode, monkeypatch):
    x, skip, gy, wt, b = (t.to(DEV) for t in R.make_inputs((2, 3, 5, 8), torch.float32, seed=3))
    if not R.is_learned(mode):
        wt = b = None
    seen = {}
    xl = x.clone().requires_grad_(True)
    e = skip.clone().requires_grad_(True) * 1.0             # not a leaf: its gradient is handed on as it is
    y = D.UpsampleAddFunction.apply(xl, e, wt, b, mode)
    y.register_hook(lambda g: seen.__setitem__('gy', g))
    e.register_hook(lambda g: seen.__setitem__('ge', g))
    y.backward(gy)
    assert seen['ge'].data_ptr() == seen['gy'].data_ptr()
    assert seen['ge'].untyped_storage().data_ptr() == seen['gy'].untyped_storage().data_ptr()
    assert torch.equal(seen['ge'], gy)
    # only what needs a gradient is asked of the backward kernels
    asked = []
    name = 'upsample2x_dw3x3_backward' if R.is_learned(mode) else 'mlpdec_upsample_concat_backward'
    real = getattr(ops, name)
    monkeypatch.setattr(ops, name, lambda *a, **k: asked.append(a) or real(*a, **k))
    sl = skip.clone().requires_grad_(True)
    D.UpsampleAddFunction.apply(x, sl, wt, b, mode).backward(gy)
    assert asked == [] and torch.equal(sl.grad, gy)
    xl = x.clone().requires_grad_(True)
    D.UpsampleAddFunction.apply(xl, skip, wt, b, mode).backward(gy)
    assert len(asked) == 1 and xl.grad is not None
    if R.is_learned(mode):
        assert asked[0][4:] == (True, False, False)         # gx alone: no partial sums, no reduction


def test_two_backward_calls_give_identical_bytes():
    for mode, dtype, shape in (('bilinear', torch.float32, (4, 5, 33, 40)),
                               ('learned-3x3', torch.bfloat16, (3, 4, 17, 37)),
                               ('nearest', torch.float16, (2, 3, 9, 12)),
                               ('learned-3x3-zeropad', torch.float32, (2, 3, 9, 7))):
        x, skip, gy, wt, b = (t.to(DEV) for t in R.make_inputs(shape, dtype, seed=9))
        grads = []
        for _ in range(2):
            leaves = [x.clone().requires_grad_(True), skip.clone().requires_grad_(True)]
            if R.is_learned(mode):
                leaves += [wt.clone().requires_grad_(True), b.clone().requires_grad_(True)]
            args = leaves + [None] * (4 - len(leaves))
            D.UpsampleAddFunction.apply(*args, mode).backward(gy)
            grads.append([t.grad for t in leaves])
        for a, e in zip(*grads):
            assert torch.equal(a.view(torch.uint8), e.view(torch.uint8)), mode


# ------------------------------------------------------------------------------ b. the decoders
@pytest.mark.parametrize('case', list(dc.DENSE_DECODER_CASES))
def test_fused_against_plain_against_the_fixture(golden, case, monkeypatch):
    module, inp = build(case)
    nodes = collections.Counter()
    fused = run(module, inp, nodes=nodes)
    assert nodes[NODE] == len(dc.fused_steps(case)) > 0
    plain(monkeypatch)
    nodes = collections.Counter()
    unfused = run(module, inp, nodes=nodes)
    assert nodes[NODE] == 0
    d_fused, at_fused = distance(fused, golden, case)
    d_plain, at_plain = distance(unfused, golden, case)
    print(f'{case}: d_fused {d_fused:.3e} ({at_fused})  d_plain {d_plain:.3e} ({at_plain})')
    recorded = {k[len(f'{case}__f64_'):] for k in golden.files if k.startswith(f'{case}__f64_')}
    assert set(fused) == {n for n in recorded if n.startswith(('out', 'gx', 'gskip'))}     # every record is held
    assert d_fused <= 2 * d_plain + U
    if dc.DENSE_DECODER_CASES[case]['mode'] == 'nearest':   # one IEEE addition either way
        for k in fused:
            assert torch.equal(fused[k], unfused[k]), k


@pytest.mark.parametrize('case', list(dc.DENSE_DECODER_CASES))
def test_the_fused_step_against_the_recorded_triples(golden, case, monkeypatch):
    """every fused step of a case, with the operands the decoder hands it: the mode is the case's, an identity
    `layer` hands on the skip itself, the node's sum lies within the node's bound of the float64 sum of its own
    operands, and its distance to the RECORDED sum obeys the rule with torch's composition on the same operands"""
    module, inp = build(case)
    c = dc.DENSE_DECODER_CASES[case]
    real, calls = dense_base.UpsampleAddFunction, []

    class Spy:
        @staticmethod
        def apply(x, e, weight, bias, mode):
            calls.append((x.detach(), e.detach(), weight, bias, mode))
            return real.apply(x, e, weight, bias, mode)

    monkeypatch.setattr(dense_base, 'UpsampleAddFunction', Spy)
    run(module, inp)
    steps = dc.fused_steps(case)
    assert len(calls) == len(steps)
    for (i, j, down), (x, e, weight, bias, mode) in zip(steps, calls):
        assert mode == c['mode'] and (weight is not None) == R.is_learned(mode)
        if isinstance(module.fusions[j].layer, torch.nn.Identity):
            assert torch.equal(e.cpu(), torch.from_numpy(inp['skips'][str(down)]['rgb']))
        with torch.no_grad():
            got = real.apply(x, e, weight, bias, mode)
            composed = R.torch_up_add(x, e, mode, weight, bias)
        host = [None if t is None else t.detach().cpu() for t in (x, e, weight, bias)]
        assert R.worst_ratio(got, R.reference64(host[0], host[1], mode, host[2], host[3]),
                             R.bounds(host[0], host[1], mode, host[2], host[3])) <= 1.0
        rec = torch.from_numpy(golden[f'{case}__f64_s{i}'])
        d_fused, d_plain = (float((t.double().cpu() - rec).abs().max() / rec.abs().max()) for t in (got, composed))
        print(f'{case} step {i}: sum d_fused {d_fused:.3e}  d_plain {d_plain:.3e}')
        assert d_fused <= 2 * d_plain + U


@pytest.mark.parametrize('case', CPU_CASES)
def test_an_sgd_step_moves_the_parameters_like_the_plain_path(case, monkeypatch):
    """one step of torch.optim.SGD on sum_k sum(out_k * gy_k), fused and plain on the device, against the same step
    of the same decoder in float64 on the CPU (the composition; the learned modes have no CPU path): the rule of the
    module docstring over the parameters after the step"""
    lr = 0.1
    ref, inp = build(case, device='cpu', dtype=torch.float64)
    opt = torch.optim.SGD(ref.parameters(), lr=lr)
    run(ref, inp, device='cpu', dtype=torch.float64)
    opt.step()
    want = {k: p.detach() for k, p in ref.named_parameters()}
    dist = {}
    for name in ('fused', 'plain'):
        if name == 'plain':
            plain(monkeypatch)
        module, _ = build(case)
        before = {k: p.detach().clone() for k, p in module.named_parameters()}
        opt = torch.optim.SGD(module.parameters(), lr=lr)
        run(module, inp)
        opt.step()
        assert any(not torch.equal(p.detach(), before[k]) for k, p in module.named_parameters())
        dist[name] = max(float((p.detach().double().cpu() - want[k]).abs().max() / want[k].abs().max().clamp_min(1e-30))
                         for k, p in module.named_parameters())
    print(f"{case} after one SGD step: d_fused {dist['fused']:.3e}  d_plain {dist['plain']:.3e}")
    assert dist['fused'] <= 2 * dist['plain'] + U


def test_what_takes_the_composition_on_the_device():
    """autocast and channels-last skips run the composition: no fused node; eval mode keeps the fused node and gives
    None side outputs"""
    case = 'sem_nb1d_bilinear_3'
    module, inp = build(case)
    x = torch.from_numpy(inp['x']).to(DEV)

    def nodes_with(skips, autocast=False):
        with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
            outs, sides = module((x.clone().requires_grad_(True), ()), skips, {}, do_postprocessing=False)
        return NC.graph_node_counts(*(t for t in dc.flat_outputs(outs, sides) if t is not None)), sides

    skips = dc.skips_to(inp, DEV)
    assert nodes_with(skips)[0][NODE] == 3
    assert nodes_with(skips, autocast=True)[0][NODE] == 0
    cl = {d: {'rgb': s['rgb'].contiguous(memory_format=torch.channels_last)} for d, s in skips.items()}
    assert not any(s['rgb'].is_contiguous() for s in cl.values())
    # the first and the last skip reach the step as they are (identity `layer`); the 1x1 adapter of the second one
    # hands on whatever layout the convolution picks
    assert nodes_with(cl)[0][NODE] <= 1
    module.eval()
    counts, sides = nodes_with(skips)
    assert counts[NODE] == 3 and sides == (None, None, None)
