"""GPU tier of the residual blocks: the four `ops.bntail_*` kernels one by one and the blocks through autograd,
against the float64 restatement and the derived bounds of testing/block_ref.py (exact equality on
constructed inputs), the recorded reference blocks, both routes and off-16-byte tensors, determinism,
training state, dropout, gradient subsets, the fallbacks, autocast and graph replay."""
import itertools
import os

import pytest
import torch
from torch import nn

from nicr_mt_scene_analysis_amd import _lib as L
from nicr_mt_scene_analysis_amd import model
from nicr_mt_scene_analysis_amd import ops
from nicr_mt_scene_analysis_amd.model import block as block_module
from nicr_mt_scene_analysis_amd.testing import block_cases as BC
from nicr_mt_scene_analysis_amd.testing import block_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = (F32, BF16, F16)
VECTOR, ELEMENT = L.NMSA_BNTAIL_ROUTE_VECTOR, L.NMSA_BNTAIL_ROUTE_ELEMENT
POISON = -1024.0
EPS, MOM = 1e-5, 0.1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'block.npz')
OPS = ('bntail_stats', 'bntail_apply', 'bntail_backward_reduce', 'bntail_backward_apply')
COMBOS = tuple(itertools.product((False, True), (False, True), BC.ACTS))       # scale, identity, act


@pytest.fixture(autouse=True)
def fused_at_every_size(monkeypatch):
    """the tier's shapes are the smallest at which a kernel can go wrong, far below the size from which the
    modules take the fused path for speed (`block.FUSED_MIN_ELEMENTS`; a test of its own holds that rule)"""
    monkeypatch.setattr(block_module, 'FUSED_MIN_ELEMENTS', 0)


def dev(t):
    return None if t is None else t.to(DEV)


class Moved:
    """a tensor one element into a larger buffer (off 16 bytes), poison around it"""

    def __init__(self, like, fill=None):
        n = like.numel()
        self.buf = torch.full((n + 16,), POISON, dtype=like.dtype, device=DEV)
        self.t = self.buf[1:1 + n].view(like.shape)
        if fill is not None:
            self.t.copy_(fill)
        assert self.t.data_ptr() % 16 != 0 and self.t.is_contiguous()

    def untouched(self):
        n = self.t.numel()
        return bool((self.buf[:1] == POISON).all()) and bool((self.buf[1 + n:] == POISON).all())


_CASES = {}


def case(B, C, hw, dtype):
    key = (B, C, hw, dtype)
    if key not in _CASES:
        _CASES[key] = R.make_tail_inputs(B, C, hw, 500 + BC.SHAPES.index((B, C, hw)), dtype)
    return _CASES[key]


def check(got, ref, what, worst):
    r = R.worst_ratio(got, ref)
    worst[what] = max(worst.get(what, 0.0), r)
    assert r <= 1.0, (what, r)


def count_calls(monkeypatch):
    calls = []
    for name in OPS:
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _r=real, **k: calls.append(_n) or _r(*a, **k))
    return calls


# ------------------------------------------------------------------------------ routes
@pytest.mark.parametrize('dtype', DTYPES)
def test_routes_of_the_tier_shapes(dtype):
    for hw in BC.PLANES:
        x = torch.zeros((2, 5) + hw, dtype=dtype, device=DEV)
        assert ops.bntail_route(x, x, x) == BC.expected_route(dtype, hw), hw
        assert ops.bntail_route(x, Moved(x).t) == BC.expected_route(dtype, hw, aligned=False), hw
    assert BC.expected_route(BF16, (15, 20))[0] == ELEMENT and BC.expected_route(F32, (15, 20))[0] == VECTOR
    assert BC.expected_route(dtype, BC.SEG_HW) == (ELEMENT, 2) and BC.expected_route(dtype, (30, 40))[1] == 1


# ------------------------------------------------------------------------------ exact tier
def exact_inputs(C, dtype, seed):
    """x in {-1, +1}, balanced in every plane (so in every unit and every channel): with eps = 0 every unit mean is
    0, the variance 1 and xh = x exactly.  gamma, beta, the Dropout2d scale from {0, 1, 2} and the identity are small
    dyadic numbers and gy small integers: every product, sum and quotient by M = 256 is exact in float32, so
    the float64 result rounded once to the dtype is the only correct answer"""
    gen = torch.Generator().manual_seed(seed)
    B, (H, W) = 2, BC.EXACT_HW
    n = H * W
    x = torch.ones((B, C, n))
    for b in range(B):
        for c in range(C):
            x[b, c, torch.randperm(n, generator=gen)[:n // 2]] = -1.0
    pick = torch.tensor([0.25, 0.5, 1.0, 2.0])
    out = {'x': x.reshape(B, C, H, W).to(dtype),
           'identity': (torch.randint(-8, 9, (B, C, H, W), generator=gen) / 4).to(dtype),
           'gy': torch.randint(-4, 5, (B, C, H, W), generator=gen).to(dtype),
           'scale': torch.tensor([0.0, 1.0, 2.0])[torch.randint(0, 3, (B, C), generator=gen)].to(dtype),
           'gamma': pick[torch.randint(0, 4, (C,), generator=gen)],
           'beta': torch.randint(-4, 5, (C,), generator=gen) / 4,
           'running_mean': torch.randint(-8, 9, (C,), generator=gen) / 8,
           'running_var': torch.randint(4, 13, (C,), generator=gen) / 8}
    return out


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C', BC.CHANNELS)
@pytest.mark.parametrize('moved', (False, True))
def test_exact_on_constructed_inputs(dtype, C, moved):
    c = exact_inputs(C, dtype, 20 + C)
    place = (lambda t: Moved(t, dev(t)).t) if moved else dev
    x, idt, gy = place(c['x']), place(c['identity']), place(c['gy'])
    assert ops.bntail_route(x, idt, gy) == BC.expected_route(dtype, BC.EXACT_HW, aligned=not moved)
    M = float(c['x'].numel() // C)
    mom = 0.25
    for with_scale, with_id in itertools.product((False, True), (False, True)):
        rm, rv = dev(c['running_mean'].clone()), dev(c['running_var'].clone())
        scale = dev(c['scale']) if with_scale else None
        y_out = Moved(x) if moved else None
        y, mean, invstd = ops.bntail_apply(x, dev(c['gamma']), dev(c['beta']), rm, rv, 0.0, mom, 'relu',
                                           part=ops.bntail_stats(x), identity=idt if with_id else None, scale=scale,
                                           save=True, out=None if y_out is None else y_out.t)
        assert torch.equal(mean.cpu(), torch.zeros(C)) and torch.equal(invstd.cpu(), torch.ones(C))
        # the running update in float32, operation by operation as include/nmsa.h states it
        keep = torch.tensor(1.0) - torch.tensor(mom)
        assert torch.equal(rm.cpu(), keep * c['running_mean'] + torch.tensor(mom) * torch.zeros(C))
        assert torch.equal(rv.cpu(), keep * c['running_var'] + torch.tensor(mom) * (torch.tensor(M) / torch.tensor(M - 1.0)))
        x64, s64 = c['x'].double(), (c['scale'].double().reshape(2, C, 1, 1) if with_scale else 1.0)
        g64 = c['gamma'].double().reshape(1, C, 1, 1)
        z = (x64 * g64 + c['beta'].double().reshape(1, C, 1, 1)) * s64 + (c['identity'].double() if with_id else 0.0)
        y64 = z.clamp_min(0.0)
        assert torch.equal(y.cpu(), y64.to(dtype))
        # backward, the gate from the y the device wrote
        gz = c['gy'].double() * (y.cpu().double() > 0)
        gu = gz * s64
        dbeta, dgamma = gu.sum((0, 2, 3)), (gu * x64).sum((0, 2, 3))
        gx64 = g64 * ((gu - (dbeta / M).reshape(1, C, 1, 1)) - x64 * (dgamma / M).reshape(1, C, 1, 1))
        args = (gy, x, y, dev(c['gamma']), None, mean, invstd, 'relu')
        outs = (Moved(x), Moved(x)) if moved else (None, None)
        gx, gid, dg, db = ops.bntail_backward_apply(*args, scale=scale, part=ops.bntail_backward_reduce(*args, scale=scale),
                                                    need_x=True, need_identity=True, need_params=True,
                                                    out_x=outs[0] and outs[0].t, out_identity=outs[1] and outs[1].t)
        assert torch.equal(gx64.float().double(), gx64), 'the exact tier must be exact in float32'
        assert torch.equal(gx.cpu(), gx64.to(dtype)) and torch.equal(gid.cpu(), gz.to(dtype))
        assert torch.equal(dg.cpu(), dgamma.float()) and torch.equal(db.cpu(), dbeta.float())
        dg2, db2 = ops.bntail_backward_reduce(*args, scale=scale, finish=True)
        assert torch.equal(dg2, dg) and torch.equal(db2, db)
        gx_eval = ops.bntail_backward_apply(*args, scale=scale)[0]
        assert torch.equal(gx_eval.cpu(), (g64 * gu).to(dtype))
        if moved:
            assert y_out.untouched() and outs[0].untouched() and outs[1].untouched()


# ------------------------------------------------------------------------------ bounds tier
@pytest.mark.parametrize('B,C,hw', BC.SHAPES)
@pytest.mark.parametrize('dtype', DTYPES)
def test_each_kernel_within_its_bound(B, C, hw, dtype):
    c = case(B, C, hw, dtype)
    x, idt, gy = dev(c['x']), dev(c['identity']), dev(c['gy'])
    gamma, beta = dev(c['gamma']), dev(c['beta'])
    assert ops.bntail_route(x, idt, gy) == BC.expected_route(dtype, hw)
    worst = {}
    # statistics: the unit partials, merged exactly
    part = ops.bntail_stats(x, part=torch.empty(ops.bntail_workspace_bytes(x.shape) // 4, device=DEV))
    U = R.units(B, hw[0] * hw[1])
    plain = R.tail_forward(c['x'], c['gamma'], c['beta'], c['running_mean'], c['running_var'], EPS, MOM, True, 'relu')
    mean, var = R.merge_partials64(part[:C * U * 2].reshape(C, U, 2), B, hw[0] * hw[1])
    check(mean, plain['mean'], 'mean', worst)
    check(var, plain['var'], 'var', worst)
    for training in (True, False):
        for with_scale, with_id, act in COMBOS:
            sc, it = (c['scale'] if with_scale else None), (c['identity'] if with_id else None)
            rm, rv = dev(c['running_mean'].clone()), dev(c['running_var'].clone())
            y, m, s = ops.bntail_apply(x, gamma, beta, rm, rv, EPS, MOM, act, part=part if training else None,
                                       identity=dev(it), scale=dev(sc), save=True)
            f = R.tail_forward(c['x'], c['gamma'], c['beta'], c['running_mean'], c['running_var'], EPS, MOM, training,
                               act, it, sc, dtype)
            tag = ('t' if training else 'e') + act[0]
            check(y, f['y'], 'y' + tag, worst)
            check(m, f['mean'], 'm' + tag, worst)
            check(s, f['invstd'], 'i' + tag, worst)
            check(rm, f['running_mean'], 'rm' + tag, worst)
            check(rv, f['running_var'], 'rv' + tag, worst)
            if not training:
                assert torch.equal(rm.cpu(), c['running_mean']) and torch.equal(rv.cpu(), c['running_var'])
            # backward: gy, x, y (or the identity), mean and invstd are INPUTS of the kernels, given by the test
            y_in = f['y'].v.to(dtype)
            m_in, s_in = f['mean'].v.float(), f['invstd'].v.float()
            aux = y_in if act == 'relu' else it
            args = (gy, x, dev(aux), gamma, beta, dev(m_in), dev(s_in), act)
            want = R.tail_backward(c['gy'], c['x'], c['gamma'], c['beta'], m_in, s_in, training, act, y_in, it, sc, dtype)
            if training:
                ws = ops.bntail_backward_reduce(*args, scale=dev(sc))
                gx, gid, dg, db = ops.bntail_backward_apply(*args, scale=dev(sc), part=ws, need_identity=True,
                                                            need_params=True)
                dg2, db2 = ops.bntail_backward_reduce(*args, scale=dev(sc), finish=True)
                assert torch.equal(dg, dg2) and torch.equal(db, db2)
            else:
                dg, db = ops.bntail_backward_reduce(*args, scale=dev(sc), finish=True)
                gx, gid, _, _ = ops.bntail_backward_apply(*args, scale=dev(sc), need_identity=True)
            for key, got in (('gx', gx), ('gid', gid), ('dgamma', dg), ('dbeta', db)):
                check(got, want[key], key + tag, worst)
    print(f'B {B} C {C} {hw} {dtype}: ' + ' '.join(f'{k} {v:.3f}' for k, v in worst.items()))


def test_ill_conditioned_statistics():
    """mean 64, deviation 1/16 in float32: a variance from E[x^2] - E[x]^2 misses by several percent"""
    gen = torch.Generator().manual_seed(3)
    for B, C, hw in ((2, 5, (15, 20)), (3, 5, BC.SEG_HW)):
        x = 64.0 + torch.randn((B, C) + hw, generator=gen) / 16
        f = R.tail_forward(x, torch.ones(C), torch.zeros(C), torch.zeros(C), torch.ones(C), EPS, MOM, True, 'relu')
        assert float((f['var'].e / f['var'].v).max()) < 0.02, 'the bound itself must be tighter than the defect'
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        y, mean, invstd = ops.bntail_apply(dev(x), torch.ones(C, device=DEV), torch.zeros(C, device=DEV), rm, rv, EPS,
                                           MOM, 'relu', part=ops.bntail_stats(dev(x)), save=True)
        var = 1.0 / invstd.double().cpu() ** 2 - EPS
        assert R.worst_ratio(mean, f['mean']) <= 1.0 and R.worst_ratio(invstd, f['invstd']) <= 1.0
        assert R.worst_ratio(rv, f['running_var']) <= 1.0 and R.worst_ratio(y, f['y']) <= 1.0
        rel = ((var - f['var'].v) / f['var'].v).abs().max()
        print(f'{hw}: relative error of the variance {float(rel):.2e}')
        assert rel < 1e-3


# ------------------------------------------------------------------------------ whole blocks
@pytest.fixture(scope='module')
def golden():
    return BC.GoldenFile(GOLDEN)


@pytest.mark.parametrize('name,act,mode,ds,p', BC.golden_records())
def test_block_against_the_recorded_reference(golden, monkeypatch, name, act, mode, ds, p):
    rec = golden.record(BC.record_name(name, act, mode, ds, p))
    module = BC.build_block(name, act, ds, p)
    module.load_state_dict(BC.GoldenFile.state_dict(rec), strict=True)
    module.to(DEV).train(mode == 'train')
    want = R.block_reference(name, BC.GoldenFile.state_dict(rec), rec['x'], rec['gy'], act, mode == 'train',
                             stride=BC.golden_channels(name, ds)[2], scale=rec.get('scale'))
    for what, own, accumulated in want['margins']:                  # no gate can flip: no position is left out
        assert own > 1.0 and accumulated > 1.0, (what, own, accumulated)
    if 'scale' in rec:
        # the recorded draw of the CPU generator; that the module draws as F.dropout2d does is a test of its own
        monkeypatch.setattr(block_module, 'dropout2d_scale', lambda x, p_: dev(rec['scale']).reshape(x.shape[0], -1, 1, 1))
    calls = count_calls(monkeypatch)
    got = BC.run_record(module, rec, DEV)
    tails = 3 if name == 'bottleneck' else 2
    assert calls.count('bntail_apply') == tails and calls.count('bntail_stats') == (tails if mode == 'train' else 0)
    worst = {}
    for key, ref in want.items():
        if key != 'margins':
            check(got[key], ref, key.split('/')[-1], worst)
    tracked = got['state/norm1.num_batches_tracked'].cpu() - rec['state/norm1.num_batches_tracked'].long()
    assert int(tracked) == (1 if mode == 'train' else 0)
    print(' '.join(f'{k} {v:.3f}' for k, v in worst.items()))


# ------------------------------------------------------------------------------ module-level behaviour
def tail_module(C, act='relu', dropout_p=0.0):
    """a NonBottleneck1D's last segment as a module of its own: norm2 -> dropout -> (+ identity) -> act2_2"""
    class TailOnly(nn.Module):
        def __init__(self):
            super().__init__()
            self.norm = nn.BatchNorm2d(C)
            self.act = nn.ReLU(inplace=True) if act == 'relu' else nn.SiLU()
            self.dropout = nn.Dropout2d(dropout_p)

        def forward(self, x, identity=None):
            return block_module.batch_norm_tail(self.norm, self.act, x, identity, self.dropout if dropout_p > 0 else None)
    return TailOnly()


def load_tail(m, c):
    with torch.no_grad():
        m.norm.weight.copy_(c['gamma'])
        m.norm.bias.copy_(c['beta'])
        m.norm.running_mean.copy_(c['running_mean'])
        m.norm.running_var.copy_(c['running_var'])
    return m.to(DEV)


def run_tail(m, x, identity, gy, need_x=True, need_id=True):
    xx = x.clone().requires_grad_(need_x)
    ii = identity.clone().requires_grad_(need_id)
    m.zero_grad(set_to_none=True)
    y = m(xx, ii)
    if y.requires_grad:
        y.backward(gy)
    return {'y': y.detach(), 'gx': xx.grad, 'gid': ii.grad, 'dgamma': m.norm.weight.grad, 'dbeta': m.norm.bias.grad}


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('hw', ((8, 16), (15, 20), BC.SEG_HW))
def test_off_16_byte_tensors_give_the_same_bits_and_touch_nothing_else(dtype, hw):
    c = R.make_tail_inputs(2, 5, hw, 61, dtype)
    x, idt, gy, sc = dev(c['x']), dev(c['identity']), dev(c['gy']), dev(c['scale'])
    gamma, beta = dev(c['gamma']), dev(c['beta'])

    def run(x, idt, gy, outs=(None, None, None)):
        rm, rv = dev(c['running_mean'].clone()), dev(c['running_var'].clone())
        y, m, s = ops.bntail_apply(x, gamma, beta, rm, rv, EPS, MOM, 'silu', part=ops.bntail_stats(x), identity=idt,
                                   scale=sc, save=True, out=outs[0])
        args = (gy, x, idt, gamma, beta, m, s, 'silu')
        gx, gid, dg, db = ops.bntail_backward_apply(*args, scale=sc, part=ops.bntail_backward_reduce(*args, scale=sc),
                                                    need_identity=True, need_params=True, out_x=outs[1],
                                                    out_identity=outs[2])
        return y, m, s, rm, rv, gx, gid, dg, db
    base = run(x, idt, gy)
    mx, mi, mg = Moved(x, x), Moved(idt, idt), Moved(gy, gy)
    assert ops.bntail_route(mx.t, mi.t, mg.t)[0] == ELEMENT
    outs = [Moved(x), Moved(x), Moved(x)]
    moved = run(mx.t, mi.t, mg.t, tuple(o.t for o in outs))
    for i, (a, b) in enumerate(zip(base, moved)):
        assert torch.equal(a, b), i
    assert all(o.untouched() for o in outs) and mx.untouched() and mi.untouched() and mg.untouched()
    assert torch.equal(mx.t, x)
    # one map off 16 bytes is enough for the element route
    for i, (a, b) in enumerate(zip(base, run(x, mi.t, gy))):
        assert torch.equal(a, b), i


@pytest.mark.parametrize('dtype', (F32, BF16))
def test_same_bits_on_every_call_and_graph_replay(dtype):
    c = R.make_tail_inputs(3, 53, (15, 20), 62, dtype)
    x, idt, gy, sc = dev(c['x']), dev(c['identity']), dev(c['gy']), dev(c['scale'])
    gamma, beta = dev(c['gamma']), dev(c['beta'])
    rm0, rv0 = dev(c['running_mean']), dev(c['running_var'])
    rm, rv = rm0.clone(), rv0.clone()

    def step():
        """the library's chain of a training step: one stream, no branches"""
        rm.copy_(rm0)
        rv.copy_(rv0)
        y, m, s = ops.bntail_apply(x, gamma, beta, rm, rv, EPS, MOM, 'relu', part=ops.bntail_stats(x), identity=idt,
                                   scale=sc, save=True)
        args = (gy, x, y, gamma, None, m, s, 'relu')
        back = ops.bntail_backward_apply(*args, scale=sc, part=ops.bntail_backward_reduce(*args, scale=sc),
                                         need_identity=True, need_params=True)
        return (y, m, s, rm.clone(), rv.clone()) + back
    first = step()
    torch.cuda.synchronize()
    for a, b in zip(first, step()):
        assert torch.equal(a, b)
    # the step has run twice already, so nothing is initialised inside the capture; no side stream is taken from
    # torch's pool here: which hardware queue a later test's streams land on depends on how many were handed out
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(2):
        for t in captured:
            t.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(first, captured):
            assert torch.equal(a, b)


def test_three_training_steps_move_the_running_statistics_as_torch_does():
    B, C, hw = 3, 16, (15, 20)
    c = R.make_tail_inputs(B, C, hw, 63)
    ours, theirs = load_tail(tail_module(C), c), nn.BatchNorm2d(C).to(DEV)
    theirs.load_state_dict(ours.norm.state_dict())
    rm, rv = R.E(c['running_mean']), R.E(c['running_var'])
    gen = torch.Generator().manual_seed(64)
    for step in range(3):
        x = c['x'] * (1.0 + 0.5 * step) + torch.randn(c['x'].shape, generator=gen)
        f = R.tail_forward(x, c['gamma'], c['beta'], rm, rv, EPS, MOM, True, 'relu')
        rm, rv = f['running_mean'], f['running_var']
        ours(dev(x))
        theirs(dev(x))
    for got in (ours.norm, theirs):
        assert R.worst_ratio(got.running_mean, rm) <= 1.0 and R.worst_ratio(got.running_var, rv) <= 1.0
        assert int(got.num_batches_tracked) == 3
    assert float((rv.e / rv.v).max()) < 1e-4


@pytest.mark.parametrize('dtype', (F32, BF16))
def test_dropout_zeroes_the_planes_of_the_torch_composition(monkeypatch, dtype):
    B, C, hw = 3, 16, (8, 16)
    torch.manual_seed(5)
    fused = model.NonBottleneck1D(C, C, dropout_p=0.5).to(DEV, dtype)
    x = torch.randn((B, C) + hw, device=DEV, dtype=dtype)
    calls = count_calls(monkeypatch)
    torch.manual_seed(123)
    y = fused(x)
    assert calls.count('bntail_apply') == 2
    # the same block on the torch path
    monkeypatch.setattr(block_module, '_fused_act', lambda *a: None)
    plain = model.NonBottleneck1D(C, C, dropout_p=0.5).to(DEV, dtype)
    plain.load_state_dict(fused.state_dict())
    calls.clear()
    torch.manual_seed(123)
    z = plain(x)
    assert not calls
    # a zeroed plane of the last segment shows as y == act(identity) over the whole plane
    zero_f = (y == torch.relu(x)).flatten(2).all(2)
    zero_p = (z == torch.relu(x)).flatten(2).all(2)
    assert torch.equal(zero_f, zero_p) and 0 < int(zero_f.sum()) < B * C


def test_gradient_subsets_skip_the_rest_and_keep_the_bits(monkeypatch):
    B, C, hw = 2, 16, (15, 20)
    c = R.make_tail_inputs(B, C, hw, 65, BF16)
    x, idt, gy = dev(c['x']), dev(c['identity']), dev(c['gy'])
    calls = count_calls(monkeypatch)
    for act in BC.ACTS:
        m = load_tail(tail_module(C, act), c)
        full = run_tail(m, x, idt, gy)
        calls.clear()

        def same(got, keys):
            for key in ('gx', 'gid', 'dgamma', 'dbeta'):
                if key in keys:
                    assert torch.equal(got[key], full[key]), (act, key)
                else:
                    assert got[key] is None, (act, key)
            assert torch.equal(got['y'], full['y'])
        same(run_tail(m, x, idt, gy), ('gx', 'gid', 'dgamma', 'dbeta'))
        assert calls == list(OPS)
        m.requires_grad_(False)                                     # frozen parameters
        calls.clear()
        same(run_tail(m, x, idt, gy), ('gx', 'gid'))
        assert calls == list(OPS)
        calls.clear()
        same(run_tail(m, x, idt, gy, need_id=False), ('gx',))
        calls.clear()
        same(run_tail(m, x, idt, gy, need_x=False), ('gid',))      # only the identity: no reduction
        assert calls == ['bntail_stats', 'bntail_apply', 'bntail_backward_apply']
        calls.clear()
        got = run_tail(m, x, idt, gy, need_x=False, need_id=False)  # nothing: no node
        assert got['y'].grad_fn is None and calls == ['bntail_stats', 'bntail_apply']
        m.requires_grad_(True)                                      # only the parameters: the reduction finishes alone
        calls.clear()
        same(run_tail(m, x, idt, gy, need_x=False, need_id=False), ('dgamma', 'dbeta'))
        assert calls == ['bntail_stats', 'bntail_apply', 'bntail_backward_reduce']
        calls.clear()
        with torch.no_grad():
            y = m(x, idt)
        assert y.grad_fn is None and torch.equal(y, full['y']) and calls == ['bntail_stats', 'bntail_apply']


def test_eval_mode_with_gradients(monkeypatch):
    B, C, hw = 2, 16, (15, 20)
    c = R.make_tail_inputs(B, C, hw, 66)
    x, idt, gy = dev(c['x']), dev(c['identity']), dev(c['gy'])
    calls = count_calls(monkeypatch)
    for act in BC.ACTS:
        m = load_tail(tail_module(C, act), c).eval()
        calls.clear()
        got = run_tail(m, x, idt, gy)
        assert calls == ['bntail_apply', 'bntail_backward_reduce', 'bntail_backward_apply']
        f = R.tail_forward(c['x'], c['gamma'], c['beta'], c['running_mean'], c['running_var'], EPS, MOM, False, act,
                           c['identity'])
        want = R.tail_backward(c['gy'], c['x'], c['gamma'], c['beta'], f['mean'], f['invstd'], False, act, f['y'],
                               c['identity'])
        assert R.worst_ratio(got['y'], f['y']) <= 1.0
        for key in ('gx', 'gid', 'dgamma', 'dbeta'):
            assert R.worst_ratio(got[key], want[key]) <= 1.0, (act, key)
        assert torch.equal(m.norm.running_mean.cpu(), c['running_mean']) and int(m.norm.num_batches_tracked) == 0
        m.requires_grad_(False)                                     # frozen parameters: no reduction
        calls.clear()
        frozen = run_tail(m, x, idt, gy)
        assert calls == ['bntail_apply', 'bntail_backward_apply'] and torch.equal(frozen['gx'], got['gx'])


def test_half_module_parameters_are_cast_for_the_kernels():
    B, C, hw = 2, 16, (15, 20)
    c = R.make_tail_inputs(B, C, hw, 67, F16)
    m = load_tail(tail_module(C, 'relu'), c).half()
    p16 = {k: getattr(m.norm, n).detach().float().cpu() for k, n in (('gamma', 'weight'), ('beta', 'bias'),
                                                                   ('running_mean', 'running_mean'),
                                                                   ('running_var', 'running_var'))}
    got = run_tail(m, dev(c['x']), dev(c['identity']), dev(c['gy']))
    f = R.tail_forward(c['x'], p16['gamma'], p16['beta'], p16['running_mean'], p16['running_var'], EPS, MOM, True, 'relu',
                       c['identity'], None, F16)
    assert R.worst_ratio(got['y'], f['y']) <= 1.0 and got['dgamma'].dtype == F16
    assert m.norm.running_mean.dtype == F16 and R.worst_ratio(m.norm.running_mean, f['running_mean'].rounded(F16)) <= 1.0
    assert R.worst_ratio(m.norm.running_var, f['running_var'].rounded(F16)) <= 1.0


# ------------------------------------------------------------------------------ refusals and fallbacks
def test_one_value_per_channel_in_training_raises():
    m = tail_module(4).to(DEV)
    with pytest.raises(ValueError, match='Expected more than 1 value per channel'):
        m(torch.randn((1, 4, 1, 1), device=DEV))
    m.eval()(torch.randn((1, 4, 1, 1), device=DEV))
    with pytest.raises(ValueError):
        ops.bntail_apply(torch.randn((1, 4, 1, 1), device=DEV), *(torch.ones(4, device=DEV) for _ in range(4)), EPS,
                         MOM, part=torch.zeros(64, device=DEV))


def torch_composition(m, x, identity):
    out = m.norm(x)
    out = out + identity
    return m.act(out)


def test_every_fallback_is_taken_and_is_the_torch_composition(monkeypatch):
    B, C, hw = 2, 16, (15, 20)
    c = R.make_tail_inputs(B, C, hw, 68)
    x, idt = dev(c['x']), dev(c['identity'])
    calls = count_calls(monkeypatch)

    def fresh():
        return load_tail(tail_module(C), c)

    def torch_path(m, a, b):
        calls.clear()
        state = {k: v.clone() for k, v in m.state_dict().items()}
        y = m(a, b)
        assert not calls
        m.load_state_dict(state)
        want = torch_composition(m, a, b)
        assert y.dtype == want.dtype and torch.equal(y, want)
    m = fresh()
    m(x, idt)
    assert calls == ['bntail_stats', 'bntail_apply']
    # channels-last and non-dense inputs
    torch_path(fresh(), x.contiguous(memory_format=torch.channels_last), idt)
    torch_path(fresh(), x, idt.contiguous(memory_format=torch.channels_last))
    wide = torch.zeros((B, C, hw[0], hw[1] + 3), device=DEV)
    wide[..., :hw[1]] = x
    torch_path(fresh(), wide[..., :hw[1]], idt)
    # mixed dtypes: an f32 identity beside a half main path (autocast), where `output + identity` promotes
    m = fresh()
    calls.clear()
    with torch.autocast('cuda', dtype=F16):
        y = m(x.half(), idt)
    assert not calls and y.dtype == F32
    # another normalization, another activation
    class Other(nn.Module):
        def __init__(self, norm, act):
            super().__init__()
            self.norm, self.act = norm, act

        def forward(self, a, b):
            return block_module.batch_norm_tail(self.norm, self.act, a, b)
    for norm, act in ((nn.GroupNorm(4, C), nn.ReLU()), (nn.BatchNorm2d(C), nn.GELU()), (nn.BatchNorm2d(C, momentum=None), nn.ReLU()),
                      (nn.BatchNorm2d(C, affine=False), nn.ReLU()), (nn.BatchNorm2d(C, track_running_stats=False), nn.ReLU())):
        torch_path(Other(norm, act).to(DEV), x, idt)
    # CPU tensors
    calls.clear()
    tail_module(C)(c['x'], c['identity'])
    assert not calls


def test_small_maps_take_torch_for_speed(monkeypatch):
    monkeypatch.undo()                                              # the shipped threshold
    n = block_module.FUSED_MIN_ELEMENTS
    assert n == 8 * 2 ** 20
    calls = count_calls(monkeypatch)
    m = tail_module(64).to(DEV, BF16)
    with torch.no_grad():
        m(torch.randn((8, 64, 128, 128), device=DEV, dtype=BF16))   # exactly n elements
        assert calls == ['bntail_stats', 'bntail_apply']
        calls.clear()
        m(torch.randn((8, 64, 128, 127), device=DEV, dtype=BF16))
        m(torch.randn((2, 64, 15, 20), device=DEV, dtype=BF16))
    assert not calls


@pytest.mark.parametrize('dtype,cast', ((F32, F16), (F16, F16), (BF16, BF16)))
def test_autocast_stays_fused_and_keeps_the_dtype(monkeypatch, dtype, cast):
    B, C, hw = 2, 16, (15, 20)
    c = R.make_tail_inputs(B, C, hw, 69, dtype)
    m = load_tail(tail_module(C), c)
    calls = count_calls(monkeypatch)
    with torch.autocast('cuda', dtype=cast):
        got = run_tail(m, dev(c['x']), dev(c['identity']), dev(c['gy']))
    assert calls == list(OPS) and got['y'].dtype == dtype and got['gx'].dtype == dtype and got['dgamma'].dtype == F32
    f = R.tail_forward(c['x'], c['gamma'], c['beta'], c['running_mean'], c['running_var'], EPS, MOM, True, 'relu',
                       c['identity'], None, dtype)
    assert R.worst_ratio(got['y'], f['y']) <= 1.0
