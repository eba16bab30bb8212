"""The scene task on the device — `ops.scene_step` (csrc/scene.hip), `CrossEntropyLossScene`,
`ConfusionMatrix`, `ScenePostprocessing`, `SceneTaskHelper` — against torch on the CPU, computed
here, and against tests/golden/scene_task.npz (tools/gen_golden_scene.py: the reference's own
modules on the CPU).

Oracles and bounds (none of them measured on the code under test):
  idx       equals `torch.max(F.softmax(x.float(), 1), 1)` on the CPU exactly.  The inputs are
            seeded so that no row has distinct top-two logits with equal float32 probabilities
            (asserted on the inputs); rows with exactly duplicated maximal logits are part of
            every batch of three rows or more, their expected index is torch's, computed.
  score, loss, grad
            compared with the same torch expressions evaluated in float64.  Allowed error per
            element: TOL_FACTOR (4) x the LARGEST error torch's own float32 CPU result shows
            against float64 on the same inputs — the order of summation legitimately differs —
            and never below one float32 ulp of the value.  bf16 / f16 gradients: plus one
            rounding of the output dtype (half an ulp of it at the value).
            torch's float32 errors on the inputs of the shape and dtype tests (128 calls each),
            measured on the CPU, the largest of a call in float32 ulps of the tensor's largest
            value, as minimum / median / maximum over the calls: score 0 / 0.74 / 3.8, loss
            0 / 0.35 / 2.8, numerator 0 / 0.29 / 1.7, divisor 0 / 0 / 1.3, grad 0 / 0.69 / 5.0.
            The allowed error of a call is therefore between 1 ulp of each value (where torch
            happens to be exact, half of the loss values among them) and 20 ulps of the largest.
  confusion matrix, status, scene_acc / scene_bacc
            exact.
"""
import ctypes as C_

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _golden import load, jload

pytestmark = pytest.mark.gpu

TOL_FACTOR = 4.0
CLASSES = (1, 2, 10, 45, 64, 65, 200, 4096)
BATCHES = (1, 3, 4, 5, 64, 257)
HALF_CLASSES, HALF_BATCHES = (1, 10, 65, 200), (3, 64)
_LABEL_DTYPES = (torch.int64, torch.int32, torch.uint8)


# --------------------------------------------------------------------------- inputs and oracles
def _index_rule_is_decided(x32):
    """no row with distinct top-two logits and equal float32 probabilities"""
    if x32.shape[1] < 2:
        return True
    p = F.softmax(x32, dim=1)
    top = torch.topk(x32, 2, dim=1)
    pa, pb = p.gather(1, top.indices[:, :1]), p.gather(1, top.indices[:, 1:])
    return not bool(((top.values[:, :1] != top.values[:, 1:]) & (pa == pb)).any())


def make_inputs(C, B, dtype=torch.float32, seed=0, void=True):
    """-> (logits [B, C] of `dtype`, labels int64 [B] in 0..C, weights float32 [C]) on the CPU;
    every row r with r % 3 == 1 has two or three exactly equal largest logits (C >= 2)"""
    for attempt in range(8):
        g = torch.Generator().manual_seed(1000 * C + 10 * B + seed + 7919 * attempt)
        x = (torch.randn((B, C), generator=g) * 3.0).to(dtype)
        for r in range(1, B, 3):
            if C >= 2:
                cols = torch.randperm(C, generator=g)[:min(C, 2 + r % 2)]
                x[r, cols] = (x[r].float().max() + 0.5).to(dtype)
        labels = torch.randint(1, C + 1, (B,), generator=g)
        if void and B >= 3:
            labels[torch.rand((B,), generator=g) < 0.25] = 0
            labels[B - 1] = 0
        weights = torch.rand((C,), generator=g) + 0.25
        if _index_rule_is_decided(x.float()):
            return x, labels, weights
    raise AssertionError('no seed with a decided index rule')


def _ce(x, target, w, eps, reduction='mean'):
    return torch.nn.CrossEntropyLoss(weight=w, label_smoothing=eps, ignore_index=-1,
                                     reduction=reduction)(x, target)


def reference(x, labels, w=None, eps=0.0):
    """torch on the CPU for logits `x` (any float dtype, promoted exactly), labels 0..C (anything
    else: void) -> dict of float32 results ('*32') and float64 truths ('*64')"""
    C = x.shape[1]
    target = torch.where((labels >= 1) & (labels <= C), labels, torch.zeros_like(labels)).long() - 1
    out = {}
    for tag, dt in (('32', torch.float32), ('64', torch.float64)):
        xx = x.to(dt).clone().requires_grad_(True)
        ww = None if w is None else w.to(dt)
        score, idx = torch.max(F.softmax(xx.detach(), dim=1), dim=1)
        loss = _ce(xx, target, ww, eps)
        grad, = torch.autograd.grad(loss, xx)
        with torch.no_grad():
            numerator = _ce(xx, target, ww, eps, 'sum')
            valid = target >= 0
            divisor = (ww[target[valid]].sum() if ww is not None else valid.sum().to(dt))
        out['score' + tag], out['loss' + tag], out['grad' + tag] = score, loss.detach(), grad
        out['num' + tag], out['div' + tag] = numerator, divisor
        if tag == '32':
            out['idx'] = idx
    cm = torch.bincount(target[valid] * C + out['idx'][valid], minlength=C * C).reshape(C, C)
    out['cm'], out['target'] = cm, target
    return out


def ulp32(v64):
    return torch.from_numpy(np.spacing(np.abs(v64.numpy()).astype(np.float32)).astype(np.float64))


def ulp_of(v64, dtype):
    """spacing of `dtype` at the value (the subnormal spacing below the smallest normal)"""
    if dtype == torch.float32:
        return ulp32(v64)
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = torch.floor(torch.log2(v64.abs().clamp(min=2.0 ** emin)))
    return torch.pow(2.0, e - mant)


def check_close(name, got, ref32, truth64, out_dtype=torch.float32, scaled_after_rounding=False, report=None):
    """the rule of the module docstring; NaN matches NaN (an all-void batch's 0 / 0).
    `scaled_after_rounding`: the 16-bit value was rounded, multiplied by a factor and rounded again
    (backward of a stored gradient): the first rounding is off by at most the unit roundoff u =
    2^-(significant bits) of the value, which the factor carries over unchanged as a RELATIVE error
    (in ulps of the scaled result it can exceed one half: 0.375 * [1, 2) lands two binades lower),
    the second by half an ulp of the result: u * |value| + ulp / 2"""
    got64, truth64 = got.detach().cpu().to(torch.float64).reshape(-1), truth64.reshape(-1)
    ref64 = ref32.to(torch.float64).reshape(-1)
    both_nan = torch.isnan(ref64) & torch.isnan(truth64)
    e_ref = torch.where(both_nan, torch.zeros_like(truth64), (ref64 - truth64).abs()).max()
    allowed = torch.maximum(TOL_FACTOR * e_ref, ulp32(truth64))
    if out_dtype != torch.float32:
        allowed = allowed + 0.5 * ulp_of(truth64, out_dtype)
        if scaled_after_rounding:
            allowed = allowed + truth64.abs() * 2.0 ** -(8 if out_dtype == torch.bfloat16 else 11)
    err = (got64 - truth64).abs()
    ok = (err <= allowed) | (torch.isnan(got64) & torch.isnan(truth64))
    finite = truth64[torch.isfinite(truth64)]
    scale = float(ulp32(finite.abs().max().reshape(1))[0]) if finite.numel() else 1.0
    worst = float((err / allowed)[torch.isfinite(err)].max()) if bool(torch.isfinite(err).any()) else 0.0
    print(f'{name}: e_ref {float(e_ref) / scale:.3f} ulp of the largest value, worst error / allowed {worst:.3f}')
    if report is not None:
        report.append((name, float(e_ref) / scale))
    assert bool(ok.all()), (name, int((~ok).sum()), got64[~ok][:4], truth64[~ok][:4], float(e_ref))


def run_and_check(x, labels, w, eps, label_dtype=torch.int64, tag=''):
    from nicr_mt_scene_analysis_amd import ops
    B, C = x.shape
    key = (tag, tuple(x.shape), x.dtype, eps, w is not None)
    ref = reference(x, labels, w, eps)
    dev = torch.device('cuda')
    confmat = torch.full((C, C), 3, dtype=torch.int64, device=dev)           # accumulated into
    r = ops.scene_step(x.to(dev), labels.to(label_dtype).to(dev), None if w is None else w.to(dev), eps,
                       want=('score', 'idx', 'loss', 'grad'), confmat=confmat)
    assert r['idx'].dtype == torch.int64 and torch.equal(r['idx'].cpu(), ref['idx']), (key, 'idx')
    check_close(f'{key} score', r['score'], ref['score32'], ref['score64'])
    check_close(f'{key} loss', r['loss'][2], ref['loss32'], ref['loss64'])
    check_close(f'{key} numerator', r['loss'][0], ref['num32'], ref['num64'])
    check_close(f'{key} divisor', r['loss'][1], ref['div32'], ref['div64'])
    assert r['grad'].dtype == x.dtype and r['grad'].shape == x.shape
    check_close(f'{key} grad', r['grad'], ref['grad32'], ref['grad64'], out_dtype=x.dtype)
    assert torch.equal(confmat.cpu(), ref['cm'] + 3), (key, 'confmat')
    assert int(r['status'].item()) == 0
    return r, ref


# --------------------------------------------------------------------------- shapes and dtypes
@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('C', CLASSES)
def test_every_shape_float32(C, B):
    x, labels, w = make_inputs(C, B)
    label_dtype = _LABEL_DTYPES[(C + B) % 3] if C < 255 else _LABEL_DTYPES[(C + B) % 2]
    run_and_check(x, labels, None, 0.0, label_dtype)
    run_and_check(x, labels, w, 0.1, label_dtype)


@pytest.mark.parametrize('weighted,eps', ((True, 0.0), (False, 0.1), (False, 1.0), (True, 1.0)))
@pytest.mark.parametrize('C,B', ((10, 5), (65, 64)))
def test_weights_and_smoothing_apart(C, B, weighted, eps):
    x, labels, w = make_inputs(C, B, seed=1)
    run_and_check(x, labels, w if weighted else None, eps)


@pytest.mark.parametrize('B', HALF_BATCHES)
@pytest.mark.parametrize('C', HALF_CLASSES)
@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float16))
def test_half_precision_logits(dtype, C, B):
    x, labels, w = make_inputs(C, B, dtype=dtype, seed=2)
    run_and_check(x, labels, None, 0.0)
    run_and_check(x, labels, w, 0.1)


def test_rows_of_equal_logits():
    """whole rows equal, ties at the ends, ties across lanes and across a lane's stride"""
    from nicr_mt_scene_analysis_amd import ops
    for C in (2, 64, 65, 200):
        x = torch.randn((6, C), generator=torch.Generator().manual_seed(C))
        x[0] = 1.25
        x[1, [0, C - 1]] = 9.0
        x[2, [C - 1, C // 2]] = 9.0
        x[3, C - 1] = 9.0
        x[4, [C // 2, min(C - 1, C // 2 + 64)]] = 9.0
        x[5] = float('-inf')
        x[5, C - 1] = -3.0
        assert _index_rule_is_decided(x)
        want_score, want_idx = torch.max(F.softmax(x, dim=1), dim=1)
        r = ops.scene_step(x.cuda())
        assert torch.equal(r['idx'].cpu(), want_idx), C
        assert sorted(r) == ['idx', 'score']
        truth = torch.max(F.softmax(x.double(), dim=1), dim=1)[0]
        check_close(f'ties C={C}', r['score'], want_score, truth)


# --------------------------------------------------------------------------- void and range
@pytest.mark.parametrize('weighted,eps', ((False, 0.0), (True, 0.1)))
def test_void_rows_all_void_and_labels_out_of_range(weighted, eps):
    from nicr_mt_scene_analysis_amd import _lib as L
    from nicr_mt_scene_analysis_amd import ops
    C, B = 10, 7
    x, labels, w = make_inputs(C, B, seed=3, void=False)
    w = w if weighted else None
    dev = torch.device('cuda')
    # all rows void: 0 / 0 loss, zero gradient, nothing counted, no status bit
    r, ref = run_and_check(x, torch.zeros_like(labels), w, eps, tag='all void')
    assert bool(torch.isnan(ref['loss64'])) and bool(torch.isnan(r['loss'][2]))
    assert not bool(r['grad'].any()) and float(r['loss'][0]) == 0.0 and float(r['loss'][1]) == 0.0
    # one row void
    labels[2] = 0
    run_and_check(x, labels, w, eps, tag='one void')
    # labels C + 1 and beyond (and, for signed labels, below 0): the bit, the rows count as void
    for label_dtype, bad in ((torch.uint8, (C + 1, 255)), (torch.int32, (C + 1, -1)), (torch.int64, (1 << 40, -5))):
        broken = labels.clone()
        broken[0], broken[4] = bad
        ref = reference(x, broken, w, eps)
        assert int((ref['target'] < 0).sum()) == 3
        cm = torch.zeros((C, C), dtype=torch.int64, device=dev)
        r = ops.scene_step(x.to(dev), broken.to(label_dtype).to(dev), None if w is None else w.to(dev), eps,
                           want=('loss', 'grad'), confmat=cm)
        assert int(r['status'].item()) == L.NMSA_ST_VALUE_RANGE
        assert torch.equal(cm.cpu(), ref['cm']) and int(cm.sum()) == B - 3
        check_close('range loss', r['loss'][2], ref['loss32'], ref['loss64'])
        check_close('range grad', r['grad'], ref['grad32'], ref['grad64'])
        assert not bool(r['grad'][[0, 2, 4]].any())


# --------------------------------------------------------------------------- metric
def test_confusion_matrix_accumulates_and_resets():
    from nicr_mt_scene_analysis_amd import ops
    from nicr_mt_scene_analysis_amd.metric import ConfusionMatrix
    C = 45
    m = ConfusionMatrix(num_classes=C, device=torch.device('cuda'))
    want = torch.zeros((C, C), dtype=torch.int64)
    for seed, B in ((4, 64), (5, 257), (6, 3)):
        x, labels, _ = make_inputs(C, B, seed=seed)
        ref = reference(x, labels)
        ops.scene_step(x.cuda(), labels.cuda(), want=(), confmat=m.state_for_kernel())
        want += ref['cm']
        assert torch.equal(m.confmat.cpu(), want), seed
    # the parity path: indices without void rows
    valid = ref['target'] >= 0
    m.update(ref['idx'][valid].cuda(), ref['target'][valid].cuda())
    want += ref['cm']
    assert torch.equal(m.compute().cpu(), want) and m.compute().dtype == torch.int64
    state = m.confmat
    m.reset()
    assert m.confmat.data_ptr() == state.data_ptr() and int(m.confmat.sum()) == 0


def test_two_calls_are_bit_identical():
    from nicr_mt_scene_analysis_amd import ops
    x, labels, w = make_inputs(45, 257, seed=7)
    args = (x.cuda(), labels.cuda(), w.cuda(), 0.1)
    a = ops.scene_step(*args, want=('score', 'loss', 'grad'))
    b = ops.scene_step(*args, want=('score', 'loss', 'grad'))
    for k in ('score', 'loss', 'grad'):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


# --------------------------------------------------------------------------- null outputs
def test_a_call_writes_only_the_outputs_it_is_given():
    from nicr_mt_scene_analysis_amd import _lib as L
    C, B = 45, 37
    x, labels, w = make_inputs(C, B, seed=8)
    ref = reference(x, labels)
    dev = torch.device('cuda')
    xd, ld = x.to(dev), labels.to(dev)
    stream = L.stream_ptr(dev)

    def ptr(t, at=0):
        return C_.c_void_p(t.data_ptr() + at * t.element_size())

    # score alone, with and without labels: the words around it keep their guard value
    for lab in (None, ld):
        arena = torch.full((3 * B,), -12345.0, dtype=torch.float32, device=dev)
        L.check(L.lib().nmsa_scene_step(ptr(xd), L.NMSA_F32, None if lab is None else ptr(lab), L.NMSA_I64, B, C,
                                        None, 0.0, ptr(arena, B), None, None, None, None, None, stream), 'score')
        torch.cuda.synchronize()
        assert bool((arena[:B] == -12345.0).all()) and bool((arena[2 * B:] == -12345.0).all())
        check_close('score alone', arena[B:2 * B], ref['score32'], ref['score64'])
    # idx alone
    arena = torch.full((3 * B,), -7, dtype=torch.int64, device=dev)
    L.check(L.lib().nmsa_scene_step(ptr(xd), L.NMSA_F32, None, 0, B, C, None, 0.0, None, ptr(arena, B), None, None,
                                    None, None, stream), 'idx')
    torch.cuda.synchronize()
    assert bool((arena[:B] == -7).all()) and bool((arena[2 * B:] == -7).all())
    assert torch.equal(arena[B:2 * B].cpu(), ref['idx'])
    # loss alone: three floats, no gradient, no counts, the status word stays clear
    arena = torch.full((9,), -12345.0, dtype=torch.float32, device=dev)
    status = torch.zeros((3,), dtype=torch.int32, device=dev)
    L.check(L.lib().nmsa_scene_step(ptr(xd), L.NMSA_F32, ptr(ld), L.NMSA_I64, B, C, None, 0.0, None, None,
                                    ptr(arena, 3), None, None, ptr(status, 1), stream), 'loss')
    torch.cuda.synchronize()
    assert bool((arena[:3] == -12345.0).all()) and bool((arena[6:] == -12345.0).all()) and not bool(status.any())
    check_close('loss alone', arena[5], ref['loss32'], ref['loss64'])


# --------------------------------------------------------------------------- helper, capture, fixture
def _helper(C, weights=None, eps=0.0):
    from nicr_mt_scene_analysis_amd.task_helper import SceneTaskHelper
    h = SceneTaskHelper(C, class_weights=weights, label_smoothing=eps)
    h.initialize(torch.device('cuda'))
    return h


def test_validation_step_is_captured_once_and_replayed():
    C, B = 45, 64
    x, labels, w = make_inputs(C, B, seed=9)
    ref = reference(x, labels, w, 0.1)
    h = _helper(C, w.numpy(), 0.1)
    batch, post = {'scene': labels.to(torch.uint8).cuda()}, {'scene_output': x.cuda()}
    h.validation_step(batch, 0, post)                           # the eager call a capture needs first
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                               # a synchronising call would fail here
        losses, logs = h.validation_step(batch, 0, post)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(h._metric_cm.confmat.cpu(), 3 * ref['cm'])
    check_close('captured loss', losses['scene_total_loss'], ref['loss32'], ref['loss64'])
    check_close('captured log', logs['scene_total_loss'], ref['loss32'], ref['loss64'])
    h.check_status()


def test_fixture_both_epochs():
    """task helper and postprocessing against every recorded key of scene_task.npz; the inputs
    are regenerated from the recipe and digest-checked (a mismatch FAILS)"""
    from nicr_mt_scene_analysis_amd.model.postprocessing import ScenePostprocessing
    from nicr_mt_scene_analysis_amd.testing import synthetic as syn
    g = load('scene_task')
    keys = jload(g['keys'])
    post = ScenePostprocessing()
    for name in jload(g['names']):
        p = jload(g[f'{name}__params'])
        inputs = syn.make_scene_inputs(name)
        assert syn.scene_input_digest(inputs) == p['digest'], f'{name}: regenerated inputs differ'
        C, eps = p['n_classes'], p['label_smoothing']
        w = torch.from_numpy(inputs['weights']) if p['weighted'] else None
        h = _helper(C, None if w is None else w.numpy(), eps)
        row = 0
        for e, epoch in enumerate(inputs['batches']):
            assert [len(labels) for _, labels in epoch] == p['batch_rows']
            for j, (logits, labels) in enumerate(epoch):
                tag = f'{name} e{e} b{j} '
                x, labels = torch.from_numpy(logits), torch.from_numpy(labels)
                rows = slice(row, row + len(labels))
                row += len(labels)
                ref = reference(x, labels, w, eps)
                batch = {'scene': labels.cuda()}
                xd = x.cuda().requires_grad_(True)
                r_train = post.postprocess((xd, None), batch, is_training=True)
                assert list(r_train) == keys['post_training'] and r_train['scene_output'] is xd
                losses, logs = h.training_step(batch, j, r_train)
                assert list(losses) == keys['losses'] and sorted(logs) == keys['training_logs']
                recorded = torch.tensor(g[f'{name}__train_loss'][e, j])
                check_close(tag + 'train_loss', losses['scene_total_loss'], recorded, ref['loss64'])
                if not bool(torch.isnan(recorded)):
                    losses['scene_total_loss'].backward()
                    check_close(tag + 'grad', xd.grad, ref['grad32'], ref['grad64'])
                with torch.no_grad():
                    r = post.postprocess((xd.detach(), None), batch, is_training=False)
                    losses, logs = h.validation_step(batch, j, r)
                assert list(r) == keys['post_inference'] and sorted(logs) == keys['validation_logs']
                assert np.array_equal(r['scene_class_idx'].cpu().numpy(), g[f'{name}__idx'][rows])
                check_close(tag + 'score', r['scene_class_score'], torch.from_numpy(g[f'{name}__score'][rows]),
                            ref['score64'])
                check_close(tag + 'val_loss', losses['scene_total_loss'],
                            torch.tensor(g[f'{name}__val_loss'][e, j]), ref['loss64'])
            artifacts, examples, logs = h.validation_epoch_end()
            assert list(artifacts) == keys['artifacts'] and list(examples) == keys['examples']
            assert sorted(logs) == keys['epoch_end_logs']
            cm = artifacts['scene_cm'].cpu().numpy()
            assert cm.dtype == np.int64 and np.array_equal(cm, g[f'{name}__cm'][e]), (name, e)
            assert np.float32(logs['scene_acc'].item()) == g[f'{name}__acc'][e], (name, e)
            assert np.float32(logs['scene_bacc'].item()) == g[f'{name}__bacc'][e], (name, e)
            assert int(h._metric_cm.confmat.sum()) == 0                      # reset for the next epoch
        assert row == len(g[f'{name}__idx'])
        h.check_status()


# --------------------------------------------------------------------------- autograd
@pytest.mark.parametrize('dtype', (torch.float32, torch.bfloat16))
def test_backward_with_a_non_unit_upstream_factor(monkeypatch, dtype):
    from nicr_mt_scene_analysis_amd.loss import CrossEntropyLossScene
    C, B, eps, factor = 45, 64, 0.1, 0.375
    x, labels, w = make_inputs(C, B, dtype=dtype, seed=10)
    target = labels - 1                                         # the reference's shifted target
    truth, ref32 = {}, {}
    for store, dt in ((ref32, torch.float32), (truth, torch.float64)):
        xx = x.to(dt).clone().requires_grad_(True)
        loss = _ce(xx, target, w.to(dt), eps)
        (loss * factor).backward()
        store['loss'], store['grad'] = loss.detach(), xx.grad
    xd = x.cuda().requires_grad_(True)
    loss = CrossEntropyLossScene(weights=w.cuda(), label_smoothing=eps)(xd, target.cuda())
    assert loss.ndim == 0 and loss.dtype == torch.float32 and loss.requires_grad
    (loss * factor).backward()
    check_close('loss', loss, ref32['loss'], truth['loss'])
    # (the gradient is stored in the logits' dtype and scaled in backward: two roundings of it)
    check_close('grad', xd.grad, ref32['grad'], truth['grad'], out_dtype=dtype, scaled_after_rounding=True)
    # without a gradient to compute, the launch is not asked for one
    from nicr_mt_scene_analysis_amd import ops
    asked = []
    real = ops.scene_step
    monkeypatch.setattr(ops, 'scene_step', lambda *a, **k: asked.append(tuple(k['want'])) or real(*a, **k))
    with torch.no_grad():
        plain = CrossEntropyLossScene(weights=w.cuda(), label_smoothing=eps)(x.cuda(), target.cuda())
    CrossEntropyLossScene(weights=w.cuda(), label_smoothing=eps)(x.cuda().requires_grad_(True), target.cuda())
    assert asked == [('loss',), ('loss', 'grad')]
    assert not plain.requires_grad and torch.equal(plain, loss.detach())
