"""GPU tier: NaN, +inf, -inf and extreme finite values through the loss kernels and the scene step
(DESIGN.md 6n).  The case table, the oracles (the CPU in float64) and the rule live in
testing/nonfinite_losses.py; tests/test_nonfinite_losses_host.py checks on the CPU that the table is honest.

Every case reaches the kernel its table row names, as far as Python can see it: whether the forward launch wrote
a gradient the backward launch then confirmed (`speculation_stats`, `SpecState.stats`), the dtype of the labels
and the saved log-sum-exp of the two-kernel cross entropy, `_multi.supported`, `cos_supported`.

Findings the tests were written for (they fail on the commit before this one):
  * center focal loss: `fmaxf(NaN, 1e-4f)` is 1e-4f, so a NaN prediction left a finite loss sum
    (test_losses_answer_a_poison_as_the_oracle_does[focal-...]: 'loss class', finite against NaN)
  * scene step: the index of a row with a NaN or a +inf was the argmax of the raw logits, not the 0 of
    softmax -> max, the confusion matrix counted in that column, and a void row holding one got a zero gradient
    where F.cross_entropy gives NaN (test_scene_step_answers_a_poison_as_the_oracle_does: 'idx')
and three the tests turned up:
  * the backward of the two-walk cosine path gave a pixel WITHOUT target a NaN gradient when it held a NaN
    (0 * NaN; [cos-D1030-3x5-...]: 'the gradient of a pixel that is never read')
  * `cosine_embedding_rows` under label -1: `fmaxf(NaN - margin, 0)` is 0
  * cross entropy at large magnitudes: the exponent fma(x, log2(e), -round(max * log2(e))) kept the rounding residual
    of max * log2(e).  One logit at +1e30 gave a loss sum of -inf (the oracle's: 183.23), a float16 target logit at
    +65504 a gradient of up to 1.6e-3 where the oracle's is exactly 0, the float32 column at 1e4 +- 1 a two-kernel
    loss 1.2e-5 off (test_losses_hold_finite_extremes, 44 cases).  The kernels take (x - max) first now, and the
    two-kernel path saves the maximum and log2 of the sum as two planes.
"""
import math

import numpy as np
import pytest
import torch

from nicr_mt_scene_analysis_amd.testing import nonfinite as NF
from nicr_mt_scene_analysis_amd.testing import nonfinite_losses as NL

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CASES = NL.all_cases()
EXTREMES = NL.extreme_cases()


def _F():
    from nicr_mt_scene_analysis_amd.loss import _functional as F_
    return F_


def _scale(count_dev, case, n):
    scale = _F().expected_scale(count_dev, case.w_up)
    assert float(scale) == NL.upstream(case.w_up, n), 'the oracle and the device divide by the same float32 factor'
    return scale


def _multi_single(case, x, item):
    """one item through `multi_loss` with a fresh record: the forward launch writes the gradient for 1 / n and
    the backward launch confirms it"""
    from nicr_mt_scene_analysis_amd.loss import _multi
    item = dict(item, pred=x, total=0)
    assert _multi.supported([item]), case.id
    spec = _multi.SpecState(1, case.w_up)
    res = _multi.multi_loss([item], 1, spec)
    (case.w_up * res.total_losses[0]).backward()
    # (the focal loss's divisor is the number of peaks, no count of mask bytes: it has no expectation, the
    # forward launch writes no gradient and the backward launch computes it)
    want = {'confirmed': 0, 'recomputed': 1} if case.kind == 'focal' else {'confirmed': 1, 'recomputed': 0}
    assert spec.stats() == want, (case.id, spec.stats())
    assert all(math.isfinite(w) for w in spec.weights(DEV)), case.id
    return {'loss': res.sums[0].detach(), 'count': int(res.counts[0]), 'grad': x.grad}


def _explicit(case, x, n_dev, n, call, inspect=None):
    """`call(expected_scale | None)` -> (loss, count) through an autograd Function of loss/_functional.py, with or
    without an expectation; the speculation tally says which launch wrote the gradient"""
    F_ = _F()
    scale = _scale(n_dev, case, n)
    before = F_.speculation_stats()
    loss, count = call(scale if case.path == 'expect' else None)
    assert int(count) == n, case.id
    if case.path == 'forward':
        assert loss.grad_fn is None
        return {'loss': loss.detach(), 'count': int(count), 'grad': None}
    if inspect is not None:
        inspect(loss.grad_fn)
    grad, = torch.autograd.grad(loss, x, scale[0])
    after = F_.speculation_stats()
    delta = (after['confirmed'] - before['confirmed'], after['recomputed'] - before['recomputed'])
    assert delta == ((1, 0) if case.path == 'expect' else (0, 0)), (case.id, delta)
    return {'loss': loss.detach(), 'count': int(count), 'grad': grad}


def device_fn(case, inp):
    F_ = _F()
    assert F_.speculation_enabled()
    kind, path = case.kind, case.path
    x = inp['x'].to(DEV).requires_grad_(path != 'forward')
    n = case.count(inp)
    if kind == 'ce':
        C, ls = case.info['C'], case.info['ls']
        t, w = inp['t'].to(DEV), inp['w'].to(DEV)
        assert t.dtype == (torch.int16 if C > 255 else torch.uint8)
        if path == 'multi':
            return _multi_single(case, x, {'kind': 'ce', 'mask': t, 'weights': w, 'param': ls})
        assert path != 'expect' or F_.ce_forward_can_write_gradient(x)
        n_dev = F_.count_u8(t, 1, C) if C <= 255 else (t != 0).sum()
        def saved(fn):
            # the labels as they travelled (uint8; int16 above 255 classes) and the saved log-sum-exp
            assert fn.saved_tensors[1].dtype == t.dtype
            assert tuple(fn.saved_tensors[3].shape) == ((2,) + tuple(t.shape) if path == 'two-kernel' else (0,))
        return _explicit(case, x, n_dev, n, lambda e: F_.cross_entropy_sum(x, t, w, ls, expected_scale=e)[:2], saved)
    if kind == 'cos':
        from nicr_mt_scene_analysis_amd.loss import CosineEmbeddingLoss, _multi
        idx, lut = inp['idx'].to(DEV), inp['lut'].to(DEV)
        assert _multi.cos_supported(x, lut) == (path != 'two-walk'), case.id
        before = F_.speculation_stats()
        loss, count = CosineEmbeddingLoss().lut_sum(x, idx, lut)
        (loss / count).backward()
        after = F_.speculation_stats()
        delta = (after['confirmed'] - before['confirmed'], after['recomputed'] - before['recomputed'])
        assert delta == ((0, 0) if path == 'two-walk' else (1, 0)), (case.id, delta)
        return {'loss': loss.detach(), 'count': int(count), 'grad': x.grad}
    y, m = inp['y'].to(DEV), inp['m'].to(DEV)
    if path == 'multi':
        return _multi_single(case, x, {'kind': kind, 'target': y, 'mask': m, 'param': case.info.get('kappa', 0.0)})
    if kind == 'focal':
        from nicr_mt_scene_analysis_amd.loss import CenterFocalLoss
        n_dev = ((y == 1) & m).sum().clamp(min=1)
        return _explicit(case, x, n_dev, n, lambda e: CenterFocalLoss().masked_sum(x, y, m))
    n_dev = F_.count_u8(m)
    if kind == 'vonmises':
        return _explicit(case, x, n_dev, n, lambda e: F_.vonmises_sum(x, y, m, case.info['kappa'], expected_scale=e))
    return _explicit(case, x, n_dev, n, lambda e: F_.masked_elementwise_sum(x, y, m, kind, expected_scale=e))


@pytest.fixture(autouse=True)
def _no_status_left():
    from nicr_mt_scene_analysis_amd.loss import check_loss_status
    check_loss_status()
    yield
    check_loss_status()                         # no label / index went out of range, no cosine call fell back


@pytest.mark.parametrize('dtype', NF.DTYPES, ids=str)
@pytest.mark.parametrize('case', CASES, ids=repr)
def test_losses_answer_a_poison_as_the_oracle_does(case, dtype):
    assert NL.run(case, dtype, device_fn) == len(case.places(case.make(dtype))) * len(NF.POISONS)


EXTREME_RUNS = [(case, dtype, k) for case in EXTREMES for dtype in NF.DTYPES for k in range(len(NL.extremes(case, dtype)))]


@pytest.mark.parametrize('case,dtype,k', EXTREME_RUNS,
                         ids=[f'{c.id}-{d}-{NL.extremes(c, d)[k][0]}'.replace(' ', '_') for c, d, k in EXTREME_RUNS])
def test_losses_hold_finite_extremes(case, dtype, k):
    assert NL.run_extremes(case, dtype, device_fn, only=k) == 1


# ------------------------------------------------------------------------------------------ the forms
def _form_device(case, inp):
    F_ = _F()
    x, y, up = inp['x'].to(DEV).requires_grad_(True), inp['y'].to(DEV), inp['up'].to(DEV)
    if case.kind in ('mse', 'l1'):
        out = F_.elementwise_none(x, y, case.kind)
    elif case.kind == 'vonmises':
        out = F_.vonmises_rows(x, y, case.info['kappa'])
    else:
        out = F_.cosine_embedding_rows(x, y, inp['labels'].to(DEV) if case.kind == 'cos-labelled' else None)
    assert out.dtype == torch.float32
    grad, = torch.autograd.grad(out, x, up)
    return {'out': out.detach().cpu(), 'grad': grad.cpu()}


@pytest.mark.parametrize('dtype', NF.DTYPES, ids=str)
@pytest.mark.parametrize('case', NL.form_cases(), ids=repr)
def test_forms_answer_a_poisoned_row_as_the_oracle_does(case, dtype):
    assert NL.run_form(case, dtype, _form_device) == len(NL.FORM_ROWS) * len(NF.POISONS)


# ------------------------------------------------------------------------------------------ scene step
def _ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def _scene_device(inp, eps):
    from nicr_mt_scene_analysis_amd import ops
    C = inp['x'].shape[1]
    cm = torch.zeros((C, C), dtype=torch.int64, device=DEV)
    r = ops.scene_step(inp['x'].to(DEV), inp['labels'].to(DEV), inp['w'].to(DEV), eps,
                       want=('score', 'idx', 'loss', 'grad'), confmat=cm)
    assert int(r['status'].item()) == 0
    return {k: v.cpu() for k, v in r.items()} | {'cm': cm.cpu()}


def _scene_compare(got, got_clean, want, want_clean, row, dtype, tag):
    assert torch.equal(got['idx'], want['idx']), (tag, 'idx', got['idx'].tolist(), want['idx'].tolist())
    assert torch.equal(got['cm'], want['cm']), (tag, 'confusion matrix')
    assert torch.equal(NF.classify(got['score']), NF.classify(want['score'])), (tag, 'score class')
    others = torch.arange(NL.SCENE_B) != row
    assert torch.equal(got['score'][others], got_clean['score'][others]), (tag, 'the score of another row moved')
    if bool(torch.isfinite(want['score'][row])):
        assert abs(float(got['score'][row]) - float(want['score'][row])) <= _ulp32(float(want['score'][row])), tag
    # numerator, divisor, loss: the divisor comes from the labels alone
    assert torch.equal(got['loss'][1], got_clean['loss'][1]), (tag, 'divisor')
    assert int(NF.classify(got['loss'][2])) == int(NF.classify(want['loss'])), (tag, 'loss class', float(got['loss'][2]))
    assert int(NF.classify(got['loss'][0])) == int(NF.classify(want['loss'])), (tag, 'numerator class')
    if bool(torch.isfinite(want['loss'])):
        assert abs(float(got['loss'][2]) - float(want['loss'])) <= 2 * _ulp32(float(want['loss'])), (tag, 'loss')
    mask = NF.touched(want_clean['grad'], want['grad'])
    NF.assert_class(got['grad'], want['grad'].to(dtype).double(), mask, False, tag)
    NF.assert_contained(got['grad'], got_clean['grad'], mask, tag)
    gmax = float(want_clean['grad'].abs().max())
    NF.assert_touched_finite(got['grad'], want['grad'], mask, NL.grad_rtol(dtype) * gmax * 0.05, tag)


@pytest.mark.parametrize('dtype', NF.DTYPES, ids=str)
@pytest.mark.parametrize('eps', (0.0, 0.1))
@pytest.mark.parametrize('C', NL.SCENE_CLASSES)
def test_scene_step_answers_a_poison_as_the_oracle_does(C, eps, dtype):
    clean = NL.scene_inputs(C, dtype)
    want_clean, got_clean = NL.scene_oracle(clean, eps), _scene_device(clean, eps)
    _scene_compare(got_clean, got_clean, want_clean, want_clean, 0, dtype, (C, eps, 'clean'))
    for label, r, c, counted in NL.scene_places(C):
        for pname, value in NF.POISONS.items():
            inp = dict(clean)
            inp['x'] = clean['x'].clone()
            inp['x'][r, c] = value
            _scene_compare(_scene_device(inp, eps), got_clean, NL.scene_oracle(inp, eps), want_clean, r, dtype,
                           (C, eps, str(dtype), label, pname))
    for r in (0, NL.SCENE_VOID_ROWS[0]):
        inp = NL.scene_all_neg_inf(clean, r)
        want = NL.scene_oracle(inp, eps)
        assert int(want['idx'][r]) == 0 and bool(torch.isnan(want['score'][r]))
        _scene_compare(_scene_device(inp, eps), got_clean, want, want_clean, r, dtype, (C, eps, str(dtype), 'all -inf', r))


# ------------------------------------------------------------------------------------------ multi-loss
def _two_totals(dtype, poison=None):
    """total 0: cross entropy (C = 40) + MSE; total 1: L1 + von Mises.  `poison`: at the first pixel of total 0's
    cross entropy"""
    hw = NL.SHAPES[0]
    ce = NL._ce_make(40, hw, 700, False)(dtype)
    mse = NL._elem_make('mse', 1, hw, 701)(dtype)
    l1 = NL._elem_make('l1', 2, hw, 702)(dtype)
    vm = NL._vm_make(hw, 703)(dtype)
    if poison is not None:
        ce['x'].view(-1)[NL._flat(ce['x'], 0, NL.CE_T, 0)] = poison
    xs = [d['x'].to(DEV).requires_grad_(True) for d in (ce, mse, l1, vm)]
    items = [{'kind': 'ce', 'pred': xs[0], 'mask': ce['t'].to(DEV), 'weights': ce['w'].to(DEV), 'param': 0.1, 'total': 0},
             {'kind': 'mse', 'pred': xs[1], 'target': mse['y'].to(DEV), 'mask': mse['m'].to(DEV), 'total': 0},
             {'kind': 'l1', 'pred': xs[2], 'target': l1['y'].to(DEV), 'mask': l1['m'].to(DEV), 'total': 1},
             {'kind': 'vonmises', 'pred': xs[3], 'target': vm['y'].to(DEV), 'mask': vm['m'].to(DEV), 'param': 1.0, 'total': 1}]
    return xs, items


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _step(spec, dtype, poison, factors):
    from nicr_mt_scene_analysis_amd.loss import _multi
    xs, items = _two_totals(dtype, poison)
    assert _multi.supported(items)
    res = _multi.multi_loss(items, 2, spec)
    sum(f * t for f, t in zip(factors, res.total_losses)).backward()
    return res, [x.grad for x in xs]


@pytest.mark.parametrize('poison', tuple(NF.POISONS))
@pytest.mark.parametrize('dtype', NF.DTYPES, ids=str)
def test_multi_loss_keeps_a_poison_of_one_total_out_of_the_other(dtype, poison):
    from nicr_mt_scene_analysis_amd.loss import _multi
    clean, clean_grads = _step(_multi.SpecState(2), dtype, None, (1.0, 1.0))
    res, grads = _step(_multi.SpecState(2), dtype, NF.POISONS[poison], (1.0, 1.0))
    assert not bool(torch.isfinite(res.sums[0])) and not bool(torch.isfinite(res.total_losses[0]))
    # (a -inf target logit: an infinite loss, and the finite gradient of a probability of 0)
    assert bool(torch.isfinite(grads[0]).all()) == (poison == '-inf')
    assert torch.equal(_bits(res.sums[1]), _bits(clean.sums[1])) and torch.equal(_bits(grads[1]), _bits(clean_grads[1]))
    for i in (2, 3):                            # total 1: every sum, item loss and gradient
        assert torch.equal(_bits(res.sums[i]), _bits(clean.sums[i])), i
        assert torch.equal(_bits(res.item_losses[i]), _bits(clean.item_losses[i])), i
        assert torch.equal(_bits(grads[i]), _bits(clean_grads[i])), i
    assert torch.equal(_bits(res.total_losses[1]), _bits(clean.total_losses[1]))
    assert torch.equal(res.counts.cpu(), clean.counts.cpu())
    assert torch.equal(_bits(res.divisors), _bits(clean.divisors))


@pytest.mark.parametrize('poison', tuple(NF.POISONS))
def test_spec_state_after_a_poisoned_step(poison):
    """clean steps until the factor is confirmed, one poisoned step, clean steps again under the factor a scaler
    would lower to: the records hold no NaN or infinity, the clean steps answer as a fresh state does and
    confirmations resume"""
    from nicr_mt_scene_analysis_amd.loss import _multi
    dtype, spec = NF.F16, _multi.SpecState(2)
    for _ in range(3):
        _step(spec, dtype, None, (4.0, 4.0))
    confirmed = spec.stats()['confirmed']
    assert confirmed >= 2 and spec.weights(DEV) == [4.0, 4.0]
    res, grads = _step(spec, dtype, NF.POISONS[poison], (4.0, 4.0))
    assert not bool(torch.isfinite(res.total_losses[0]))
    assert bool(torch.isfinite(grads[0]).all()) == (poison == '-inf')
    assert all(bool(torch.isfinite(g).all()) for g in grads[1:])
    assert spec.weights(DEV) == [4.0, 4.0]
    assert bool(torch.isfinite(spec.records(DEV).view(torch.float32)[:2, 2]).all())
    fresh = _multi.SpecState(2)
    for k in range(3):
        before = spec.stats()['confirmed']
        a, ga = _step(spec, dtype, None, (2.0, 2.0))
        b, gb = _step(fresh, dtype, None, (2.0, 2.0))
        assert torch.equal(_bits(a.packed), _bits(b.packed)), k
        for u, v in zip(ga, gb):
            assert bool(torch.isfinite(u).all()) and torch.equal(_bits(u), _bits(v)), k
        if k > 0:
            assert spec.stats()['confirmed'] == before + 2, (k, spec.stats())
    assert spec.weights(DEV) == [2.0, 2.0]


@pytest.mark.parametrize('poison', (None,) + tuple(NF.POISONS), ids=str)
def test_grad_scaler_skips_the_step_behind_a_poisoned_loss(poison):
    """the semantic task helper under torch.amp.GradScaler.  The poison is put into the LOGITS (the target class of a
    counted pixel), behind the 1x1 head, so the head's gradients are non-finite only if the loss kernel's gradient
    is: NaN and +inf give a NaN loss and non-finite weight and bias gradients, the scaler skips the step and halves
    its scale.  A -inf target logit gives, as F.cross_entropy does, a loss of +inf and the finite gradient of a
    probability of 0: nothing for the scaler to skip.  The steps after it answer as a helper that never saw the poison"""
    from nicr_mt_scene_analysis_amd.task_helper import SemanticTaskHelper
    C, hw = 5, NL.SHAPES[1]
    data = NL._ce_make(C, hw, 710, False)(NF.F16)
    batch = {'semantic': data['t'].to(DEV)}
    torch.manual_seed(711)
    head = torch.nn.Conv2d(C, C, 1).to(DEV)

    def helper():
        h = SemanticTaskHelper(n_classes=C, disable_multiscale_supervision=True)
        h.initialize(torch.device(DEV))
        return h

    def step(h, x, scaler, poison=None):
        head.zero_grad()
        with torch.autocast('cuda', dtype=NF.F16):
            logits = head(x)
        assert logits.dtype == NF.F16
        if poison is not None:
            bump = torch.zeros_like(logits)
            bump[0, NL.CE_T, 0, 0] = NF.POISONS[poison]             # 0 + NaN, x + inf: the logit itself is the poison
            logits = logits + bump
        losses, _ = h.training_step(batch, 0, {'semantic_output': logits})
        scaler.scale(losses['semantic_total_loss']).backward()
        return losses['semantic_total_loss'].detach(), [p.grad.clone() for p in head.parameters()]

    h, opt = helper(), torch.optim.SGD(head.parameters(), lr=0.0)          # (lr 0: every step sees the same head)
    scaler = torch.amp.GradScaler('cuda', init_scale=4.0, growth_interval=1000)
    x = data['x'].float().to(DEV)
    for _ in range(3):
        loss, grads = step(h, x, scaler)
        scaler.step(opt)
        scaler.update()
    spec = h.spec_state(('semantic',))
    assert scaler.get_scale() == 4.0 and spec.stats()['confirmed'] >= 2 and spec.weights(DEV) == [4.0]
    assert int(data['t'][0, 0, 0]) == NL.CE_T + 1                   # the poisoned logit is the target of a counted pixel
    loss, grads = step(h, x, scaler, poison)
    skipped = poison in ('nan', '+inf')
    want_class = {None: NF.FINITE, 'nan': NF.NAN, '+inf': NF.NAN, '-inf': NF.POS_INF}[poison]
    assert int(NF.classify(loss)) == want_class, (poison, float(loss))
    weight_grad, bias_grad = grads
    assert bias_grad.shape == (C,) and bool(torch.isfinite(bias_grad).all()) == (not skipped)   # = sum of the loss's gradient
    assert bool(torch.isfinite(weight_grad).all()) == (not skipped)
    scaler.step(opt)
    scaler.update()
    assert scaler.get_scale() == (2.0 if skipped else 4.0)
    assert all(math.isfinite(w) for w in spec.weights(DEV))
    fresh, fresh_scaler = helper(), torch.amp.GradScaler('cuda', init_scale=scaler.get_scale(), growth_interval=1000)
    for k in range(3):
        before = spec.stats()['confirmed']
        la, ga = step(h, x, scaler)
        lb, gb = step(fresh, x, fresh_scaler)
        assert bool(torch.isfinite(la)) and torch.equal(_bits(la), _bits(lb)), k
        for u, v in zip(ga, gb):
            assert bool(torch.isfinite(u).all()) and torch.equal(_bits(u), _bits(v)), k
        scaler.step(opt)
        scaler.update()
        if k > 0:
            assert spec.stats()['confirmed'] == before + 1, (k, spec.stats())
    assert spec.weights(DEV) == [scaler.get_scale()]
