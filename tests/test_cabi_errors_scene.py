"""CPU tier: the host checks of nmsa_scene_step (csrc/scene.hip).  Every argument is checked
before anything is enqueued, so a bad call comes back as NMSA_ERR_ARG (-1) or
NMSA_ERR_UNSUPPORTED (-4) without a device: no broken call below reaches a HIP call, and the fake
addresses are never dereferenced.  That the unbroken call gets past the checks is shown by a call
that wants nothing: it returns NMSA_OK after the last check, before the launch."""
import ctypes as C

from nicr_mt_scene_analysis_amd import _lib as L

ARG, UNSUPPORTED = -1, -4
X, LAB, W, SCORE, IDX, LOSS, GRAD, CM, ST = (0x10000 * (i + 1) for i in range(9))
GOOD = dict(logits=X, logits_dtype=L.NMSA_F32, labels=LAB, label_dtype=L.NMSA_I64, B=32, C=45, weights=W,
            smoothing=0.1, score=SCORE, idx=IDX, loss=LOSS, grad=GRAD, confmat=CM, status=ST)


def rc(**changes):
    a = dict(GOOD, **changes)
    p = lambda v: C.c_void_p(v) if v else None                                 # noqa: E731
    return L.lib().nmsa_scene_step(p(a['logits']), a['logits_dtype'], p(a['labels']), a['label_dtype'], a['B'],
                                   a['C'], p(a['weights']), a['smoothing'], p(a['score']), p(a['idx']),
                                   p(a['loss']), p(a['grad']), p(a['confmat']), p(a['status']), None)


def test_symbol_is_declared_and_exported():
    assert 'nmsa_scene_step' in L.declared_symbols() and 'nmsa_scene_step' in L._SIGNATURES
    assert hasattr(C.CDLL(L.LIB_PATH), 'nmsa_scene_step')
    assert len(L._SIGNATURES['nmsa_scene_step'][1]) == 15


def test_the_unbroken_arguments_pass_the_checks():
    """the arguments every other test breaks in one place, with no output wanted: NMSA_OK comes
    from behind the last check and nothing is launched (no device needed, none touched)"""
    nothing = dict(score=0, idx=0, loss=0, grad=0, confmat=0, status=0)
    assert rc(**nothing) == 0
    assert rc(labels=0, **nothing) == 0                                         # the postprocessing's inputs


def test_null_logits_and_sizes():
    assert rc(logits=0) == ARG
    assert rc(B=0) == ARG and rc(B=-1) == ARG
    assert rc(C=0) == ARG and rc(C=-3) == ARG and rc(C=4097) == ARG


def test_label_smoothing_range():
    for bad in (-0.001, 1.001, float('nan'), float('inf'), -float('inf')):
        assert rc(smoothing=bad) == ARG, bad


def test_dtypes():
    for bad in (3, -1, 7):
        assert rc(logits_dtype=bad) == UNSUPPORTED, bad
    for bad in (L.NMSA_I16, 4, -1):
        assert rc(label_dtype=bad) == UNSUPPORTED, bad
    # the label dtype is read with labels only (no output wanted: NMSA_OK, nothing is launched)
    assert rc(label_dtype=L.NMSA_I16, labels=0, score=0, idx=0, loss=0, grad=0, confmat=0, status=0) == 0


def test_outputs_that_need_labels():
    only = dict(labels=0, loss=0, grad=0, confmat=0)
    for name in ('loss', 'grad', 'confmat'):
        assert rc(**dict(only, **{name: GOOD[name]})) == ARG, name


def test_the_checks_hold_when_nothing_is_wanted():
    nothing = dict(score=0, idx=0, loss=0, grad=0, confmat=0, status=0)
    assert rc(logits=0, **nothing) == ARG and rc(C=4097, **nothing) == ARG
    assert rc(smoothing=2.0, **nothing) == ARG and rc(logits_dtype=5, **nothing) == UNSUPPORTED
