"""`DenseVisualEmbeddingPostprocessing` and `ops.dve_project` (reference
model/postprocessing/dense_visual_embedding.py) against tests/golden/dve_postprocess.npz
(tools/gen_golden_dve_post.py: the reference's own module on CPU).

Bounds (none of them measured on the code under test):
  ceiling    any summation order of D float32 products of two unit vectors errs by at most
             gamma_D ||x^|| ||w||, so |logit - truth64| <= (D + 4) 2^-24 ||w_c||; the same argument
             on the sum of squares bounds the normalised channels RELATIVE to |x / ||x||_64|
  quality    max abs error <= 4 x the reference's own error against the float64 truth (`e_ref`,
             `e_norm_ref` of the fixture): a strictly sequential float32 sum is up to 2 x the
             reference's blocked sum, the other factor 2 is headroom
  class maps identical to the reference's wherever the float64 top-2 gap exceeds 2 x ceiling; the
             share of pixels below that is capped at 1 % per case, at the network resolution and
             after the crop / resize alike (for the full-resolution map the gap is taken on the
             float64 logits put through the same crop and bilinear resize)
  scores     rtol 1e-5 / atol 1e-7, as tests/test_fullres.py and tests/test_hip_parity.py
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _golden import load, jload
from nicr_mt_scene_analysis_amd.testing import synthetic as syn

TEXT = 'dense_visual_embedding_text_based_'
VISUAL = 'dense_visual_embedding_visual_mean_based_'
HEADS = (('a', TEXT), ('b', VISUAL))
CASES = ('clean', 'noise', 'wide', 'odd')


def _case(name):
    """regenerated inputs (digest-checked: a mismatch FAILS), recipe, fixture"""
    g = load('dve_postprocess')
    p = jload(g[f'{name}__params'])
    inp = syn.make_dve_post_inputs(p['recipe'], p['seed'])
    assert syn.input_digest(*(inp[k] for k in sorted(inp))) == p['digest'], \
        f'{name}: regenerated inputs differ from the fixture generator\'s'
    return inp, syn.DVE_POST_RECIPES[name], g


def _heads(inp):
    return [(h, pfx, inp['weight_' + h]) for h, pfx in HEADS if 'weight_' + h in inp]


def _truth64(emb, w):
    x = torch.from_numpy(emb).double()
    xn = x / x.norm(dim=1, keepdim=True)
    return xn, torch.einsum('bdhw,cd->bchw', xn, torch.from_numpy(w).double())


def _ceiling(w, D):
    """per class: (D + 4) 2^-24 ||w_c||"""
    return (D + 4) * 2.0 ** -24 * np.linalg.norm(w.astype(np.float64), axis=1)


def _fullres(logits, crop, full):
    x = logits[..., crop[0]:crop[1], crop[2]:crop[3]]
    if tuple(x.shape[-2:]) != tuple(full):
        x = F.interpolate(x, size=full, mode='bilinear', align_corners=False)
    return x


def _gap(l64):
    top = torch.topk(torch.nan_to_num(l64), 2, dim=1).values
    return top[:, 0] - top[:, 1]


def _batch(recipe, inp, device='cpu'):
    from nicr_mt_scene_analysis_amd.data.preprocessing import APPLIED_PREPROCESSING_KEY
    B, crop = recipe[0], recipe[6]
    return {'semantic_fullres': torch.from_numpy(inp['semantic_fullres']).to(device),
            APPLIED_PREPROCESSING_KEY: [[{'type': 'Resize',
                                          'valid_region_slice_y': slice(crop[0], crop[1]),
                                          'valid_region_slice_x': slice(crop[2], crop[3])}]] * B}


def _post(inp, device='cpu'):
    from nicr_mt_scene_analysis_amd.model.postprocessing import get_postprocessing_class
    wb = inp.get('weight_b')
    return get_postprocessing_class('dense-visual-embedding')(
        with_text_embeddings_per_class=True,
        text_embeddings_per_class=torch.from_numpy(inp['weight_a']).to(device),
        with_mean_visual_embedding_per_class=wb is not None,
        mean_visual_embedding_per_class=None if wb is None else torch.from_numpy(wb).to(device))


# ------------------------------------------------------------------------------------ CPU tier
def test_factory_returns_the_class():
    from nicr_mt_scene_analysis_amd.model.postprocessing import (
        DenseVisualEmbeddingPostprocessing, get_postprocessing_class)
    assert get_postprocessing_class('dense-visual-embedding') is DenseVisualEmbeddingPostprocessing
    cls = get_postprocessing_class('dense-visual-embedding', with_text_embeddings_per_class=True,
                                   text_embeddings_per_class=torch.ones(3, 8))
    assert issubclass(cls, DenseVisualEmbeddingPostprocessing)
    assert cls().with_semantic_text_embeddings
    for name in ('normal', 'scene'):
        with pytest.raises(NotImplementedError):
            get_postprocessing_class(name)


def test_training_pass_through_on_cpu_tensors():
    from nicr_mt_scene_analysis_amd.model.postprocessing import DenseVisualEmbeddingPostprocessing
    out, side = torch.randn(1, 8, 4, 4), (torch.randn(1, 8, 2, 2),)
    before = out.clone()
    r = DenseVisualEmbeddingPostprocessing(
        with_text_embeddings_per_class=True, text_embeddings_per_class=torch.ones(3, 8)
    ).postprocess((out, side), {}, is_training=True)
    assert type(r) is dict and list(r) == ['dense_visual_embedding_output',
                                           'dense_visual_embedding_side_outputs']
    assert r['dense_visual_embedding_output'] is out and r['dense_visual_embedding_side_outputs'] is side
    assert torch.equal(out, before)


def test_constructor_asserts():
    from nicr_mt_scene_analysis_amd.model.postprocessing import DenseVisualEmbeddingPostprocessing
    with pytest.raises(AssertionError):
        DenseVisualEmbeddingPostprocessing(with_text_embeddings_per_class=True)
    with pytest.raises(AssertionError):
        DenseVisualEmbeddingPostprocessing(with_mean_visual_embedding_per_class=True)
    p = DenseVisualEmbeddingPostprocessing(text_embeddings_per_class=torch.ones(3, 8), unknown_kwarg=1)
    assert not p.with_semantic_text_embeddings and not p.with_mean_visual_embedding_per_class


def test_cpu_tensor_and_dtype_errors():
    from nicr_mt_scene_analysis_amd import ops
    from nicr_mt_scene_analysis_amd._lib import NmsaError
    with pytest.raises(NmsaError):
        ops.dve_project(torch.zeros(1, 8, 4, 4))
    with pytest.raises(TypeError):
        ops.dve_project(torch.zeros(1, 8, 4, 4, dtype=torch.float16))


@pytest.mark.parametrize('name', CASES)
def test_fixture_self_check(name):
    """the yardstick itself: the reference's logits lie within the ceiling of the float64 truth
    and at most 1 % of the pixels are too close to call"""
    inp, (B, D, H, W, Ca, Cb, crop, full), g = _case(name)
    sample = g[f'{name}__sample']
    for h, pfx, w in _heads(inp):
        st = jload(g[f'{name}__{h}__stats'])
        ceil = _ceiling(w, D)
        _, l64 = _truth64(inp['emb'], w)
        want = l64.permute(0, 2, 3, 1).reshape(-1, w.shape[0])[sample].numpy()
        got = g[f'{name}__{h}__logits_px']
        finite = np.isfinite(want)
        assert (np.isnan(got) == np.isnan(want)).all()
        assert (np.abs(got - want)[finite] <= np.broadcast_to(ceil, want.shape)[finite]).all()
        assert st['e_ref'] <= ceil.max() and 0 < st['e_norm_ref'] <= (D + 4) * 2.0 ** -24
        gap = _gap(l64)
        valid = torch.isfinite(l64).all(dim=1)
        excluded = float(((gap <= 2 * ceil.max()) & valid).sum()) / gap.numel()
        print(f'{name}/{h}: excluded {excluded:.5f} (fixture {st["excluded"]:.5f}), '
              f'fullres {st["excluded_fullres"]:.5f}, e_ref {st["e_ref"]:.3g}')
        assert abs(excluded - st['excluded']) < 1e-3        # float64 noise moves borderline pixels only
        assert excluded <= 0.01 and st['excluded_fullres'] <= 0.01
        if name == 'clean':
            assert excluded == 0.0


# ------------------------------------------------------------------------------------ GPU tier
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_against_truth(name, h, st, emb_in, w, xn_gpu, logits_gpu):
    """check (1): the ceiling, and 4 x the reference's own error"""
    D = emb_in.shape[1]
    xn64, l64 = _truth64(emb_in, w)
    ceil = torch.from_numpy(_ceiling(w, D)).view(1, -1, 1, 1)
    err = (logits_gpu.double() - l64).abs()
    finite = torch.isfinite(l64)
    assert (torch.isnan(logits_gpu) == ~finite).all()
    err_n = (xn_gpu.double() - xn64).abs()
    finite_n = torch.isfinite(xn64)
    assert (torch.isnan(xn_gpu) == ~finite_n).all()
    e, e_n = float(err[finite].max()), float(err_n[finite_n].max())
    print(f'{name}/{h}: logits max err {e:.3e} (reference {st["e_ref"]:.3e}), '
          f'normalised max err {e_n:.3e} (reference {st["e_norm_ref"]:.3e})')
    assert (err <= ceil)[finite].all()
    assert (err_n <= (D + 4) * 2.0 ** -24 * xn64.abs())[finite_n].all()
    assert e <= 4 * st['e_ref'] and e_n <= 4 * st['e_norm_ref']
    return l64


@pytest.mark.gpu
@pytest.mark.parametrize('generic', [False, True])
@pytest.mark.parametrize('name', CASES)
def test_ops_dve_project_vs_truth(name, generic):
    """checks (1), (5) and (6): both kernels on every case ('odd' only has the generic one)"""
    from nicr_mt_scene_analysis_amd import ops
    inp, recipe, g = _case(name)
    heads = _heads(inp)
    emb = _dev(inp['emb'])
    logits = ops.dve_project(emb, *[_dev(w) for _, _, w in heads], generic=generic)
    assert logits[len(heads):] == (None,) * (2 - len(heads))
    for (h, _, w), lg in zip(heads, logits):
        assert lg.dtype == torch.float32 and tuple(lg.shape) == (recipe[0], w.shape[0]) + emb.shape[2:]
        _check_against_truth(name, h, jload(g[f'{name}__{h}__stats']), inp['emb'], w, emb.cpu(), lg.cpu())
    if name == 'odd':
        lg = logits[0].cpu()
        assert torch.isnan(lg[0, :, 7, 11]).all() and torch.isnan(lg[0, :, 20, 33]).all()
        assert torch.isnan(emb[0, :, 7, 11]).all() and torch.isnan(emb[0, 5, 20, 33])
        assert (emb[0, :5, 20, 33] == 0).all()


@pytest.mark.gpu
def test_ops_dve_project_strided_and_headless():
    from nicr_mt_scene_analysis_amd import ops
    x = torch.randn(2, 5, 7, 64, device='cuda')
    base = x.clone()
    view = x.permute(0, 2, 1, 3)                        # [2, 7, 5, 64], not contiguous: D = 7
    w = torch.randn(3, 7, device='cuda')
    lg, none = ops.dve_project(view, w)
    assert none is None
    ref = base.permute(0, 2, 1, 3).double()
    refn = ref / ref.norm(dim=1, keepdim=True)
    assert torch.allclose(view.double(), refn, rtol=0, atol=1e-6)        # caller's tensor
    assert torch.allclose(lg.double(), torch.einsum('bdhw,cd->bchw', refn, w.double()), rtol=0, atol=1e-5)
    y = torch.randn(1, 16, 4, 8, device='cuda')
    y0 = y.clone()
    assert ops.dve_project(y) == (None, None)
    assert torch.allclose(y, y0 / y0.norm(dim=1, keepdim=True), rtol=0, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_postprocess_vs_reference(name):
    """checks (1)-(5) through `postprocess`"""
    from nicr_mt_scene_analysis_amd.data.preprocessing.resize import get_fullres_key
    inp, (B, D, H, W, Ca, Cb, crop, full), g = _case(name)
    emb = _dev(inp['emb'])
    data = (emb, None)
    r = _post(inp, 'cuda').postprocess(data, _batch((B, D, H, W, Ca, Cb, crop, full), inp, 'cuda'),
                                       is_training=False)
    # (4) dict contract
    assert list(r.keys()) == jload(g[f'{name}__keys'])
    assert r['dense_visual_embedding_output'] is data[0]
    assert r['dense_visual_embedding_side_outputs'] is None
    for h, pfx, w in _heads(inp):
        st = jload(g[f'{name}__{h}__stats'])
        C = w.shape[0]
        logits = r[pfx + 'semantic_output']
        l64 = _check_against_truth(name, h, st, inp['emb'], w, emb.cpu(), logits.cpu())
        lc = logits.cpu()
        for sfx, lres in (('', lc), ('_fullres', _fullres(lc, crop, full))):
            idx, score = r[pfx + 'semantic_idx' + sfx], r[pfx + 'semantic_score' + sfx]
            sm, out = r[pfx + 'semantic_softmax_scores' + sfx], r[pfx + 'semantic_output' + sfx]
            assert idx.dtype == torch.int64 and all(t.dtype == torch.float32 for t in (score, sm, out))
            # (2) everything after the logits, from the GPU's own logits through torch CPU
            assert torch.equal(torch.nan_to_num(out.cpu(), nan=7.0), torch.nan_to_num(lres, nan=7.0))
            want_sm = F.softmax(lres, dim=1)
            want_score, want_idx = torch.max(want_sm, dim=1)
            assert torch.equal(idx.cpu(), want_idx), (name, h, sfx)
            np.testing.assert_allclose(score.cpu().numpy(), want_score.numpy(), rtol=1e-5, atol=1e-7,
                                       equal_nan=True)
            np.testing.assert_allclose(sm.cpu().numpy(), want_sm.numpy(), rtol=1e-5, atol=1e-7,
                                       equal_nan=True)
            if C <= 256:
                assert r.aux[pfx + 'semantic_idx' + sfx].dtype == torch.uint8
                assert torch.equal(r.aux[pfx + 'semantic_idx' + sfx].long(), idx)
            else:
                assert pfx + 'semantic_idx' + sfx not in r.aux
            # (3) class maps against the reference wherever float64 can tell the classes apart
            ref_idx = torch.from_numpy(g[f'{name}__{h}__idx{sfx}'].astype(np.int64))
            l64_res = l64 if not sfx else _fullres(l64, crop, full)
            sure = (_gap(l64_res) > 2 * st['ceiling']) & torch.isfinite(l64_res).all(dim=1)
            share = 1.0 - float(sure.sum()) / sure.numel()
            print(f'{name}/{h}{sfx}: {share:.5f} of the pixels excluded')
            assert share <= 0.01
            assert torch.equal(idx.cpu()[sure], ref_idx[sure]), (name, h, sfx)
            if name == 'clean':
                assert torch.equal(idx.cpu(), ref_idx), (name, h, sfx)
        sample = torch.from_numpy(g[f'{name}__sample'].astype(np.int64))
        # the reference's score: every logit within 2 x ceiling of the reference's, so every
        # softmax term within a factor exp(+-4 x ceiling)
        np.testing.assert_allclose(r[pfx + 'semantic_score'].cpu().reshape(-1)[sample].numpy(),
                                   g[f'{name}__{h}__score_px'], rtol=4 * st['ceiling'] + 1e-5, atol=1e-7,
                                   equal_nan=True)
        assert get_fullres_key(pfx + 'semantic_idx') in r


@pytest.mark.gpu
def test_both_heads_equal_two_single_head_calls():
    from nicr_mt_scene_analysis_amd import ops
    inp, recipe, _ = _case('clean')
    wa, wb = _dev(inp['weight_a']), _dev(inp['weight_b'])
    e2, ea, eb = (_dev(inp['emb']) for _ in range(3))
    la2, lb2 = ops.dve_project(e2, wa, wb)
    la, _ = ops.dve_project(ea, wa)
    _, lb = ops.dve_project(eb, None, wb)
    for a, b in ((la2, la), (lb2, lb), (e2, ea), (e2, eb)):
        assert torch.equal(a, b)
    # both heads off: the call still normalises in place and returns the two base keys
    from nicr_mt_scene_analysis_amd.model.postprocessing import DenseVisualEmbeddingPostprocessing
    e0 = _dev(inp['emb'])
    r = DenseVisualEmbeddingPostprocessing().postprocess((e0, None), _batch(recipe, inp, 'cuda'),
                                                         is_training=False)
    assert list(r) == ['dense_visual_embedding_output', 'dense_visual_embedding_side_outputs']
    assert r['dense_visual_embedding_output'] is e0
    xn64, _ = _truth64(inp['emb'], inp['weight_a'])
    e_norm_ref = jload(load('dve_postprocess')['clean__a__stats'])['e_norm_ref']
    assert float((e0.cpu().double() - xn64).abs().max()) <= 4 * e_norm_ref


def _clean_validation():
    """[(artifacts, logs)] of validation_step + validation_epoch_end on 'clean', from the LazyDict
    (uint8 maps) and from a plain dict with int64 maps"""
    from nicr_mt_scene_analysis_amd.task_helper import DenseVisualEmbeddingTaskHelper
    inp, recipe, g = _case('clean')
    B, D, H, W = recipe[:4]
    batch = _batch(recipe, inp, 'cuda')
    gen = torch.Generator().manual_seed(5)
    batch['dense_visual_embedding_lut'] = F.normalize(torch.randn((B, 3, D), generator=gen), dim=-1).cuda()
    batch['dense_visual_embedding_indices'] = torch.randint(0, 4, (B, H, W), generator=gen,
                                                            dtype=torch.int32).cuda()
    r = _post(inp, 'cuda').postprocess((_dev(inp['emb']), None), batch, is_training=False)
    plain = {k: r[k] for k in r.keys()}
    out = []
    for post in (r, plain):
        helper = DenseVisualEmbeddingTaskHelper(n_classes=recipe[4], disable_multiscale_supervision=True)
        helper.initialize(torch.device('cuda'))
        helper.validation_step(batch, 0, post)
        artifacts, _, logs = helper.validation_epoch_end()
        out.append((artifacts, logs))
    return g, out


@pytest.mark.gpu
def test_clean_validation_matches_reference_confusion_matrices():
    """check (3), 'clean': the DVE helper's confusion matrices equal the reference's exactly"""
    g, runs = _clean_validation()
    for artifacts, _ in runs:
        for h, pfx in HEADS:
            assert np.array_equal(artifacts[pfx + 'semantic_cm'].cpu().numpy(), g[f'clean__{h}__cm'])


@pytest.mark.gpu
def test_clean_validation_matches_reference_mious():
    """check (3), 'clean': the mIoUs equal the reference's exactly (`MeanIntersectionOverUnion.compute`
    does the reference's arithmetic on a host copy of the matrix: a float32 mean taken on the device
    was one ulp off, 0.9133874774 against 0.9133874178, with identical confusion matrices)"""
    g, runs = _clean_validation()
    for _, logs in runs:
        for h, pfx in HEADS:
            want = np.float32(jload(g[f'clean__{h}__stats'])['miou'])
            print(f'{h}: mIoU {float(logs[pfx + "miou"])!r} reference {float(want)!r}')
            assert float(logs[pfx + 'miou']) == want


@pytest.mark.gpu
def test_postprocess_does_not_synchronise():
    inp, recipe, _ = _case('noise')
    post, batch = _post(inp, 'cuda'), _batch(recipe, inp, 'cuda')
    post.postprocess((_dev(inp['emb']), None), batch, is_training=False)          # weights in place
    emb = _dev(inp['emb'])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        r = post.postprocess((emb, None), batch, is_training=False)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert r.aux[TEXT + 'semantic_idx_fullres'].dtype == torch.uint8


@pytest.mark.gpu
def test_embeddings_updated_in_place_are_picked_up():
    """the reference reads its class embeddings on every call: an in-place update between two
    inference calls (mean visual embeddings recomputed per epoch) must reach the next call"""
    from nicr_mt_scene_analysis_amd.model.postprocessing import DenseVisualEmbeddingPostprocessing
    inp, recipe, _ = _case('noise')
    for device in ('cpu', 'cuda'):
        w = torch.from_numpy(inp['weight_a'].copy()).to(device)
        post = DenseVisualEmbeddingPostprocessing(with_text_embeddings_per_class=True,
                                                  text_embeddings_per_class=w)
        batch = _batch(recipe, inp, 'cuda')
        first = post.postprocess((_dev(inp['emb']), None), batch, is_training=False)[TEXT + 'semantic_output']
        w.mul_(-1.0)
        second = post.postprocess((_dev(inp['emb']), None), batch, is_training=False)[TEXT + 'semantic_output']
        assert torch.equal(second, -first), device
