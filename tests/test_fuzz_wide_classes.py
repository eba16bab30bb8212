"""
GPU tier (pytest -m gpu): randomised parity of the HIP path at 49..256 semantic classes, where the
kernels take code paths of their own: the thing LUT in four 64-bit ballot words (k_panoptic_fused),
the [256 x NC] vote table staged through LDS in several passes of whole rows (k_assign), the
two-pass softmax above 48 classes, the confusion matrix outside the fused PQ pass above 64
classes and the parts path's 255-entry LUT, the LDS ring of the resized argmax.  Class counts are
drawn with a bias toward the word and pass edges.  Integer outputs are compared bit for bit with
the C oracle (itself pinned to the reference by tests/test_oracle_vs_golden.py), probabilities
with a float64 softmax.
"""
import numpy as np
import pytest
import torch

from _golden import ids_from_arrays
from nicr_mt_scene_analysis_amd.testing import synthetic as syn
from test_fuzz_parity import _DERANDOMIZE, _n, check_argmax_probability_ties, check_pipeline, dev

pytestmark = pytest.mark.gpu

hypothesis = pytest.importorskip('hypothesis')
from hypothesis import example, given, settings, strategies as st, HealthCheck   # noqa: E402

EDGE_CLASSES = (49, 63, 64, 65, 127, 128, 129, 143, 144, 145, 150, 191, 192, 193, 255, 256)
# rows of the vote table per LDS pass of k_assign: ASSIGN_LDS_WORDS (csrc/panoptic.hip) // columns
ASSIGN_LDS_WORDS = 36 * 1024

_EFFECTIVE = {}


def _count(name, k=1):
    _EFFECTIVE[name] = _EFFECTIVE.get(name, 0) + int(k)


def rows_per_pass(n_cols):
    return max(1, min(256, ASSIGN_LDS_WORDS // n_cols))


def classes(lo=49, hi=256, ragged=False):
    """edge class counts or a uniform draw in between; `ragged`: only counts that leave a
    partial last group of four classes"""
    edge = [c for c in EDGE_CLASSES if lo <= c <= hi and (not ragged or c % 4)]
    uni = st.integers(lo, hi)
    if ragged:
        uni = uni.filter(lambda c: c % 4 != 0)
    return st.one_of(st.sampled_from(edge), uni)


def settings_(examples, **kw):
    return settings(max_examples=_n(examples), deadline=None, derandomize=_DERANDOMIZE,
                    suppress_health_check=[HealthCheck.too_slow, HealthCheck.function_scoped_fixture,
                                           HealthCheck.data_too_large, HealthCheck.filter_too_much],
                    **kw)


def edge_ties(logits):
    """pixels whose maximum is shared by the two classes of a word edge (c - 1, c)"""
    x = np.asarray(logits, np.float64)
    m = x.max(axis=1)
    n = 0
    for e in syn.WORD_EDGES:
        if e < x.shape[1]:
            n += int(((x[:, e - 1] == m) & (x[:, e] == m) & np.isfinite(m)).sum())
    return n


# --------------------------------------------------------------------------------------- 1
@st.composite
def wide_cases(draw):
    C = draw(classes())
    regime = draw(st.sampled_from(['few', 'lds', 'late'] if C >= 144 else ['few', 'lds']))
    if regime == 'few':             # <= 64 centers: the lane-held center table
        n = draw(st.integers(0, 64))
        H = draw(st.integers(3, 24))
        W = draw(st.sampled_from([5, 13, 31, 32, 33, 47, 64]))
    elif regime == 'lds':           # 65..142: the LDS center table
        n = draw(st.integers(65, 142))
        H = draw(st.integers(20, 26))
        W = draw(st.sampled_from([32, 45, 61, 64]))
    else:                           # 143..255 peaks: votes in the second pass of k_assign
        n = draw(st.one_of(st.just(255), st.integers(143, 255)))
        H = draw(st.integers(20, 26))
        W = draw(st.sampled_from([61, 64, 96]))
    fewer = draw(st.sampled_from([0, 0, 0, 1, 9]))
    dtype = draw(st.sampled_from(['float32', 'bfloat16', 'float16']))
    return dict(C=C, B=draw(st.integers(1, 2)), H=H, W=W, n=n, seed=draw(st.integers(0, 2 ** 31 - 1)),
                levels=draw(st.sampled_from([2, 4, 6])), p_tie=draw(st.sampled_from([0.0, 0.3, 0.7])),
                p_thing=draw(st.sampled_from([0.2, 0.5, 0.9])), p_far=draw(st.sampled_from([0.0, 0.2])),
                specials=draw(st.sampled_from([False, False, False, True])), dtype=dtype,
                thr=0.1, ksize=3, topk=max(1, min(255, n - fewer)),
                apply_fg=draw(st.sampled_from([False, False, True])),
                dist_thr=draw(st.sampled_from([None, None, 0.5, 3.0])))


def make_wide_inputs(p):
    inp = syn.make_wide_class_inputs(p['B'], p['C'], p['H'], p['W'], p['n'], p['seed'],
                                     levels=p['levels'], p_tie=p['p_tie'], p_thing=p['p_thing'],
                                     p_far=p['p_far'])
    logits = inp['semantic_logits'].astype(np.float32)
    if p['specials']:           # non-finite logits: softmax-then-max semantics (index 0, NaN score)
        rng = np.random.default_rng(p['seed'] + 1)
        B, C, H, W = logits.shape
        for _ in range(int(rng.integers(1, 6))):
            logits[rng.integers(B), rng.integers(C), rng.integers(H), rng.integers(W)] = \
                rng.choice([np.nan, np.inf, -np.inf])
        if rng.random() < 0.5:  # a column of nothing but -inf
            logits[rng.integers(B), :, rng.integers(H), rng.integers(W)] = -np.inf
    return logits, inp['instance_center'], inp['instance_offset'], inp['semantic_classes_is_thing']


def count_pipeline(p, inputs, res):
    idx, fg = res['idx'], res['fg']
    _count('fg_class_ge64', (fg & (idx >= 64)).sum())
    _count('fg_class_ge192', (fg & (idx >= 192)).sum())
    _count('edge_ties', edge_ties(inputs[0]))
    _count('images_over_64_centers', (res['n'] > 64).sum())
    late = rows_per_pass(p['C'] + 1)
    _count('ids_in_later_pass', sum(sum(1 for i in d.values() if i >= late) for d in res['ids']))


@settings_(60)
@given(p=wide_cases())
@example(p=dict(C=256, B=2, H=24, W=64, n=255, seed=5, levels=2, p_tie=0.7, p_thing=0.9, p_far=0.0,
                specials=False, dtype='float32', thr=0.1, ksize=3, topk=255, apply_fg=False,
                dist_thr=None))
@example(p=dict(C=144, B=1, H=24, W=64, n=255, seed=6, levels=4, p_tie=0.3, p_thing=0.5, p_far=0.2,
                specials=True, dtype='bfloat16', thr=0.1, ksize=3, topk=255, apply_fg=False,
                dist_thr=None))
def test_fuzz_wide_pipeline_vs_oracle(oracle, p):
    """ops.panoptic_pipeline at 49..256 classes: thing sets on the word edges, maxima tied across
    them, <= 64 / 65..142 / 143..255 centers, every logits dtype, non-finite logits"""
    inputs = make_wide_inputs(p)
    res = check_pipeline(oracle, p, max_centers=256, inputs=inputs)
    assert res is not None, p           # isolated peaks: no tie at k, never more than 255 centers
    count_pipeline(p, inputs, res)


# --------------------------------------------------------------------------------------- 2
@settings_(40)
@given(seed=st.integers(0, 2 ** 31 - 1), C=classes(), B=st.integers(1, 2), H=st.integers(1, 9),
       W=st.sampled_from([1, 3, 7, 8, 32, 37, 64]), shift=st.booleans(),
       step=st.sampled_from([1.0, 0.37, 2.5]), dtype=st.sampled_from(['float32', 'bfloat16', 'float16']))
def test_fuzz_wide_argmax_and_softmax(oracle, seed, C, B, H, W, shift, step, dtype):
    """ops.semantic_argmax (u8 / i64 / score) against the oracle and ops.semantic_softmax against
    a float64 softmax, vector path (H*W % 4 == 0, aligned) and scalar paths (ragged H*W, a view
    whose base pointer is one element past an aligned allocation)"""
    from nicr_mt_scene_analysis_amd import ops
    inp = syn.make_wide_class_inputs(B, C, H, W, 0, seed)
    x = torch.from_numpy(inp['semantic_logits'].astype(np.float32) * np.float32(step))
    x = x.to(getattr(torch, dtype))
    xf = x.float().numpy()
    xd = x.cuda()
    if shift:
        buf = torch.zeros((x.numel() + 1,), dtype=x.dtype, device='cuda')
        xd = buf[1:].view(x.shape)
        xd.copy_(x.cuda())
        assert xd.data_ptr() % 16 != 0
    want, score = oracle.semantic_argmax(xf)
    r = ops.semantic_argmax(xd, want_u8=True, want_i64=True, want_score=True)
    r2 = ops.semantic_argmax(xd, want_u8=True, want_i64=False, want_score=False)
    probs = ops.semantic_softmax(xd)
    torch.cuda.synchronize()
    assert np.array_equal(r['idx'].cpu().numpy(), want)
    assert np.array_equal(r['idx_u8'].cpu().numpy(), want.astype(np.uint8))
    assert np.array_equal(r2['idx_u8'].cpu().numpy(), want.astype(np.uint8))
    np.testing.assert_allclose(r['score'].cpu().numpy(), score, rtol=1e-5, atol=1e-7)
    # fp32 exp and a running fp32 sum over up to 256 classes: a few ulps from the exact value
    ref = torch.softmax(torch.from_numpy(xf).double(), dim=1).numpy()
    np.testing.assert_allclose(probs.cpu().numpy(), ref, rtol=1e-5, atol=1e-8)
    _count('edge_ties', edge_ties(xf))


@settings_(15)
@given(seed=st.integers(0, 2 ** 31 - 1), C=classes(), scale=st.sampled_from([1.0, 0.5, 0.03, 1e-4]),
       spread=st.sampled_from([0.2, 2.0, 8.0, 40.0, 120.0]),
       dtype=st.sampled_from(['float32', 'float32', 'bfloat16', 'float16']))
def test_fuzz_wide_argmax_probability_ties(oracle, seed, C, scale, spread, dtype):
    """test_fuzz_parity's probability ties (maxima a few ulps apart, decided by ATen's fp32
    softmax) at 49..256 classes"""
    _count('probability_ties', check_argmax_probability_ties(oracle, seed, C, scale, spread, dtype))


# --------------------------------------------------------------------------------------- 3
@settings_(30)
@given(seed=st.integers(0, 2 ** 31 - 1), B=st.integers(1, 2),
       NC=st.sampled_from([145, 200, 257, 1000, 4096]),
       sem_dtype=st.sampled_from(['int64', 'int32', 'int16']), p_void=st.sampled_from([0.0, 0.1]),
       via_api=st.booleans())
@example(seed=1, B=2, NC=4096, sem_dtype='int64', p_void=0.0, via_api=False)   # 29 LDS passes
def test_fuzz_wide_standalone_merge_vs_oracle(oracle, seed, B, NC, sem_dtype, p_void, via_api):
    """nmsa_panoptic_merge with 145..4096 class values: every instance id 1..255 in the image,
    so that every LDS pass of k_assign holds rows, and two classes per instance (tied counts are
    common: the smaller class must win in every pass)"""
    from nicr_mt_scene_analysis_amd import ops
    from nicr_mt_scene_analysis_amd.utils.panoptic_merge import deeplab_merge_batch
    rng = np.random.default_rng(seed)
    H, W = 32, 64                                        # 256 blocks of 2 x 4 px
    ins = np.stack([np.kron(rng.permutation(256).reshape(16, 16), np.ones((2, 4), np.int64))
                    for _ in range(B)])
    pool = np.unique(np.concatenate([[1, 63, 64, 65, 127, 128, 255, 256, NC - 2, NC - 1],
                                     rng.integers(1, NC, 6)]))
    pool = pool[pool < NC]
    pair = rng.choice(pool, (B, 16, 16, 2))
    pick = rng.integers(0, 2, (B, H, W))
    sem = np.take_along_axis(np.repeat(np.repeat(pair, 2, 1), 4, 2), pick[..., None], -1)[..., 0]
    sem = np.where(rng.random((B, H, W)) < p_void, 0, sem).astype(np.int64)
    lut = (rng.random(NC) < 0.6).astype(np.uint8)
    lut[0] = 0
    thing_ids = np.where(lut)[0].tolist()
    thing_seg = (lut[sem] > 0) ^ (rng.random((B, H, W)) < 0.05)
    want_pan, want_ids = oracle.deeplab_merge(sem, ins, thing_seg, 1 << 16, thing_ids, 0)
    d_sem = dev(sem.astype(sem_dtype))
    if via_api:
        pan, got = deeplab_merge_batch(d_sem, dev(ins.astype(np.uint8)), dev(thing_seg), 1 << 16,
                                       thing_ids, 0, n_classes=NC)
        pan = pan.cpu().numpy()
    else:
        r = ops.panoptic_merge(d_sem, dev(ins.astype(np.uint8)), dev(thing_seg), dev(lut), 1 << 16, 0)
        torch.cuda.synchronize()
        pan = r['panoptic'].cpu().numpy()
        got = ids_from_arrays(r['n_ids'].cpu().numpy(), r['ids_pan'].cpu().numpy(),
                              r['ids_ins'].cpu().numpy())
    assert np.array_equal(pan, want_pan), (seed, NC)
    assert [list(d.items()) for d in got] == [list(d.items()) for d in want_ids], (seed, NC)
    late = rows_per_pass(NC)
    _count('ids_in_later_pass', sum(sum(1 for i in d.values() if i >= late) for d in want_ids))


# --------------------------------------------------------------------------------------- 4
def test_wide_vote_table_reuse(oracle):
    """the fused pipeline clears the vote table as k_assign reads it (ops._vote_table keeps it for
    the next call): back-to-back calls through the same cached table — many ids at C = 256, then
    few, then another class count and back — each must match the oracle"""
    from nicr_mt_scene_analysis_amd import ops
    B, H, W = 2, 24, 64
    seq = [(256, 255, 11), (256, 12, 12), (256, 200, 13), (150, 140, 14), (256, 30, 15),
           (144, 255, 16), (144, 5, 17), (256, 0, 18)]
    for C, n, seed in seq:
        p = dict(C=C, B=B, H=H, W=W, n=n, seed=seed, levels=2, p_tie=0.3, p_thing=0.9, p_far=0.0,
                 specials=False, dtype='float32', thr=0.1, ksize=3, topk=max(n, 1), apply_fg=False,
                 dist_thr=None)
        inputs = make_wide_inputs(p)
        res = check_pipeline(oracle, p, max_centers=256, inputs=inputs)
        assert res is not None and (res['n'] == n).all(), (C, n)
        count_pipeline(p, inputs, res)
    keys = [k for k in ops._VOTE_TABLES if k[1] == B and k[2] == 257]
    assert keys, 'the C = 256 table was not cached'


# --------------------------------------------------------------------------------------- 5
@settings_(25)
@given(p=wide_cases())
def test_fuzz_wide_scores_vs_oracle(oracle, p):
    """ops.panoptic_scores (score maps, per-instance mean semantic score) at 49..256 classes"""
    from nicr_mt_scene_analysis_amd import ops
    logits, heat, offset, is_thing = make_wide_inputs(p)
    logits = logits + np.random.default_rng(p['seed']).random(logits.shape).astype(np.float32)
    B, C, H, W = logits.shape
    x = dev(logits).to(getattr(torch, p['dtype']))
    r = ops.panoptic_pipeline(x, dev(heat), dev(offset), dev(is_thing), threshold=p['thr'],
                              kernel_size=p['ksize'], top_k=p['topk'],
                              apply_foreground_mask=p['apply_fg'], distance_threshold=p['dist_thr'],
                              want_score=True, want_panoptic_semantic=True, max_centers=256)
    assert int(r['n_centers'].max()) <= 255
    tab = torch.zeros((B, 256), dtype=torch.float32, device='cuda')
    tab[:, 1:] = r['center_scores'][:, :255]
    sc = ops.panoptic_scores(x, r['semantic_idx_u8'], r['semantic_score'], r['instance'],
                             r['panoptic'], r['pan_of_inst'], tab, 1 << 16)
    torch.cuda.synchronize()
    ids = ids_from_arrays(r['n_ids'].cpu().numpy(), r['ids_pan'].cpu().numpy(), r['ids_ins'].cpu().numpy())
    sem, ins, pns, mean = oracle.panoptic_scores(
        x.float().cpu().numpy(), r['panoptic_semantic'].cpu().numpy(), r['panoptic'].cpu().numpy(),
        ids, tab.cpu().numpy())
    np.testing.assert_allclose(sc['semantic_score'].cpu().numpy(), sem, rtol=2e-5, atol=1e-7, equal_nan=True)
    assert np.array_equal(sc['instance_score'].cpu().numpy(), ins)
    np.testing.assert_allclose(sc['panoptic_score'].cpu().numpy(), pns, rtol=2e-5, atol=1e-7, equal_nan=True)
    got_mean = sc['mean_semantic_score'].cpu().numpy()
    for b, d in enumerate(ids):
        for ins_id in d.values():
            g_, w_ = got_mean[b, ins_id], mean[b, ins_id]
            assert (np.isnan(g_) and np.isnan(w_)) or abs(g_ - w_) <= 2e-5 * abs(w_) + 1e-9
    _count('scores')


@settings_(30)
@given(seed=st.integers(0, 2 ** 31 - 1), C=classes(ragged=True), Hs=st.integers(1, 24),
       Ws=st.integers(1, 40), Ho=st.integers(1, 50), Wo=st.integers(1, 90), cropped=st.booleans(),
       dtype=st.sampled_from(['float32', 'bfloat16', 'float16']))
def test_fuzz_wide_argmax_resized_vs_oracle(oracle, seed, C, Hs, Ws, Ho, Wo, cropped, dtype):
    """ops.semantic_argmax_resized (crop + bilinear + argmax through an LDS ring of class groups)
    at class counts with a partial last group, against the oracle's resize followed by argmax"""
    from nicr_mt_scene_analysis_amd import ops
    rng = np.random.default_rng(seed)
    crop = None
    if cropped:
        y0, x0 = int(rng.integers(0, Hs)), int(rng.integers(0, Ws))
        crop = (slice(y0, int(rng.integers(y0 + 1, Hs + 1))), slice(x0, int(rng.integers(x0 + 1, Ws + 1))))
    inp = syn.make_wide_class_inputs(1, C, Hs, Ws, 0, seed)
    x = torch.from_numpy(inp['semantic_logits'].astype(np.float32) * np.float32(0.37))
    x = x.to(getattr(torch, dtype))
    want = oracle.resize_bilinear(x.float().numpy(), (Ho, Wo), crop)
    # the reference's interpolate returns the storage dtype: round like it
    want = torch.from_numpy(want).to(x.dtype).float().numpy()
    want_idx, want_score = oracle.semantic_argmax(want)
    r = ops.semantic_argmax_resized(x.cuda(), (Ho, Wo), crop, want_u8=True)
    torch.cuda.synchronize()
    assert np.array_equal(r['idx'].cpu().numpy(), want_idx), (seed, C)
    assert np.array_equal(r['idx_u8'].cpu().numpy(), want_idx.astype(np.uint8)), (seed, C)
    np.testing.assert_allclose(r['score'].cpu().numpy(), want_score, rtol=1e-5, atol=1e-7)
    _count('resized')


# --------------------------------------------------------------------------------------- 6
@settings_(40)
@given(seed=st.integers(0, 2 ** 31 - 1), B=st.integers(1, 2), H=st.integers(3, 40),
       W=st.sampled_from([5, 16, 31, 64, 130]), C=st.one_of(st.sampled_from([60, 63, 64, 65, 127, 254, 255, 256]),
                                                          st.integers(60, 256)),
       n_seg=st.integers(4, 24))
@example(seed=2, B=2, H=32, W=64, C=256, n_seg=20)          # 257 categories: the int64 fallback
def test_fuzz_wide_metrics_vs_oracle(oracle, seed, B, H, W, C, n_seg):
    """PanopticQuality.update / update_with_miou / update_with_miou_parts at 61..257 categories
    (across the 64-class fused confusion matrix and the 255-entry thing LUT of the parts path):
    PQ states bit-identical to the oracle, confusion matrices equal"""
    from nicr_mt_scene_analysis_amd import ops
    from nicr_mt_scene_analysis_amd.metric import MeanIntersectionOverUnion, PanopticQuality
    rng = np.random.default_rng(seed)
    n = C + 1
    # (256 ** 3 holds the ids of 256 categories: category 256 needs a larger offset)
    max_inst, offset = 1 << 16, (256 ** 3 if n <= 256 else 1 << 25)
    thing_c = rng.random(C) < 0.5
    edge = syn.wide_edge_classes(C)

    def rects(draw_value, fill=None):
        out = np.zeros((B, H, W), np.int64) if fill is None else fill.copy()
        for b in range(B):
            for _ in range(n_seg):
                y0, x0 = rng.integers(0, H), rng.integers(0, W)
                y1, x1 = rng.integers(y0, H) + 1, rng.integers(x0, W) + 1
                out[b, y0:y1, x0:x1] = draw_value()
        return out
    cls = lambda: rng.choice(edge) if rng.random() < 0.5 else rng.integers(0, C)     # noqa: E731
    sem = rects(cls).astype(np.uint8)                                    # class index 0..C-1
    inst = (rects(lambda: rng.integers(0, 7)) * thing_c[sem]).astype(np.uint8)
    pan_of_inst = np.zeros((B, 256), np.int64)
    pan_of_inst[:, 1:7] = (rng.choice(np.where(thing_c)[0], (B, 6)) + 1 if thing_c.any()
                           else rng.integers(0, C, (B, 6)) + 1) * max_inst + np.arange(1, 7)
    tgt = rects(lambda: cls() + 1) * max_inst + rects(lambda: rng.integers(0, 3))
    # (a uint8 semantic target holds class values up to 255: at 257 categories the last is absent)
    tsem = rects(lambda: min(cls() + 1, 255)).astype(np.uint8)
    d_pred = torch.empty((B, H, W), dtype=torch.int64, device='cuda')
    L_ = ops.L
    d_sem, d_inst, d_poi, d_thing = dev(sem), dev(inst), dev(pan_of_inst), dev(thing_c.astype(np.uint8))
    L_.check(L_.lib().nmsa_panoptic_paint(L_.ptr(d_sem), L_.ptr(d_inst), L_.ptr(d_poi), L_.ptr(d_thing),
                                          B, C, H, W, max_inst, 0, L_.ptr(d_pred), None,
                                          L_.stream_ptr(d_pred.device)), 'nmsa_panoptic_paint')
    pred = d_pred.cpu().numpy()
    assert np.array_equal(pred, np.where(inst > 0, np.take_along_axis(
        pan_of_inst, inst.reshape(B, -1).astype(np.int64), 1).reshape(B, H, W),
        np.where(thing_c[sem], 0, (sem.astype(np.int64) + 1) * max_inst)))
    is_thing = [False] + thing_c.tolist()
    state = None
    for b in range(B):
        *state, _ = oracle.pq_compare_and_accumulate(pred[b], tgt[b], n, 0, max_inst, offset, state=state)

    def check_pq(pq, what):
        got = [pq.iou_per_class, pq.tp_per_class, pq.fn_per_class, pq.fp_per_class]
        for g_, w in zip(got, state):
            assert np.array_equal(g_.cpu().numpy(), np.asarray(w, dtype=np.float64)), (seed, n, what)
        assert int(pq._status) == 0

    pq = PanopticQuality(n, 0, max_inst, offset, is_thing, device='cuda')
    pq.update(d_pred, dev(tgt))
    torch.cuda.synchronize()
    check_pq(pq, 'update')
    _count('pq_over_64_categories', n > 64)
    want_cm = oracle.confmat_update(pred // max_inst, tsem, n)
    pq2 = PanopticQuality(n, 0, max_inst, offset, is_thing, device='cuda')
    miou2 = MeanIntersectionOverUnion(n, device='cuda')
    pq2.update_with_miou(d_pred, dev(tgt), miou2, dev(tsem), max_inst)
    torch.cuda.synchronize()
    check_pq(pq2, 'update_with_miou')
    assert np.array_equal(miou2.confmat.cpu().numpy(), want_cm), (seed, n)
    parts = {'panoptic': d_pred, 'semantic_idx_u8': d_sem, 'instance': d_inst, 'pan_of_inst': d_poi,
             'is_thing': d_thing, 'void_label': 0, 'max_instances_per_category': max_inst}
    assert PanopticQuality.parts_usable(parts, d_pred, max_inst) == (C <= 255)
    pq3 = PanopticQuality(n, 0, max_inst, offset, is_thing, device='cuda')
    miou3 = MeanIntersectionOverUnion(n, device='cuda')
    pq3.update_with_miou_parts(parts, dev(tgt), miou3, dev(tsem), max_inst)
    torch.cuda.synchronize()
    check_pq(pq3, 'update_with_miou_parts')
    assert np.array_equal(miou3.confmat.cpu().numpy(), want_cm), (seed, n)
    assert int(miou2._status) == 0 and int(miou3._status) == 0
    if C > 255:
        _count('parts_fallback')        # (the states above equal the int64 map's: same oracle state)


# --------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize('C', [256, 257])
def test_wide_class_limit(C):
    """every entry capped at 256 classes: NMSA_ERR_ARG (NmsaError) at 257, results at 256"""
    from nicr_mt_scene_analysis_amd import ops
    from nicr_mt_scene_analysis_amd._lib import NmsaError
    B, H, W = 1, 12, 16
    inp = syn.make_wide_class_inputs(B, C, H, W, 8, seed=C)
    x = dev(inp['semantic_logits'].astype(np.float32))
    heat, off, thing = dev(inp['instance_center']), dev(inp['instance_offset']), \
        dev(inp['semantic_classes_is_thing'])
    sem = torch.zeros((B, H, W), dtype=torch.uint8, device='cuda')
    inst = torch.zeros((B, H, W), dtype=torch.uint8, device='cuda')
    poi = torch.zeros((B, 256), dtype=torch.int64, device='cuda')
    prob = torch.ones((B, H, W), dtype=torch.float32, device='cuda')
    pan = torch.zeros((B, H, W), dtype=torch.int64, device='cuda')
    tab = torch.zeros((B, 256), dtype=torch.float32, device='cuda')
    L_ = ops.L

    def paint():
        L_.check(L_.lib().nmsa_panoptic_paint(L_.ptr(sem), L_.ptr(inst), L_.ptr(poi),
                                              L_.ptr(ops._u8(thing)), B, C, H, W, 1 << 16, 0, L_.ptr(pan), None,
                                              L_.stream_ptr(pan.device)), 'nmsa_panoptic_paint')

    calls = {
        'pipeline': lambda: ops.panoptic_pipeline(x, heat, off, thing, want_score=True),
        'paint': paint,
        'scores': lambda: ops.panoptic_scores(x, sem, prob, inst, pan, poi, tab, 1 << 16),
        'argmax_u8': lambda: ops.semantic_argmax(x, want_u8=True, want_i64=False, want_score=False),
        'argmax_resized_u8': lambda: ops.semantic_argmax_resized(x, (H + 3, W + 5), want_u8=True,
                                                                 want_i64=False, want_score=False),
    }
    for name, call in calls.items():
        if C > 256:
            with pytest.raises(NmsaError):
                call()
        else:
            call()
            torch.cuda.synchronize()
    # the u8-free forms have no class cap
    r = ops.semantic_argmax(x, want_u8=False, want_i64=True, want_score=False)
    torch.cuda.synchronize()
    assert np.array_equal(r['idx'].cpu().numpy(), inp['semantic_logits'].argmax(axis=1))


# --------------------------------------------------------------------------------------- 8
def test_fuzz_wide_effective_cases():
    """runs last: the draws reached the paths they are aimed at (each count is checked when a
    test that makes it ran)"""
    want = {'fg_class_ge64': 500, 'fg_class_ge192': 100, 'edge_ties': 200,
            'images_over_64_centers': 20, 'ids_in_later_pass': 200, 'pq_over_64_categories': 20}
    for name, least in want.items():
        if name in _EFFECTIVE:
            assert _EFFECTIVE[name] >= least, _EFFECTIVE
