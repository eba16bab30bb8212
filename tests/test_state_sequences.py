"""
GPU tier (pytest -m gpu): state that lives from one call to the next.

Several entry points keep device (or pinned host) state between calls and skip its initialisation
on the next one: the vote tables of the pipeline (ops._VOTE_TABLES), the target-generator
workspaces (ops._TARGET_WORKSPACES), the PQ workspaces of a metric instance, the pinned table ring
of PanopticPostprocessing and the spec records of the losses (loss/_multi.py SpecState).  Each
rests on one invariant: a call leaves the state as it found it, whatever its parameters, its
stream or its status bits.  The tests here draw SEQUENCES of calls on shared state and check
every call against the oracle (fp64 for the losses) as if it had run on fresh state:

 1. call-history independence: parameters that change which words a call writes, more keys than
    the caches keep (eviction, recreation), status-raising calls followed by clean ones;
 2. stream independence: the same sequences on three streams ordered by wait_stream, and two
    streams released at the same moment behind one event (overlap measured with HIP events);
 3. graph capture beside eager calls: captured target generators, metric chain and pipeline
    replayed with eager calls of the same shapes in between.
"""
import contextlib

import numpy as np
import pytest
import torch

from _golden import ids_from_arrays
from test_fuzz_parity import _DERANDOMIZE, _n, check_pipeline, dev  # noqa: F401
from test_fuzz_wide_classes import make_wide_inputs, rows_per_pass, settings_
from test_speculative_grad import _gen, check_multi_loss, random_item_mix

pytestmark = pytest.mark.gpu

hypothesis = pytest.importorskip('hypothesis')
from hypothesis import given, strategies as st   # noqa: E402

_EFFECTIVE = {}
_RAN = set()                 # which producers of the counts ran (the evidence test checks those)
ROUNDS = 8                   # overlap rounds per surface (fixed: no retry loop)


def _count(name, k=1):
    _EFFECTIVE[name] = _EFFECTIVE.get(name, 0) + int(k)


_STREAMS = []


def streams():
    """three side streams shared by the whole module (cache keys hold the stream handle)"""
    if not _STREAMS:
        _STREAMS.extend(torch.cuda.Stream() for _ in range(3))
    return _STREAMS


@contextlib.contextmanager
def ordered(stream):
    """run the block on `stream`, ordered after and before the current stream's work"""
    if stream is None:
        yield
        return
    cur = torch.cuda.current_stream()
    stream.wait_stream(cur)
    with torch.cuda.stream(stream):
        yield
    cur.wait_stream(stream)


def pick_stream(draw, use_streams):
    return streams()[draw(st.integers(0, 2))] if use_streams else None


def _stream_id():
    return torch.cuda.current_stream().cuda_stream


class Gate:
    """release the work of two streams at one moment: both wait for an event that a third stream
    records behind a long sleep.  HIP timing events say whether the two streams' kernels actually
    ran side by side: each stream marks the end of its first launch (`mark`) and of its last one;
    the round overlapped when each stream's first launch ended before the other's last one did
    (streams served one after the other never give that)"""

    def __init__(self):
        self.s_a, self.s_b, self.s_gate = streams()
        self.gate = torch.cuda.Event()
        self.ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        self.overlapped = False

    @contextlib.contextmanager
    def run(self, which):
        s = (self.s_a, self.s_b)[which]
        s.wait_stream(torch.cuda.current_stream())
        s.wait_event(self.gate)
        with torch.cuda.stream(s):
            yield
            self.ev[2 + 2 * which].record(s)

    def mark(self, which):
        """call on stream `which` right after its first launch"""
        self.ev[1 + 2 * which].record()

    def __enter__(self):
        self.s_gate.wait_stream(torch.cuda.current_stream())
        self.ev[0].record(self.s_gate)
        with torch.cuda.stream(self.s_gate):
            torch.cuda._sleep(20_000_000)        # holds both streams while the host enqueues
        self.gate.record(self.s_gate)
        return self

    def __exit__(self, *exc):
        _RAN.add('overlap')
        cur = torch.cuda.current_stream()
        for s in (self.s_a, self.s_b, self.s_gate):
            cur.wait_stream(s)
        torch.cuda.synchronize()
        if exc[0] is None:
            t = [self.ev[0].elapsed_time(e) for e in self.ev[1:]]
            self.overlapped = t[0] < t[3] and t[2] < t[1]
            _count('overlap_rounds', self.overlapped)
        return False


# ===================================================================================== pipeline
WORD_C = (2, 5, 31, 47, 48, 49, 63, 64, 65, 127, 128, 129, 143, 144, 145, 191, 192, 193, 255, 256)


def assign_is_ragged(n_cols):
    """k_assign leaves its 16-byte loop for the word-by-word one in some pass: a pass of a word
    count that is not a multiple of 4, or a pass that starts off a 16-byte boundary"""
    rpp = rows_per_pass(n_cols)
    return any((min(rpp, 256 - r0) * n_cols) % 4 or (r0 * n_cols) % 4 for r0 in range(0, 256, rpp))


@st.composite
def pipeline_call(draw):
    C = draw(st.one_of(st.sampled_from(WORD_C), st.integers(2, 256)))
    regime = draw(st.sampled_from(['none', 'few', 'many']))
    if regime == 'many':            # the LDS center table, votes in later passes of k_assign
        n = draw(st.integers(65, 255))
        H, W = draw(st.integers(20, 26)), draw(st.sampled_from([61, 64, 96]))
    else:
        n = 0 if regime == 'none' else draw(st.integers(1, 8))
        H, W = draw(st.integers(3, 24)), draw(st.sampled_from([5, 13, 31, 32, 33, 47, 64]))
    fewer = draw(st.sampled_from([0, 0, 1, 9]))
    return dict(C=C, B=draw(st.integers(1, 3)), H=H, W=W, n=n, seed=draw(st.integers(0, 2 ** 31 - 1)),
                levels=draw(st.sampled_from([2, 4])), p_tie=draw(st.sampled_from([0.0, 0.3])),
                p_thing=draw(st.sampled_from([0.2, 0.5, 0.9])), p_far=draw(st.sampled_from([0.0, 0.2])),
                specials=False, dtype=draw(st.sampled_from(['float32', 'bfloat16', 'float16'])),
                thr=0.1, ksize=3, topk=max(1, min(255, n - fewer)),
                apply_fg=draw(st.sampled_from([False, True])),
                dist_thr=draw(st.sampled_from([None, None, 0.5, 3.0])),
                normalized=draw(st.booleans()), max_centers=draw(st.sampled_from([256, 1024])))


def pipeline_inputs(p):
    logits, heat, offset, is_thing = make_wide_inputs(p)
    if not p['normalized']:         # the same vectors in pixels
        H, W = logits.shape[2:]
        offset = (offset * np.array([H, W], np.float32).reshape(1, 2, 1, 1)).astype(np.float32)
    return logits, heat, offset, is_thing


def assert_vote_tables_zero():
    from nicr_mt_scene_analysis_amd import ops
    torch.cuda.synchronize()
    for key, t in ops._VOTE_TABLES.items():
        assert not bool(t.any()), f'vote table {key[1:3]} left dirty'


_SEEN_TABLES = set()


def run_pipeline_call(oracle, p):
    from nicr_mt_scene_analysis_amd import ops
    key = (torch.device('cuda', torch.cuda.current_device()), p['B'], p['C'] + 1, _stream_id())
    before = set(ops._VOTE_TABLES)
    inputs = pipeline_inputs(p)
    res = check_pipeline(oracle, p, max_centers=p['max_centers'], inputs=inputs)
    assert res is not None and (res['n'] <= p['n']).all(), p
    assert_vote_tables_zero()
    if key in before and assign_is_ragged(p['C'] + 1) and res['n'].any():
        _count('ragged_assign_with_reuse')
    if key not in before and key in _SEEN_TABLES:
        _count('vote_table_recreated')
    _SEEN_TABLES.add(key)
    return res


@pytest.mark.parametrize('use_streams', [False, True])
@settings_(10)
@given(data=st.data())
def test_pipeline_call_sequences(oracle, use_streams, data):
    """6..12 pipeline calls of random (B, C), dtypes, center counts, masks and offsets on the
    shared vote tables (more keys than the LRU keeps); every call bit-exact vs the oracle and
    every cached table all zero after it"""
    _RAN.add('pipeline')
    calls = data.draw(st.lists(pipeline_call(), min_size=6, max_size=12))
    for i, p in enumerate(calls):
        if i and data.draw(st.booleans()):      # the table of an earlier call again
            p.update(B=calls[i - 1]['B'], C=calls[i - 1]['C'])
        with ordered(pick_stream(data.draw, use_streams)):
            run_pipeline_call(oracle, p)


def test_postprocessing_pinned_ring_reuse(oracle):
    """one PanopticPostprocessing object with defer_host_sync: 12 calls of one shape (more than the
    ring of 8 pinned slots) whose lazy id tables are read late and out of order, with eager calls
    of a second object in between; center counts rise (host columns grow), overflow the center
    table (the lazy read raises and enlarges it, the eager call re-runs larger) and fall again"""
    _RAN.add('postprocessing')
    from nicr_mt_scene_analysis_amd import ops
    from nicr_mt_scene_analysis_amd.model.postprocessing import get_postprocessing_class

    def make(defer):
        return get_postprocessing_class('panoptic')(
            semantic_postprocessing=get_postprocessing_class('semantic')(),
            instance_postprocessing=get_postprocessing_class('instance')(
                heatmap_threshold=0.1, heatmap_nms_kernel_size=3, top_k_instances=254),
            semantic_classes_is_thing=is_thing_t, semantic_class_has_orientation=is_thing_t,
            compute_scores=False, defer_host_sync=defer)

    B, C, H, W = 2, 40, 24, 96
    base = dict(C=C, B=B, H=H, W=W, levels=2, p_tie=0.0, p_thing=0.6, p_far=0.0, specials=False,
                dtype='float32', thr=0.1, ksize=3, apply_fg=False, dist_thr=None, normalized=True)
    lut = make_wide_inputs(dict(base, n=0, seed=0, topk=1))[3]        # one thing LUT for every call
    is_thing_t = tuple(bool(v) for v in lut)
    lazy, eager = make(True), make(False)
    from nicr_mt_scene_analysis_amd.data.preprocessing import APPLIED_PREPROCESSING_KEY
    batch = {'rgb_fullres': torch.zeros((B, 3, H, W)),
             APPLIED_PREPROCESSING_KEY: [[{'type': 'Resize', 'valid_region_slice_y': slice(0, H),
                                           'valid_region_slice_x': slice(0, W)}]] * B}

    def tied_peaks(seed, n=300):
        """n equal isolated peaks: the top-k keeps them all as ties (> 256 centers)"""
        logits, _, offset, _ = make_wide_inputs(dict(base, n=0, seed=seed, topk=1))
        heat = np.zeros((B, 1, H, W), np.float32)
        ys, xs = np.meshgrid(np.arange(1, H, 2), np.arange(1, W, 2), indexing='ij')
        heat[:, 0, ys.reshape(-1)[:n], xs.reshape(-1)[:n]] = 1.0
        return (dev(logits), (dev(heat), dev(offset))), (None, None)

    spied = lazy._pinned_slot

    def spy(shape, ring=8):                 # a slot taken while its previous result is unread
        slots = lazy._pinned_ring.get(shape, [])
        if len(slots) >= ring and slots[lazy._pinned_next[shape]]['detach'] is not None:
            _count('pinned_slot_reused_before_read')
        return spied(shape, ring)
    lazy._pinned_slot = spy

    def same_ids(r, want):
        return [list(d.items()) for d in r['panoptic_segmentation_deeplab_ids']] == \
            [list(d.items()) for d in want['ids']]

    pending = []
    rng = np.random.default_rng(5)
    for i, n in enumerate([3, 40, 200, 7, 0, 120, 9, 254, 12, 60, 2, 180]):
        if i == 4:                  # center-table overflow: the lazy read raises, the table grows
            r = lazy.postprocess(tied_peaks(41), batch, is_training=False)
            with pytest.raises(RuntimeError, match='center table'):
                r['panoptic_segmentation_deeplab_ids']
            assert lazy._instance_postprocessing._max_centers == 512
        p = dict(base, n=n, seed=100 + i, topk=254)
        inputs = make_wide_inputs(p)[:3] + (lut,)
        want = check_pipeline(oracle, p, max_centers=256, inputs=inputs)
        x = ((dev(inputs[0]), (dev(inputs[1]), dev(inputs[2]))), (None, None))
        pending.append((lazy.postprocess(x, batch, is_training=False), want))
        if i == 5:                  # the eager object overflows and re-runs with a larger table
            xo = tied_peaks(42)
            re = eager.postprocess(xo, batch, is_training=False)
            assert eager._instance_postprocessing._max_centers == 512
            o = ops.panoptic_pipeline(xo[0][0], *xo[0][1], dev(lut), threshold=0.1, kernel_size=3,
                                      top_k=254, max_centers=512)
            assert int(o['n_centers'].max()) > 256
            assert torch.equal(re['panoptic_segmentation_deeplab'], o['panoptic'])
        elif i % 3 == 2:            # an eager call of another object in between
            n_e = int(rng.choice([1, 70, 254, 4]))
            pe = dict(base, n=n_e, seed=500 + i, topk=254)
            ie = make_wide_inputs(pe)[:3] + (lut,)
            we = check_pipeline(oracle, pe, max_centers=256, inputs=ie)
            re = eager.postprocess(((dev(ie[0]), (dev(ie[1]), dev(ie[2]))), (None, None)), batch,
                                   is_training=False)
            assert same_ids(re, we)
        if len(pending) > 8 and rng.random() < 0.5:     # read one result late, out of order
            r, want = pending.pop(int(rng.integers(0, len(pending))))
            assert same_ids(r, want)
    rng.shuffle(pending)
    for r, want in pending:
        assert np.array_equal(r['panoptic_segmentation_deeplab'].cpu().numpy(), want['pan'])
        assert same_ids(r, want)
    assert_vote_tables_zero()


# ===================================================================================== targets
def label_maps(rng, B, H, W, NC, n_inst, kind):
    sem = rng.integers(0, NC, (B, H, W)).astype(np.uint8)
    ins = np.zeros((B, H, W), np.int32)
    for b in range(B):
        for _ in range(n_inst):
            ya, xa = rng.integers(0, H), rng.integers(0, W)
            yb, xb = rng.integers(ya, H) + 1, rng.integers(xa, W) + 1
            ins[b, ya:yb, xa:xb] = rng.integers(1, 65536)
            if rng.random() < 0.6:
                sem[b, ya:yb, xa:xb] = rng.integers(0, NC)
    if kind == 'id_range':
        ins[rng.integers(0, B), rng.integers(0, H), rng.integers(0, W)] = 70000 + int(rng.integers(0, 1000))
    elif kind == 'class_range':     # (a class is checked where it votes: on an instance pixel)
        b, y, x = rng.integers(0, B), rng.integers(0, H), rng.integers(0, W)
        sem[b, y, x] = NC + int(rng.integers(0, 3))
        ins[b, y, x] = 5
    elif kind == 'too_many':        # one distinct id per pixel of the first rows
        k = min(H * W, 4096)
        ins[0].reshape(-1)[:k] = np.arange(1, k + 1, dtype=np.int32) * 7
    return sem, ins


@st.composite
def target_call(draw, keys):
    NC, B, max_inst = keys[draw(st.integers(0, len(keys) - 1))]
    wire = draw(st.booleans())
    W = 4 * draw(st.integers(1, 12)) if wire else draw(st.sampled_from([5, 7, 13, 22, 31]))
    kind = draw(st.sampled_from(['clean'] * 5 + ['id_range', 'class_range', 'too_many']))
    what = draw(st.sampled_from(['instance', 'panoptic', 'both']))
    return dict(NC=NC, B=B, max_inst=max_inst, H=draw(st.integers(3, 40)), W=W, wire=wire,
                ins_i64=(not wire) and draw(st.booleans()), kind=kind,
                what='instance' if kind == 'class_range' else what,
                n_inst=draw(st.integers(0, 12)), sigma=draw(st.integers(1, 5)),
                normalized=draw(st.booleans()), seed=draw(st.integers(0, 2 ** 31 - 1)))


_WS_HISTORY = {}


def run_target_call(oracle, c, launch_only=False, gate=None, which=0):
    """one instance / panoptic target call (or both) against the oracle; status-raising calls
    must report their bit, every other call must be exact"""
    from nicr_mt_scene_analysis_amd import ops
    rng = np.random.default_rng(c['seed'])
    B, H, W, NC = c['B'], c['H'], c['W'], c['NC']
    sem, ins = label_maps(rng, B, H, W, NC, c['n_inst'], c['kind'])
    is_thing = rng.random(NC) < 0.5
    is_thing[0] = False
    stuff = np.zeros((NC,), np.uint8)
    stuff[np.where(~is_thing)[0][1:]] = 1
    d_sem, d_ins = dev(sem), dev(ins.astype(np.int64) if c['ins_i64'] else ins)
    d_th, d_st = dev(is_thing.astype(np.uint8)), dev(stuff)
    whats = ['instance', 'panoptic'] if c['what'] == 'both' else [c['what']]
    key = (torch.device('cuda', torch.cuda.current_device()), _stream_id(), B, NC, c['max_inst'])
    out = []
    for i, what in enumerate(whats):
        if i and gate is not None:
            gate.mark(which)
        if what == 'instance':
            r = ops.instance_targets(d_sem, d_ins, NC, d_th, d_st, c['sigma'], c['normalized'],
                                     max_instances=c['max_inst'])
        else:
            r = ops.panoptic_targets(d_sem, d_ins, NC, d_th, 1 << 16, 0, max_instances=c['max_inst'])
        out.append((what, r))
        if ops._targets_on_wire(d_sem, d_ins, H, W, NC):
            hist = _WS_HISTORY.setdefault(key, [])
            hist.append((what, (H, W), c['kind']))
            if len({h[1] for h in hist}) > 1:
                _count('workspace_two_sizes')
            if [h[0] for h in hist[-3:]] == ['instance', 'panoptic', 'instance']:
                _count('instance_panoptic_instance')
            if len(hist) > 1 and hist[-2][2] != 'clean' and c['kind'] == 'clean':
                _count('status_then_clean')
    if launch_only:
        return lambda: check_target_results(oracle, c, out, sem, ins, is_thing, stuff)
    check_target_results(oracle, c, out, sem, ins, is_thing, stuff)


def check_target_results(oracle, c, out, sem, ins, is_thing, stuff):
    torch.cuda.synchronize()
    B = c['B']
    for what, r in out:
        status = int(r['status'].item())
        if c['kind'] != 'clean':
            if c['kind'] == 'id_range':
                assert status & 32, (c, what, status)
            elif c['kind'] == 'class_range':
                assert status & 64, (c, what, status)
            elif max(len(np.unique(ins[b][ins[b] > 0])) for b in range(B)) > -(-c['max_inst'] // 1024) * 1024:
                assert status & 1, (c, what, status)    # more distinct ids than the tables hold
            continue                    # (too_many within the tables: the next call must be exact)
        assert status == 0, (c, what, status)
        if what == 'instance':
            o = oracle.instance_targets(sem, ins, c['NC'], is_thing, stuff, c['sigma'], c['normalized'])
            assert np.array_equal(r['center'].cpu().numpy(), o['center']), c
            assert np.array_equal(r['offset'].cpu().numpy(), o['offset']), c
            assert np.array_equal(r['foreground'].cpu().numpy(), o['foreground']), c
            assert np.array_equal(r['center_mask'].cpu().numpy(), o['center_mask']), c
            ne, ns = r['n_encoded'].cpu().numpy(), r['n_skipped'].cpu().numpy()
            for b in range(B):
                assert r['encoded_ids'][b, :ne[b]].cpu().tolist() == o['encoded'][b], c
                assert r['skipped_ids'][b, :ns[b]].cpu().tolist() == o['skipped'][b], c
        else:
            pan, dicts = oracle.naive_merge(sem, ins, 1 << 16, np.where(is_thing)[0], 0)
            assert np.array_equal(r['panoptic'].cpu().numpy(), pan), c
            got = ids_from_arrays(r['n_ids'].cpu().numpy(), r['ids_pan'].cpu().numpy(),
                                  r['ids_ins'].cpu().numpy())
            assert [list(d.items()) for d in got] == [list(d.items()) for d in dicts], c


@st.composite
def target_keys(draw):
    return [(draw(st.integers(2, 12)), draw(st.integers(1, 2)), draw(st.sampled_from([16, 64, 1024])))
            for _ in range(draw(st.integers(1, 3)))]


@pytest.mark.parametrize('use_streams', [False, True])
@settings_(12)
@given(data=st.data())
def test_target_call_sequences(oracle, use_streams, data):
    """6..12 target-generator calls on few (B, classes, max_instances) keys — so that one
    workspace serves images of different size, instance and panoptic targets in turn, on-wire and
    off-wire layouts, status-raising calls among clean ones — each exact vs the oracle"""
    _RAN.add('targets')
    keys = data.draw(target_keys())
    for c in data.draw(st.lists(target_call(keys), min_size=6, max_size=12)):
        with ordered(pick_stream(data.draw, use_streams)):
            run_target_call(oracle, c)


# ===================================================================================== PQ
PQ_B, PQ_H, PQ_W = 2, 64, 96


def pq_inputs(rng, C, max_inst, overflow=False):
    """(parts dict, prediction, target, target semantic) on PQ_B x PQ_H x PQ_W: rectangles of
    classes, instances on thing classes only, the prediction painted from its parts"""
    from nicr_mt_scene_analysis_amd import ops
    B, H, W = PQ_B, PQ_H, PQ_W
    n = C + 1
    thing_c = np.zeros(C, bool)
    thing_c[: C // 2] = True

    def rects(hi, k=9):
        out = np.zeros((B, H, W), np.int64)
        for b in range(B):
            for _ in range(k):
                y0, x0 = rng.integers(0, H), rng.integers(0, W)
                y1, x1 = rng.integers(y0, H) + 1, rng.integers(x0, W) + 1
                out[b, y0:y1, x0:x1] = rng.integers(0, hi)
        return out
    sem = rects(C).astype(np.uint8)
    inst = (rects(7) * thing_c[sem]).astype(np.uint8)
    pan_of_inst = np.zeros((B, 256), np.int64)
    pan_of_inst[:, 1:7] = rng.integers(1, n, (B, 6)) * max_inst + np.arange(1, 7)
    tgt = rects(n) * max_inst + rects(3)
    tsem = rects(n).astype(np.uint8)
    if overflow:                    # per-pixel noise: more distinct intersections than the table holds
        tgt = rng.integers(1, n, (B, H, W)) * max_inst + rng.integers(0, 3000, (B, H, W))
    d_pred = torch.empty((B, H, W), dtype=torch.int64, device='cuda')
    L_ = ops.L
    d_sem, d_inst, d_poi, d_thing = dev(sem), dev(inst), dev(pan_of_inst), dev(thing_c.astype(np.uint8))
    L_.check(L_.lib().nmsa_panoptic_paint(L_.ptr(d_sem), L_.ptr(d_inst), L_.ptr(d_poi), L_.ptr(d_thing),
                                          B, C, H, W, max_inst, 0, L_.ptr(d_pred), None,
                                          L_.stream_ptr(d_pred.device)), 'nmsa_panoptic_paint')
    parts = {'panoptic': d_pred, 'semantic_idx_u8': d_sem, 'instance': d_inst, 'pan_of_inst': d_poi,
             'is_thing': d_thing, 'void_label': 0, 'max_instances_per_category': max_inst}
    return parts, dev(tgt), dev(tsem), tgt, tsem


class PQRef:
    """the oracle's accumulation of the same updates"""

    def __init__(self, n, max_inst):
        self.n, self.max_inst = n, max_inst
        self.reset()

    def reset(self):
        self.state, self.cm = None, np.zeros((self.n, self.n), np.int64)

    def add(self, oracle, pred, tgt, tsem=None):
        for b in range(pred.shape[0]):
            *self.state, _ = oracle.pq_compare_and_accumulate(pred[b], tgt[b], self.n, 0, self.max_inst,
                                                              256 ** 3, state=self.state)
        if tsem is not None:
            self.cm = oracle.confmat_update(pred // self.max_inst, tsem, self.n, confmat=self.cm)

    def check(self, pq, miou, what):
        got = [pq.iou_per_class, pq.tp_per_class, pq.fn_per_class, pq.fp_per_class]
        if self.state is None:
            assert all(not bool(g.any()) for g in got), what
        else:
            for g, w in zip(got, self.state):
                assert np.array_equal(g.cpu().numpy(), np.asarray(w, dtype=np.float64)), what
        assert np.array_equal(miou.confmat.cpu().numpy(), self.cm), what


PQ_PATHS = ('pred', 'pred_cm', 'parts', 'parts_cm')


def pq_update(pq, miou, path, parts, d_tgt, d_tsem, max_inst):
    if path == 'pred':
        pq.update(parts['panoptic'], d_tgt)
    elif path == 'pred_cm':
        pq.update_with_miou(parts['panoptic'], d_tgt, miou, d_tsem, max_inst)
    elif path == 'parts':
        pq._device_update(parts['panoptic'], d_tgt, want_matches=False, parts=parts)
    else:
        pq.update_with_miou_parts(parts, d_tgt, miou, d_tsem, max_inst)


_PQ_PAIRS = set()


@pytest.mark.parametrize('use_streams', [False, True])
@settings_(8)
@given(data=st.data())
def test_pq_update_sequences(oracle, use_streams, data):
    """one PanopticQuality + MeanIntersectionOverUnion and one (B, H, W): the four update paths in
    random order on the shared workspace, overflowing updates and reset() among them; after every
    update the accumulated states equal the oracle's accumulation of the same inputs"""
    _RAN.add('pq')
    steps = data.draw(st.lists(st.sampled_from(PQ_PATHS * 3 + ('overflow', 'reset')), min_size=6, max_size=12))
    run_pq_steps(oracle, steps, data.draw(st.integers(2, 12)), data.draw(st.integers(0, 2 ** 31 - 1)),
                 lambda: pick_stream(data.draw, use_streams))


def test_pq_every_path_after_every_other(oracle):
    """a fixed walk through all 12 ordered pairs of update paths on one workspace"""
    _RAN.add('pq')
    a, b, c, d = PQ_PATHS
    run_pq_steps(oracle, [a, b, c, d, a, c, a, d, b, d, c, b, a], 5, 21, lambda: None)


def run_pq_steps(oracle, steps, C, seed, stream_of):
    from nicr_mt_scene_analysis_amd.metric import MeanIntersectionOverUnion, PanopticQuality
    max_inst = 1 << 16
    n = C + 1
    rng = np.random.default_rng(seed)
    pq = PanopticQuality(n, 0, max_inst, 256 ** 3, [False] + [c < C // 2 for c in range(C)], device='cuda')
    miou = MeanIntersectionOverUnion(n, device='cuda')
    ref = PQRef(n, max_inst)
    last = None
    for step in steps:
        with ordered(stream_of()):
            if step == 'reset':
                pq.reset()
                miou.reset()
                ref.reset()
                continue
            parts, d_tgt, d_tsem, tgt, tsem = pq_inputs(rng, C, max_inst, overflow=step == 'overflow')
            pq_update(pq, miou, 'pred' if step == 'overflow' else step, parts, d_tgt, d_tsem, max_inst)
            torch.cuda.synchronize()
            pred = parts['panoptic'].cpu().numpy()
            if step == 'overflow':
                if int(pq._status):         # reported: the states are void until reset()
                    _count('pq_overflow')
                    pq.reset()
                    miou.reset()
                    ref.reset()
                    last = None
                    continue
                step = 'pred'
            assert int(pq._status) == 0 and int(miou._status) == 0, step
            ref.add(oracle, pred, tgt, tsem if step.endswith('_cm') else None)
            ref.check(pq, miou, step)
            key = (_stream_id(),)
            if last is not None and last[0] == key:
                _PQ_PAIRS.add((last[1], step))
            last = (key, step)


# ===================================================================================== losses
def ticket_rows_zero(specs):
    torch.cuda.synchronize()
    for spec in specs:
        for key, r in spec._rec.items():
            assert not bool(r[spec.n_totals].any()), f'spec tickets left non-zero {key}'


def loss_mix(rng, g, T):
    items, refs, n_totals = random_item_mix(rng, g)
    for it in items:
        it['total'] = it['total'] % T
    T = min(T, max(it['total'] for it in items) + 1)
    leaves = [it['pred'].clone().requires_grad_(True) for it in items]
    for it, lf in zip(items, leaves):
        it['pred'] = lf
    return items, refs, T, leaves


def run_loss_call(helper, l1, mode, rng, g, T):
    """one multi-loss call through `helper`'s spec records (or the L1Loss instance) in `mode`,
    checked against fp64"""
    from nicr_mt_scene_analysis_amd.loss import _multi
    names = tuple(f't{i}' for i in range(T))
    factors = torch.tensor(rng.choice([1.0, 0.5, 2.0, 3.0], size=T), dtype=torch.float32, device='cuda')
    if mode == 'loss_instance':
        B, H, W = int(rng.integers(1, 3)), 4 * int(rng.integers(1, 6)), 4 * int(rng.integers(1, 9))
        p = torch.randn((B, 2, H, W), device='cuda', generator=g).requires_grad_(True)
        y = torch.randn((B, 2, H, W), device='cuda', generator=g)
        m = torch.rand((B, H, W), device='cuda', generator=g) < 0.6
        ls, n = l1.masked_sum(p, y, m)
        f = float(factors[0])
        (f * ls / n).backward()
        pr = p.detach().double().requires_grad_(True)
        want = (pr * m.unsqueeze(1) - y.double()).abs().mean(dim=1).sum()
        (want * f / max(int(m.sum()), 1)).backward()
        assert int(n) == int(m.sum())
        np.testing.assert_allclose(float(ls), float(want), rtol=2e-5, atol=1e-5)
        np.testing.assert_allclose(p.grad.double().cpu().numpy(), pr.grad.cpu().numpy(), rtol=2e-5, atol=1e-9)
        return
    items, refs, T_, leaves = loss_mix(rng, g, T)
    spec = helper.spec_state(names[:T_])
    factors = factors[:T_]
    if mode == 'no_grad':
        with torch.no_grad():
            res = _multi.multi_loss(items, T_, spec)
        check_multi_loss(items, refs, T_, res, leaves, factors, check_grads=False)
    elif mode == 'no_backward':
        res = _multi.multi_loss(items, T_, spec)
        check_multi_loss(items, refs, T_, res, leaves, factors, check_grads=False)
    elif mode == 'two_forwards':
        items2, refs2, T2, leaves2 = loss_mix(rng, g, T_)
        spec2 = helper.spec_state(names[:T2])
        res = _multi.multi_loss(items, T_, spec)
        res2 = _multi.multi_loss(items2, T2, spec2)
        ((res.total_losses * factors).sum() + (res2.total_losses * factors[:T2]).sum()).backward()
        check_multi_loss(items, refs, T_, res, leaves, factors)
        check_multi_loss(items2, refs2, T2, res2, leaves2, factors[:T2])
    elif mode == 'retain_graph':
        res = _multi.multi_loss(items, T_, spec)
        total = (res.total_losses * factors).sum()
        total.backward(retain_graph=True)
        total.backward()
        check_multi_loss(items, refs, T_, res, leaves, 2 * factors)
    else:
        res = _multi.multi_loss(items, T_, spec)
        (res.total_losses * factors).sum().backward()
        check_multi_loss(items, refs, T_, res, leaves, factors)


LOSS_MODES = ('plain', 'plain', 'no_grad', 'no_backward', 'two_forwards', 'retain_graph', 'loss_instance')


def all_specs(helper, l1):
    specs = list(helper.__dict__.get('_spec_states', {}).values())
    if l1.__dict__.get('_spec') is not None:
        specs.append(l1._spec)
    return specs


@pytest.mark.parametrize('use_streams', [False, True])
@settings_(6)
@given(data=st.data())
def test_loss_call_sequences(use_streams, data):
    """one SemanticTaskHelper's spec records and one L1Loss instance across calls of changing
    item mixes, dtypes, shapes and upstream factors, under no_grad, without backward, two forwards
    with one backward and retain_graph: values and gradients vs fp64, the ticket rows zero after
    every call"""
    from nicr_mt_scene_analysis_amd.loss import L1Loss
    from nicr_mt_scene_analysis_amd.task_helper.semantic import SemanticTaskHelper
    helper, l1 = SemanticTaskHelper(n_classes=4), L1Loss()
    seed = data.draw(st.integers(0, 2 ** 31 - 1))
    rng, g = np.random.default_rng(seed), _gen(seed % 10007)
    T = data.draw(st.integers(1, 3))
    for mode in data.draw(st.lists(st.sampled_from(LOSS_MODES), min_size=6, max_size=10)):
        with ordered(pick_stream(data.draw, use_streams)):
            run_loss_call(helper, l1, mode, rng, g, T)
        ticket_rows_zero(all_specs(helper, l1))


# ===================================================================================== overlap
def test_spec_records_are_per_stream():
    """deterministic: a loss caller never hands two streams the same record tensor (the launch
    tickets live in it); the summed statistics and reset() cover every stream's set"""
    from nicr_mt_scene_analysis_amd.loss import _multi
    spec = _multi.SpecState(2, [1.0, 3.0])
    s_a, s_b, _ = streams()
    with torch.cuda.stream(s_a):
        ra = spec.records('cuda')
        assert spec.records('cuda') is ra
        assert spec.weights('cuda') == [1.0, 3.0]
    with torch.cuda.stream(s_b):
        rb = spec.records('cuda')
    r0 = spec.records('cuda')
    assert ra.data_ptr() != rb.data_ptr() and r0.data_ptr() not in (ra.data_ptr(), rb.data_ptr())
    ra[0, 0] = 2
    rb[1, 1] = 5
    assert spec.stats() == {'confirmed': 2, 'recomputed': 5}
    spec.reset()
    assert spec.stats() == {'confirmed': 0, 'recomputed': 0}
    graph = torch.cuda.CUDAGraph()          # a set made inside a capture: no host copy in it
    with torch.cuda.graph(graph):
        rc = spec.records('cuda')
    graph.replay()
    torch.cuda.synchronize()
    assert rc.view(torch.float32)[:2, 2].tolist() == [1.0, 3.0] and not bool(rc[2].any())
    extra = [torch.cuda.Stream() for _ in range(_multi.SpecState.MAX_RECORDS + 2)]
    for s in extra:
        with torch.cuda.stream(s):
            spec.records('cuda')
    assert len(spec._rec) == _multi.SpecState.MAX_RECORDS


def test_overlapping_pipelines(oracle):
    """two streams run their own pipeline calls released at one moment: both exact, the vote
    tables clean afterwards"""
    from nicr_mt_scene_analysis_amd import ops
    B, C, H, W = 2, 193, 24, 96
    p = dict(C=C, B=B, H=H, W=W, levels=2, p_tie=0.3, p_thing=0.9, p_far=0.0, specials=False,
             dtype='float32', thr=0.1, ksize=3, topk=255, apply_fg=False, dist_thr=None, normalized=True)
    for rnd in range(ROUNDS):
        calls = []
        for which in range(2):
            q = dict(p, n=[200, 90][which], seed=1000 * rnd + which)
            inputs = make_wide_inputs(q)
            calls.append((q, inputs, [dev(a) for a in inputs]))
        outs = []
        with Gate() as gate:
            for which, (q, _, d) in enumerate(calls):
                with gate.run(which):
                    rs = [ops.panoptic_pipeline(*d, top_k=255, want_score=True)]
                    gate.mark(which)
                    rs += [ops.panoptic_pipeline(*d, top_k=255, want_score=True) for _ in range(2)]
                    outs.append(rs)
        for (q, inputs, _), rs in zip(calls, outs):
            want = check_pipeline(oracle, q, max_centers=256, inputs=inputs)
            for r in rs:
                assert np.array_equal(r['panoptic'].cpu().numpy(), want['pan']), rnd
                assert np.array_equal(r['instance'].cpu().numpy(), want['inst']), rnd
        assert_vote_tables_zero()


def test_overlapping_target_generators(oracle):
    """two streams run target generators on workspaces of the same key (B, classes,
    max_instances) released at one moment: every call exact"""
    for rnd in range(ROUNDS):
        cs = [dict(NC=7, B=2, max_inst=64, H=48, W=64, wire=True, ins_i64=False, kind='clean',
                   what='both', n_inst=10, sigma=3, normalized=True, seed=77 * rnd + w) for w in range(2)]
        run_target_call(oracle, cs[0])               # warm (gauss LUT, workspaces)
        checks = []
        with Gate() as gate:
            for which, c in enumerate(cs):
                with gate.run(which):
                    checks.append(run_target_call(oracle, c, launch_only=True, gate=gate, which=which))
        for chk in checks:
            chk()


def test_overlapping_pq_instances(oracle):
    """one metric pair per stream, both updated at one moment: each equals the oracle"""
    from nicr_mt_scene_analysis_amd.metric import MeanIntersectionOverUnion, PanopticQuality
    C, max_inst = 6, 1 << 16
    n = C + 1
    rng = np.random.default_rng(11)
    mets = [(PanopticQuality(n, 0, max_inst, 256 ** 3, [False] + [c < C // 2 for c in range(C)], device='cuda'),
             MeanIntersectionOverUnion(n, device='cuda'), PQRef(n, max_inst)) for _ in range(2)]
    for rnd in range(ROUNDS):
        ins = [pq_inputs(rng, C, max_inst) for _ in range(2)]
        torch.cuda.synchronize()
        with Gate() as gate:
            for which, ((pq, miou, _), (parts, d_tgt, d_tsem, _, _)) in enumerate(zip(mets, ins)):
                with gate.run(which):
                    gate.mark(which)        # (one update: the mark is its start)
                    pq_update(pq, miou, PQ_PATHS[(rnd + which) % 4], parts, d_tgt, d_tsem, max_inst)
        for which, ((pq, miou, ref), (parts, _, _, tgt, tsem)) in enumerate(zip(mets, ins)):
            path = PQ_PATHS[(rnd + which) % 4]
            ref.add(oracle, parts['panoptic'].cpu().numpy(), tgt, tsem if path.endswith('_cm') else None)
            ref.check(pq, miou, (rnd, which))


def test_overlapping_shared_loss_helper():
    """ONE task helper's spec records used from two streams at one moment (a validation step on a
    side stream while training goes on): values and gradients vs fp64, every ticket row zero"""
    from nicr_mt_scene_analysis_amd.loss import _multi
    from nicr_mt_scene_analysis_amd.task_helper.semantic import SemanticTaskHelper
    helper = SemanticTaskHelper(n_classes=4)
    spec = helper.spec_state(('semantic',))
    g = _gen(17)

    def items_of(seed):
        rng = np.random.default_rng(seed)
        B, H, W = 2, 96, 128
        out = []
        C = int(rng.choice([7, 40]))
        x = torch.randn((B, C, H, W), device='cuda', generator=g)
        t = torch.randint(0, C + 1, (B, H, W), device='cuda', generator=g).to(torch.uint8)
        out.append(({'kind': 'ce', 'pred': x.requires_grad_(True), 'mask': t, 'total': 0},
                    lambda xd, t=t: (torch.nn.functional.cross_entropy(xd, t.long() - 1, ignore_index=-1,
                                                                       reduction='sum'), int((t != 0).sum()))))
        y = torch.randn((B, H, W), device='cuda', generator=g)
        m = torch.rand((B, H, W), device='cuda', generator=g) < 0.5
        out.append(({'kind': 'mse', 'pred': torch.randn((B, H, W), device='cuda', generator=g).requires_grad_(True),
                     'target': y, 'mask': m, 'total': 0},
                    lambda xd, y=y, m=m: (((xd * m - y.double()) ** 2).sum(), int(m.sum()))))
        return [o[0] for o in out], [o[1] for o in out]

    failures = []
    factors = torch.tensor([2.0], device='cuda')
    for which in range(2):              # warm: each stream's records, the status word
        with torch.cuda.stream(streams()[which]):
            items, refs = items_of(which)
            _multi.multi_loss(items, 1, spec).total_losses.sum().backward()
    torch.cuda.synchronize()
    for rnd in range(ROUNDS):
        calls = [items_of(100 * rnd + w) for w in range(2)]
        res = []
        with Gate() as gate:
            for which, (items, refs) in enumerate(calls):
                with gate.run(which):
                    r = _multi.multi_loss(items, 1, spec)
                    gate.mark(which)
                    (r.total_losses * factors).sum().backward()
                    res.append(r)
        try:
            for (items, refs), r in zip(calls, res):
                check_multi_loss(items, refs, 1, r, [it['pred'] for it in items], factors)
            ticket_rows_zero([spec])
        except AssertionError as e:
            failures.append((rnd, gate.overlapped, str(e)[:200]))
    assert not failures, failures


# ===================================================================================== graphs
def test_graphed_targets_and_metrics_beside_eager_calls(oracle):
    """instance + panoptic targets and the metric chain from the parts (PQ + mIoU, as bench.py
    replays it) captured after a warm-up on a side stream — so the capture makes the target
    workspace of its own stream and zeroes it inside the graph; 3 replays with new inputs copied
    into the static tensors, eager calls of the same shapes between them on the replay stream and
    on a side stream: every replay and eager call exact, the metric states the oracle's
    accumulation of every input.  (A workspace zeroed by hipMemsetAsync was not zeroed again on
    the second and later replays: the targets of those replays were wrong.)"""
    from nicr_mt_scene_analysis_amd import ops
    from nicr_mt_scene_analysis_amd.metric import MeanIntersectionOverUnion, PanopticQuality
    rng = np.random.default_rng(3)
    NC, B, H, W, sigma = 7, 2, 48, 64, 3
    is_thing = np.array([False, True, True, False, True, False, True])
    stuff = np.zeros((NC,), np.uint8)
    stuff[np.where(~is_thing)[0][1:]] = 1
    d_th, d_st = dev(is_thing.astype(np.uint8)), dev(stuff)
    s_sem = torch.zeros((B, H, W), dtype=torch.uint8, device='cuda')
    s_ins = torch.zeros((B, H, W), dtype=torch.int32, device='cuda')
    C, max_inst = 6, 1 << 16
    n = C + 1
    pq = PanopticQuality(n, 0, max_inst, 256 ** 3, [False] + [c < C // 2 for c in range(C)], device='cuda')
    miou = MeanIntersectionOverUnion(n, device='cuda')
    ref = PQRef(n, max_inst)
    parts0, d_tgt0, d_tsem0, _, _ = pq_inputs(rng, C, max_inst)
    s_parts = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in parts0.items()}
    s_tgt, s_tsem = d_tgt0.clone(), d_tsem0.clone()

    def step():
        r_i = ops.instance_targets(s_sem, s_ins, NC, d_th, d_st, sigma, True, max_instances=64)
        r_p = ops.panoptic_targets(s_sem, s_ins, NC, d_th, 1 << 16, 0, max_instances=64)
        pq.update_with_miou_parts(s_parts, s_tgt, miou, s_tsem, max_inst)
        return r_i, r_p

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    pq.reset()
    miou.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_i, out_p = step()
    torch.cuda.synchronize()            # (the graph holds the state tensors: no reset() from here on)

    def new_labels(seed):
        c = dict(NC=NC, B=B, H=H, W=W, max_inst=64, wire=True, ins_i64=False, kind='clean', what='both',
                 n_inst=10, sigma=sigma, normalized=True, seed=seed)
        r = np.random.default_rng(seed)
        sem, ins = label_maps(r, B, H, W, NC, c['n_inst'], 'clean')
        return c, sem, ins

    def check_targets(c, sem, ins, r_i, r_p):
        check_target_results(oracle, c, [('instance', r_i), ('panoptic', r_p)], sem, ins, is_thing, stuff)

    for rep in range(3):
        c, sem, ins = new_labels(900 + rep)
        parts, d_tgt, d_tsem, tgt, tsem = pq_inputs(rng, C, max_inst)
        s_sem.copy_(dev(sem))
        s_ins.copy_(dev(ins))
        for k in ('panoptic', 'semantic_idx_u8', 'instance', 'pan_of_inst', 'is_thing'):
            s_parts[k].copy_(parts[k])
        s_tgt.copy_(d_tgt)
        s_tsem.copy_(d_tsem)
        graph.replay()
        torch.cuda.synchronize()
        check_targets(c, sem, ins, out_i, out_p)
        ref.add(oracle, parts['panoptic'].cpu().numpy(), tgt, tsem)
        ref.check(pq, miou, ('replay', rep))
        for where in (None, side):      # eager calls of the same shapes: replay stream, side stream
            with ordered(where):
                c2, sem2, ins2 = new_labels(950 + 10 * rep + (where is not None))
                r_i = ops.instance_targets(dev(sem2), dev(ins2), NC, d_th, d_st, sigma, True, max_instances=64)
                r_p = ops.panoptic_targets(dev(sem2), dev(ins2), NC, d_th, 1 << 16, 0, max_instances=64)
                check_targets(c2, sem2, ins2, r_i, r_p)
                parts2, d_tgt2, d_tsem2, tgt2, tsem2 = pq_inputs(rng, C, max_inst)
                pq.update_with_miou_parts(parts2, d_tgt2, miou, d_tsem2, max_inst)
                torch.cuda.synchronize()
                ref.add(oracle, parts2['panoptic'].cpu().numpy(), tgt2, tsem2)
                ref.check(pq, miou, ('eager', rep, where is not None))
    _count('graph_replays', 3)


def test_graphed_pipeline_beside_eager_calls(oracle):
    """GraphedPanopticPipeline replayed 3 times with new inputs, eager pipeline calls of the same
    (B, C) between the replays on the replay stream and on a side stream: all exact vs the oracle,
    the vote tables clean"""
    from nicr_mt_scene_analysis_amd import ops
    from nicr_mt_scene_analysis_amd.graph import GraphedPanopticPipeline
    B, C, H, W = 2, 145, 24, 96
    base = dict(C=C, B=B, H=H, W=W, levels=2, p_tie=0.3, p_thing=0.9, p_far=0.0, specials=False,
                dtype='float32', thr=0.1, ksize=3, topk=255, apply_fg=False, dist_thr=None, normalized=True)
    first = make_wide_inputs(dict(base, n=30, seed=1))
    static = [dev(a) for a in first]
    pipe = GraphedPanopticPipeline(*static, top_k=255, want_score=True)
    side = torch.cuda.Stream()
    for rep in range(3):
        p = dict(base, n=[200, 5, 120][rep], seed=10 + rep)
        inputs = make_wide_inputs(p)[:3] + (first[3],)         # the graph's thing LUT
        for s, a in zip(static[:3], inputs[:3]):
            s.copy_(dev(a))
        out = pipe.replay()
        torch.cuda.synchronize()
        want = check_pipeline(oracle, p, max_centers=256, inputs=inputs)
        assert np.array_equal(out['panoptic'].cpu().numpy(), want['pan']), rep
        assert np.array_equal(out['instance'].cpu().numpy(), want['inst']), rep
        for where in (None, side):
            q = dict(base, n=[7, 255][where is not None], seed=100 + rep)
            qi = make_wide_inputs(q)
            qi = (qi[0], qi[1], qi[2], first[3])        # the graph's thing LUT
            with ordered(where):
                check_pipeline(oracle, q, max_centers=256, inputs=qi)
        assert_vote_tables_zero()


# ===================================================================================== evidence
def test_state_sequences_effective_cases():
    """runs last (file order): the draws reached the cases they are aimed at (each case is checked
    when a test that makes it ran)"""
    want = {'vote_table_recreated': 'pipeline', 'ragged_assign_with_reuse': 'pipeline',
            'workspace_two_sizes': 'targets', 'instance_panoptic_instance': 'targets',
            'status_then_clean': 'targets', 'pinned_slot_reused_before_read': 'postprocessing',
            'overlap_rounds': 'overlap'}
    missing = [k for k, by in want.items() if by in _RAN and not _EFFECTIVE.get(k)]
    if 'pq' in _RAN:
        pairs = {(a, b) for a in PQ_PATHS for b in PQ_PATHS if a != b}
        missing += [f'pq {a} -> {b}' for a, b in sorted(pairs - _PQ_PAIRS)]
    assert not missing, (missing, _EFFECTIVE)
