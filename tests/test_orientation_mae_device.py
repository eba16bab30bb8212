"""Orientation MAE on device tables: `utils.OrientationTable` / `utils.IdTable`, the kernels of
csrc/maae.hip behind `MeanAbsoluteAngularError` and `PanopticQualityWithOrientationMAE`, the tables
the postprocessing hands out and the task helpers' validation steps on them.

The yardstick of every device result is the host path of the same metric (the reference's loops
over Python dicts, unchanged).  The counts must be equal.  With N counted pairs the sums may differ
by N * 2^-52 * sum: the terms are non-negative float32 values widened to float64, so each of the
<= N - 1 additions of either order errs by <= 2^-53 of a partial sum <= the total."""
import math

import numpy as np
import pytest
import torch

from nicr_mt_scene_analysis_amd.testing import synthetic as syn

gpu = pytest.mark.gpu
RTOL = 1e-5                     # of tests/test_task_helpers.py, for the golden epoch logs
MAX_INST = 1 << 16
SPECIAL = (0.0, -0.0, math.pi, -math.pi, 2 * math.pi, -2 * math.pi, 7.0, -7.0)


def _tables():
    from nicr_mt_scene_analysis_amd.utils import IdTable, OrientationTable
    return IdTable, OrientationTable


# ------------------------------------------------------------------------------ CPU tier
def _dict_of(n, rng, high=65536):
    keys = sorted(rng.choice(high, size=n, replace=False).tolist())
    return {int(k): float(a) for k, a in zip(keys, rng.uniform(-7, 7, size=n))}


def test_orientation_table_round_trip_on_cpu():
    _, OrientationTable = _tables()
    rng = np.random.default_rng(0)
    dicts = [{}, _dict_of(1, rng), _dict_of(64, rng), _dict_of(65, rng),
             {65535: 0.1, 0: -0.0}, {np.int64(7): 1.5, np.int32(3): 2.5, np.uint16(65535): 1e-3}]
    t = OrientationTable.from_dicts(dicts, 'cpu')
    assert t.keys.dtype == torch.int32 and t.angle.dtype == torch.float32
    assert t.valid.dtype == torch.uint8 and t.n.dtype == torch.int32
    assert t.keys.shape == t.angle.shape == t.valid.shape == (6, 128)          # 65 keys -> 2 x 64
    assert t.n.tolist() == [0, 1, 64, 65, 2, 3] and t.status is None
    back = t.to_dicts()
    for want, got in zip(dicts, back):
        want = {int(k): float(np.float32(v)) for k, v in want.items()}           # float32-rounded
        assert got == want and list(got) == sorted(want)                         # ascending keys
        assert all(type(k) is int and type(v) is float for k, v in got.items())
    assert math.copysign(1.0, back[4][0]) == -1.0                                # -0.0 survives
    # K is padded to 64 and an empty batch of dicts still has columns
    assert OrientationTable.from_dicts([{}, {}], 'cpu').angle.shape == (2, 64)
    assert OrientationTable.from_dicts([_dict_of(64, rng)], 'cpu').angle.shape == (1, 64)


def test_orientation_table_rejects_keys_out_of_range_and_too_many():
    _, OrientationTable = _tables()
    with pytest.raises(ValueError):
        OrientationTable.from_dicts([{65536: 0.0}], 'cpu')
    with pytest.raises(ValueError):
        OrientationTable.from_dicts([{-1: 0.0}], 'cpu')
    with pytest.raises(ValueError):
        OrientationTable.from_dicts([{}, {k: 0.0 for k in range(4097)}], 'cpu')
    assert OrientationTable.from_dicts([{k: 0.0 for k in range(4096)}], 'cpu').n.tolist() == [4096]


def test_id_table_round_trip_on_cpu():
    IdTable, _ = _tables()
    dicts = [{}, {3 * MAX_INST + 2: 7, 2 * MAX_INST + 1: 300, 5: 0}, {i * MAX_INST + 1: i for i in range(65)}]
    t = IdTable.from_dicts(dicts, 'cpu')
    assert t.pan.dtype == torch.int64 and t.ins.dtype == torch.int64 and t.n.dtype == torch.int32
    assert t.pan.shape == (3, 128) and t.n.tolist() == [0, 3, 65] and t.ascending
    assert t.to_dicts() == dicts
    assert t.pan[1, :3].tolist() == sorted(dicts[1])                             # ascending rows
    merged = {'ids_pan': torch.tensor([[9, 4, 0]]), 'ids_ins': torch.tensor([[1, 2, 0]]),
              'n_ids': torch.tensor([2], dtype=torch.int32)}
    w = IdTable.from_merge(merged)
    assert w.pan is merged['ids_pan'] and w.ins is merged['ids_ins'] and w.n is merged['n_ids']
    assert not w.ascending and w.to_dicts() == [{9: 1, 4: 2}]


def test_header_and_binding_declare_the_entry_points():
    from nicr_mt_scene_analysis_amd import _lib, ops
    names = {'nmsa_maae_update_keyed', 'nmsa_maae_update_matched'}
    assert names <= set(_lib.declared_symbols()) and names <= set(_lib._SIGNATURES)
    assert len(_lib._SIGNATURES['nmsa_maae_update_keyed'][1]) == 17
    assert len(_lib._SIGNATURES['nmsa_maae_update_matched'][1]) == 30
    assert callable(ops.maae_update_keyed) and callable(ops.maae_update_matched)


# ------------------------------------------------------------------------------ GPU tier
def _dense_table(dicts):
    """what the uint8 prediction path hands out: key = column, 256 columns"""
    _, OrientationTable = _tables()
    angle = np.zeros((len(dicts), 256), np.float32)
    valid = np.zeros((len(dicts), 256), np.uint8)
    for b, d in enumerate(dicts):
        for k, a in d.items():
            angle[b, k], valid[b, k] = np.float32(a), 1
    return OrientationTable(None, torch.from_numpy(angle).cuda(), torch.from_numpy(valid).cuda(), None)


def _insertion_order_id_table(dicts):
    """an id table as the merge kernels leave it: insertion order, `ascending` False"""
    IdTable, _ = _tables()
    K = max(4, max(len(d) for d in dicts))
    pan = np.full((len(dicts), K), -5, np.int64)
    ins = np.full((len(dicts), K), -5, np.int64)
    for b, d in enumerate(dicts):
        pan[b, :len(d)], ins[b, :len(d)] = list(d.keys()), list(d.values())
    return IdTable.from_merge({'ids_pan': torch.from_numpy(pan).cuda(), 'ids_ins': torch.from_numpy(ins).cuda(),
                               'n_ids': torch.tensor([len(d) for d in dicts], dtype=torch.int32).cuda()})


def _assert_angular_states(dev_metric, host_metric, scale=1):
    n = int(host_metric.n_elements)
    assert int(dev_metric.n_elements) == scale * n
    want = scale * float(host_metric.sum_angular_error)
    got = float(dev_metric.sum_angular_error)
    print(f'pairs {scale * n}: device sum {got!r}, host sum {want!r}, |diff| {abs(got - want)!r}, '
          f'bound {scale * n * 2.0 ** -52 * want!r}')
    assert abs(got - want) <= scale * n * 2.0 ** -52 * want


def _mae():
    from nicr_mt_scene_analysis_amd.metric import MeanAbsoluteAngularError
    return MeanAbsoluteAngularError(device='cuda')


@gpu
@pytest.mark.parametrize('kind', ['dense', 'wide', 'dense_target'])
@pytest.mark.parametrize('lengths', [(0, 1, 64), (65, 0, 1)])
def test_keyed_update_against_the_host_path(kind, lengths):
    _, OrientationTable = _tables()
    rng = np.random.default_rng(sum(lengths))
    high = 65536 if kind == 'wide' else 256
    preds = [_dict_of(n, rng, high) for n in lengths]
    # the targets hold every predicted key and some more, with their own angles
    target = []
    for d in preds:
        extra = _dict_of(5, rng, high)
        target.append({k: float(rng.uniform(-7, 7)) for k in sorted(set(d) | set(extra))})
    host, dev = _mae(), _mae()
    host.update(preds, target)
    p = OrientationTable.from_dicts(preds, 'cuda') if kind == 'wide' else _dense_table(preds)
    t = _dense_table(target) if kind == 'dense_target' else OrientationTable.from_dicts(target, 'cuda')
    dev.update(p, t)
    assert int(host.n_elements) == sum(lengths)
    _assert_angular_states(dev, host)
    rad, deg = dev.compute()
    np.testing.assert_allclose(float(rad), float(host.compute()[0]), rtol=1e-12)
    # mixed arguments take the host path on the tables' dicts
    mixed = _mae()
    mixed.update(p, target)
    assert int(mixed.n_elements) == sum(lengths)
    assert float(mixed.sum_angular_error) == float(host.sum_angular_error)


@gpu
def test_keyed_update_without_any_pair_leaves_nan():
    _, OrientationTable = _tables()
    m = _mae()
    m.update(OrientationTable.from_dicts([{}, {}, {}], 'cuda'), OrientationTable.from_dicts([{1: 0.5}, {}, {}], 'cuda'))
    assert int(m.n_elements) == 0 and math.isnan(float(m.compute()[0]))          # 0 / 0, as the reference


@gpu
def test_per_pair_arithmetic_is_the_reference_chain_bit_for_bit():
    from nicr_mt_scene_analysis_amd import ops
    from nicr_mt_scene_analysis_amd.metric.mae import abs_angle_error_rad
    _, OrientationTable = _tables()
    rng = np.random.default_rng(11)
    pairs = [(p, t) for p in SPECIAL for t in SPECIAL]
    pairs += list(zip(rng.uniform(-2 * math.pi, 2 * math.pi, 200), rng.uniform(-2 * math.pi, 2 * math.pi, 200)))
    pairs += list(zip(rng.uniform(-100, 100, 100), rng.uniform(-100, 100, 100)))
    pairs += [(float(np.float32(k * math.pi)), float(np.float32(j * math.pi))) for k in range(-3, 4)
              for j in range(-3, 4)]
    pairs = [(float(a), float(b)) for a, b in pairs]
    N = len(pairs)
    # one table of N images with one pair each; update i sees image i alone and its own states
    p = OrientationTable.from_dicts([{3: a} for a, _ in pairs], 'cuda')
    t = OrientationTable.from_dicts([{3: b} for _, b in pairs], 'cuda')
    sums = torch.zeros(N, dtype=torch.float64, device='cuda')
    counts = torch.zeros(N, dtype=torch.int64, device='cuda')
    status = torch.zeros(1, dtype=torch.int32, device='cuda')

    def row(tab, i):
        return OrientationTable(tab.keys[i:i + 1], tab.angle[i:i + 1], tab.valid[i:i + 1], tab.n[i:i + 1])
    for i in range(N):
        ops.maae_update_keyed(sums[i], counts[i], status, row(p, i), row(t, i))
    want = torch.stack([abs_angle_error_rad(torch.tensor(a), torch.tensor(b)) for a, b in pairs])
    assert want.dtype == torch.float32
    got = sums.cpu()
    assert counts.cpu().tolist() == [1] * N and int(status) == 0
    assert (got.view(torch.int64) == want.double().view(torch.int64)).all(), \
        [(pairs[i], float(got[i]), float(want[i])) for i in (got != want.double()).nonzero().flatten().tolist()[:5]]


def _pq(capacity=None):
    from nicr_mt_scene_analysis_amd.metric import PanopticQualityWithOrientationMAE
    m = PanopticQualityWithOrientationMAE(num_categories=4, ignored_label=0, max_instances_per_category=MAX_INST,
                                          offset=256 ** 3, is_thing=[False, False, True, True], device='cuda')
    if capacity is not None:
        m._match_capacity = capacity
    return m


def _planted_scene():
    """three 40x60 image pairs and the dicts of both sides.  Image 0: identical maps of vertical
    strips — void (id 0), stuff, and things of which one target instance has no orientation, one
    predicted id is absent from the id dict, one predicted instance has no orientation ('count
    0'); image 1: nothing matches; image 2: 300 two-by-two things (more than 256 matches: several
    waves and loop iterations)."""
    rng = np.random.default_rng(5)
    H, W = 40, 60
    pred = np.zeros((3, H, W), np.int64)
    tgt = np.zeros((3, H, W), np.int64)
    thing = lambda c, i: c * MAX_INST + i                                        # noqa: E731
    # image 0: strips of 6 columns: void, stuff, things 1..8 (classes 2 / 3)
    strips = [0, 1 * MAX_INST] + [thing(2 + i % 2, 1 + i) for i in range(8)]
    for s, pid in enumerate(strips):
        pred[0, :, 6 * s:6 * s + 6] = pid
        tgt[0, :, 6 * s:6 * s + 6] = pid
    things0 = strips[2:]
    t_ids0 = {pid: 100 + i for i, pid in enumerate(things0)}                     # target instances 100..107
    p_ids0 = {pid: 1 + i for i, pid in reversed(list(enumerate(things0)))}       # descending: not sorted
    t_ids0[0] = 99
    p_ids0[0] = 9                     # id 0 is in every dict and table: only the skip keeps it out
    t_ori0 = {100 + i: float(rng.uniform(-7, 7)) for i in range(8)}
    p_ori0 = {1 + i: float(rng.uniform(-7, 7)) for i in range(8)}
    t_ori0[99], p_ori0[9] = 1.0, 2.0
    del t_ori0[101]                   # a target instance without orientation
    del p_ids0[things0[2]]            # a predicted id absent from the id dict
    del p_ori0[4]                     # a predicted instance without orientation
    # image 1: all stuff against one thing
    pred[1], tgt[1] = 1 * MAX_INST, thing(2, 1)
    # image 2: 300 2x2 things on a stuff background
    pred[2] = tgt[2] = 1 * MAX_INST
    ids2 = []
    for i in range(300):
        y, x = 2 * (i // 30), 2 * (i % 30)
        pred[2, y:y + 2, x:x + 2] = tgt[2, y:y + 2, x:x + 2] = thing(3, 1 + i)
        ids2.append(thing(3, 1 + i))
    t_ids2 = {pid: 1000 + i for i, pid in enumerate(ids2)}
    p_ids2 = {pid: 1 + i for i, pid in enumerate(ids2)}
    t_ori2 = {1000 + i: float(rng.uniform(-7, 7)) for i in range(300)}
    p_ori2 = {1 + i: float(rng.uniform(-7, 7)) for i in range(0, 300, 2)}        # every other one
    return {'pred': torch.from_numpy(pred).cuda(), 'target': torch.from_numpy(tgt).cuda(),
            'pred_ori': [p_ori0, {1: 0.3}, p_ori2], 'pred_ids': [p_ids0, {1 * MAX_INST: 1}, p_ids2],
            'target_ori': [t_ori0, {5: 0.2}, t_ori2], 'target_ids': [t_ids0, {thing(2, 1): 5}, t_ids2]}


@pytest.fixture(scope='module')
def scene():
    return _planted_scene()


def _scene_tables(s):
    IdTable, OrientationTable = _tables()
    return (OrientationTable.from_dicts(s['pred_ori'], 'cuda'), _insertion_order_id_table(s['pred_ids']),
            OrientationTable.from_dicts(s['target_ori'], 'cuda'), IdTable.from_dicts(s['target_ids'], 'cuda'))


def _update_host(m, s):
    m.update(s['pred'], s['pred_ori'], s['pred_ids'], s['target'], s['target_ori'], s['target_ids'])
    return m


def _update_device(m, s, tables=None):
    p_ori, p_ids, t_ori, t_ids = tables or _scene_tables(s)
    m.update(s['pred'], p_ori, p_ids, s['target'], t_ori, t_ids)
    return m


PQ_STATES = ('iou_per_class', 'tp_per_class', 'fn_per_class', 'fp_per_class')


@gpu
def test_matched_update_against_the_host_path(scene):
    host, dev = _update_host(_pq(), scene), _update_device(_pq(), scene)
    for name in PQ_STATES:
        assert torch.equal(getattr(dev, name), getattr(host, name)), name       # bit-equal
    # image 0: things 1..8 minus the three planted misses; image 2: every other of the 300
    assert int(host.n_elements) == 5 + 150
    _assert_angular_states(dev, host)
    assert float(dev.compute()['mae_rad']) == pytest.approx(float(host.compute()['mae_rad']), rel=1e-12)
    # a predicted instance whose table column is switched off ('count 0') instead of missing
    p_ori, p_ids, t_ori, t_ids = _scene_tables(scene)
    col = scene['pred_ori'][2]
    first = sorted(col)[0]
    p_ori.valid[2, 0] = 0
    less = dict(scene, pred_ori=scene['pred_ori'][:2] + [{k: v for k, v in col.items() if k != first}])
    host2, dev2 = _update_host(_pq(), less), _update_device(_pq(), scene, (p_ori, p_ids, t_ori, t_ids))
    assert int(host2.n_elements) == 5 + 149
    _assert_angular_states(dev2, host2)
    # a dense prediction table (ids below 256: images 0 and 1) against the same host path
    small = {k: v[:2] for k, v in scene.items()}
    tables = (_dense_table(small['pred_ori']),) + _scene_tables(small)[1:]
    host3, dev3 = _update_host(_pq(), small), _update_device(_pq(), small, tables)
    assert int(host3.n_elements) == 5
    _assert_angular_states(dev3, host3)


@gpu
def test_matched_kernel_on_hand_made_match_rows():
    """the join on a match table written by hand, against `update_mae` of the host path: target id
    0 (in every table: only the skip keeps it out), unknown ids on either side, an empty image"""
    from nicr_mt_scene_analysis_amd import ops
    IdTable, OrientationTable = _tables()
    rows = [[(0, 0), (17, 17), (19, 18), (20, 17), (17, 99), (21, 18)], [], [(30, 31)]]
    p_ori, p_ids = [{0: 0.1, 1: 0.5, 2: 2.0}, {}, {4: -3.0}], [{0: 0, 17: 1, 18: 2}, {}, {31: 4}]
    t_ori, t_ids = [{0: 0.2, 7: 1.0, 9: -6.5}, {}, {8: 3.0}], [{0: 0, 17: 7, 19: 8, 21: 9}, {}, {30: 8}]
    host = _pq()
    for b in range(3):
        host.update_mae(p_ori[b], p_ids[b], t_ori[b], t_ids[b], rows[b])
    assert int(host.n_elements) == 3
    cap = 8
    matches = torch.full((3, cap, 2), 17, dtype=torch.int64)                     # stale rows past n
    for b, r in enumerate(rows):
        if r:
            matches[b, :len(r)] = torch.tensor(r)
    dev = _pq()
    dev._pack()
    ops.maae_update_matched(dev.sum_angular_error, dev.n_elements, dev._status, matches.cuda(),
                            torch.tensor([len(r) for r in rows], dtype=torch.int32).cuda(),
                            _insertion_order_id_table(p_ids), OrientationTable.from_dicts(p_ori, 'cuda'),
                            IdTable.from_dicts(t_ids, 'cuda'), OrientationTable.from_dicts(t_ori, 'cuda'))
    _assert_angular_states(dev, host)
    assert int(dev._status) == 0


@gpu
def test_status_bits_raise_at_compute(scene):
    _, OrientationTable = _tables()
    m = _mae()
    m.update(OrientationTable.from_dicts([{3: 0.1, 4: 0.2}], 'cuda'), OrientationTable.from_dicts([{4: 0.0}], 'cuda'))
    assert int(m.n_elements) == 1                                                # the pair is skipped
    with pytest.raises(ValueError, match='missing in the target'):
        m.compute()
    m.compute()                                                                  # the word is cleared
    # more matches than the match table holds: the image contributes its first rows
    pq = _update_device(_pq(capacity=4), scene)
    assert 0 < int(pq.n_elements) <= 4 + 4
    with pytest.raises(ValueError, match='more matched segments per image than the match table holds'):
        pq.compute()


@gpu
def test_more_than_4096_wide_ids_raise():
    """65 x 64 pixels, every one its own instance: the smallest map that holds 4097 ids"""
    from nicr_mt_scene_analysis_amd.model.postprocessing import get_postprocessing_class
    _, OrientationTable = _tables()
    post = get_postprocessing_class('instance')()
    inst = torch.arange(1, 65 * 64 + 1, dtype=torch.int32).reshape(1, 65, 64).cuda()
    ori = torch.randn((1, 2, 65, 64), generator=torch.Generator().manual_seed(0)).cuda()
    table = post._get_instance_orientation_table(ori, inst, None)
    assert table.status is not None and table.keys.shape == (1, 4096)
    m = _mae()
    m.update(table, OrientationTable.from_dicts([{1: 0.0}], 'cuda'))
    with pytest.raises(ValueError, match='more than 4096 distinct instance ids'):
        m.compute()
    with pytest.raises(NotImplementedError, match='more than 4096 distinct instance ids in one image'):
        table.to_dicts()
    with pytest.raises(NotImplementedError, match='more than 4096 distinct instance ids in one image'):
        post._get_instance_orientation(ori, inst, None)
    # 4096 ids fit
    inst[0, 64:] = 0
    inst[0, 0, 0] = 0
    ok = post._get_instance_orientation(ori, inst, inst != 0)
    assert len(ok[0]) == 4095 and list(ok[0])[:2] == [2, 3]


@gpu
def test_two_runs_give_bit_identical_states(scene):
    a, b = _update_device(_pq(), scene), _update_device(_pq(), scene)
    for dtype, buf in a._pack().items():
        assert torch.equal(buf, b._pack()[dtype])
    rng = np.random.default_rng(2)
    _, OrientationTable = _tables()
    preds = [_dict_of(n, rng) for n in (700, 0, 65)]
    p = OrientationTable.from_dicts(preds, 'cuda')
    t = OrientationTable.from_dicts([{k: -v for k, v in d.items()} for d in preds], 'cuda')
    x, y = _mae(), _mae()
    x.update(p, t)
    y.update(p, t)
    assert int(x.n_elements) == 765
    assert float(x.sum_angular_error) == float(y.sum_angular_error) and int(x.n_elements) == int(y.n_elements)


@gpu
def test_update_with_tables_in_a_graph_on_a_side_stream(scene):
    """no host sync anywhere in the table path: it can be captured, and a replay adds again"""
    tables = _scene_tables(scene)
    once = _update_device(_pq(), scene, tables)
    n = int(once.n_elements)
    m = _update_device(_pq(), scene, tables)                                     # eager: packs the states
    m.reset()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _update_device(m, scene, tables)
    torch.cuda.synchronize()
    assert int(m.n_elements) == 0                                                # captured, not run
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(m.n_elements) == 3 * n
    want, got = 3 * float(once.sum_angular_error), float(m.sum_angular_error)
    print(f'3 replays: sum {got!r}, 3 x single {want!r}, bound {3 * n * 2.0 ** -52 * want!r}')
    assert abs(got - want) <= 3 * n * 2.0 ** -52 * want
    assert torch.equal(m.tp_per_class, 3 * once.tp_per_class)
    m.compute()                                                                  # no status bit


# ---- postprocessing and the task helpers on the reference's validation fixture -------------------
def _validation_case():
    from _golden import load, jload, ids_from_arrays
    from nicr_mt_scene_analysis_amd.data.preprocessing import APPLIED_PREPROCESSING_KEY
    from nicr_mt_scene_analysis_amd.model.postprocessing import get_postprocessing_class
    g = load('task_helper_cases')
    gt = {k[len('val__gt_'):]: g[k] for k in g.files if k.startswith('val__gt_')}
    B, H, W = gt['semantic'].shape
    is_thing_nc = tuple(bool(x) for x in g['val__is_thing_with_void'])
    C = len(is_thing_nc) - 1
    batch = _to_cuda(gt)
    for k in ('semantic', 'instance', 'panoptic'):
        batch[f'{k}_fullres'] = batch[k]
    batch['panoptic_ids_to_instance_dict'] = ids_from_arrays(
        g['val__pan_ids_n'], g['val__pan_ids_pan'], g['val__pan_ids_ins'])
    batch['orientations_present'] = [{int(k): v for k, v in d.items()}
                                     for d in jload(g['val__orientations_present'])]
    batch['rgb_fullres'] = torch.zeros((B, 3, H, W))
    batch[APPLIED_PREPROCESSING_KEY] = [[{'type': 'Resize', 'valid_region_slice_y': slice(0, H),
                                          'valid_region_slice_x': slice(0, W)}]] * B
    post = get_postprocessing_class('panoptic')(
        semantic_postprocessing=get_postprocessing_class('semantic')(),
        instance_postprocessing=get_postprocessing_class('instance')(),
        semantic_classes_is_thing=is_thing_nc[1:], semantic_class_has_orientation=is_thing_nc[1:])

    def predictions(step):
        logits, center, offset, ori = syn.make_predictions_from_targets(
            gt['semantic'], gt['instance_center'], gt['instance_offset'], gt['orientation'], C, seed=step)
        return ((_to_cuda(logits), (_to_cuda(center), _to_cuda(offset), _to_cuda(ori))),
                ((None, None), (None, None)))
    return g, batch, post, predictions, C, is_thing_nc


def _to_cuda(x):
    if isinstance(x, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()
    if isinstance(x, dict):
        return {k: _to_cuda(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_to_cuda(v) for v in x)
    return x


ORIENTATION_KEYS = ('orientations_gt_instance_gt_orientation_foreground',
                    'orientations_instance_segmentation_gt_orientation_foreground',
                    'orientations_panoptic_segmentation_deeplab_instance')


@gpu
def test_postprocessing_hands_out_tables_next_to_the_dicts():
    from nicr_mt_scene_analysis_amd import ops
    IdTable, OrientationTable = _tables()
    g, batch, post, predictions, C, _ = _validation_case()
    data = predictions(0)
    r = post.postprocess(data, batch, is_training=False)
    tables = r.aux['orientation_tables']
    assert sorted(tables.keys()) == sorted(ORIENTATION_KEYS)
    assert all(r.is_pending(k) and tables.is_pending(k) for k in ORIENTATION_KEYS)   # built when read
    for k in ORIENTATION_KEYS:
        t = tables[k]
        assert isinstance(t, OrientationTable) and t.angle.is_cuda
        assert type(r[k]) is list and t.to_dicts() == r[k] and any(len(d) for d in r[k]), k
        assert all(type(a) is float for d in r[k] for a in d.values())
    assert tables[ORIENTATION_KEYS[0]].keys is not None and tables[ORIENTATION_KEYS[0]].status is not None
    assert tables[ORIENTATION_KEYS[1]].keys is None                                  # uint8 ids: dense
    # the dicts are what the sums kernel + atan2 + one copy gave before the tables existed
    k = ORIENTATION_KEYS[1]
    s = ops.instance_orientation_sums(data[0][1][2], r['instance_segmentation_gt_foreground'].contiguous(),
                                      batch['orientation_foreground'])
    f = s['sums'].to(torch.float32)
    angle = torch.atan2(f[..., 1], f[..., 0]).to(torch.float64).cpu().tolist()
    count = s['count'].cpu().tolist()
    assert r[k] == [{i: angle[b][i] for i in range(1, 256) if count[b][i] > 0} for b in range(len(count))]
    ids = r.aux['panoptic_id_table']
    assert isinstance(ids, IdTable) and ids.to_dicts() == r['panoptic_segmentation_deeplab_ids']


@gpu
def test_validation_chain_on_tables_against_the_golden_logs_and_the_dict_path():
    from _golden import jload
    from nicr_mt_scene_analysis_amd.task_helper import InstanceTaskHelper, PanopticTaskHelper
    g, batch, post, predictions, C, is_thing_nc = _validation_case()
    dev = torch.device('cuda')
    helpers = {}
    for use_tables in (True, False):
        ins, pan = InstanceTaskHelper(C + 1, is_thing_nc), PanopticTaskHelper(C + 1, is_thing_nc, None)
        for h in (ins, pan):
            h.use_orientation_tables = use_tables
            h.initialize(dev)
        helpers[use_tables] = {'ins': ins, 'pan': pan}
    for step in range(2):
        for use_tables in (True, False):
            r = post.postprocess(predictions(step), batch, is_training=False)
            for h in helpers[use_tables].values():
                h.validation_step(batch, step, r)
            if use_tables:          # the table path has not built a single host object
                assert all(r.is_pending(k) for k in ORIENTATION_KEYS + ('panoptic_segmentation_deeplab_ids',))
    ins_t, pan_t = helpers[True]['ins'], helpers[True]['pan']
    ins_d, pan_d = helpers[False]['ins'], helpers[False]['pan']
    for t, d in ((ins_t._mae_gt, ins_d._mae_gt), (ins_t._mae_pq_deeplab, ins_d._mae_pq_deeplab),
                 (pan_t._mae_pq_deeplab, pan_d._mae_pq_deeplab)):
        assert int(d.n_elements) > 0
        _assert_angular_states(t, d)
    for name in PQ_STATES:
        assert torch.equal(getattr(pan_t._mae_pq_deeplab, name), getattr(pan_d._mae_pq_deeplab, name))
    for name, h in (('ins', ins_t), ('pan', pan_t)):
        _, _, logs = h.validation_epoch_end()
        keys, values = jload(g[f'val__{name}__log_keys']), g[f'val__{name}__log_values']
        scal = {k: v for k, v in logs.items() if not k.endswith('_time')}
        assert list(scal) == keys
        for k, v in zip(keys, values):
            np.testing.assert_allclose(float(scal[k]), v, rtol=RTOL, atol=1e-9, err_msg=f'{name}: {k}')
        assert any('mae' in k for k in keys)
