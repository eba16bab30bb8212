"""The surface-normal task — `ops.normal_valid_mask`, `ops.rmse_update`, `RootMeanSquaredError`,
`NormalPostprocessing`, `NormalTaskHelper` — against tests/golden/normal_task.npz
(tools/gen_golden_normal.py: the reference's own modules on CPU).

Bounds (none of them measured on the code under test):
  masks, counts, the full-resolution map     bit-identical / exact
  RMSE sum    |sum - truth64| <= 4 * 2^-24 * truth64, truth64 = float64 evaluation of the reference
              formula on the host: each float32 step of subtract, square, three-term add, divide
              and square root contributes at most one unit roundoff to a non-negative quantity and
              the square root halves what precedes it; the float64 accumulation adds nothing at
              these sizes
  compute()   within e_ref / n + one float32 ulp of the fixture's compute() (e_ref: the reference's
              own error of the sum against the float64 truth)
  losses      rtol 1e-5; gradients rtol 1e-5 / atol 1e-7 — the tolerances of tests/test_losses.py
              for `masked_sum` of the same kinds
"""
import os
import socket

import numpy as np
import pytest
import torch

from _golden import load, jload
from nicr_mt_scene_analysis_amd.testing import synthetic as syn

CASES = ('same', 'up', 'holes', 'wide')
RMSE_RTOL = 4 * 2.0 ** -24
LOSS_RTOL = 1e-5
GRAD_TOL = dict(rtol=1e-5, atol=1e-7)
_CACHE = {}


def _case(name):
    """regenerated inputs (digest-checked: a mismatch FAILS), recipe, fixture"""
    if name not in _CACHE:
        g = load('normal_task')
        p = jload(g[f'{name}__params'])
        inp = syn.make_normal_inputs(p['recipe'], p['seed'])
        assert syn.input_digest(*(inp[k] for k in sorted(inp))) == p['digest'], \
            f'{name}: regenerated inputs differ from the fixture generator\'s'
        _CACHE[name] = (inp, syn.NORMAL_RECIPES[name], g)
    return _CACHE[name]


def _valid_np(target):
    return ~((target[:, 0] == 0) & (target[:, 1] == 0) & (target[:, 2] == 0))


def _fullres_np(pred, recipe):
    """crop + F.interpolate(mode='nearest') on the host: the materialised map"""
    _, _, crop, full, _ = recipe
    x = torch.from_numpy(pred)[..., crop[0]:crop[1], crop[2]:crop[3]]
    if tuple(x.shape[-2:]) != tuple(full):
        x = torch.nn.functional.interpolate(x, size=full, mode='nearest')
    return x.numpy()


def _truth64(pred_full, target, mask):
    d = pred_full.astype(np.float64) - target.astype(np.float64)
    px = np.sqrt((d * d).mean(axis=1))
    return float(px[mask].sum()) if mask is not None else float(px.sum())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _batch(inp, recipe, device='cuda'):
    from nicr_mt_scene_analysis_amd.data.preprocessing import APPLIED_PREPROCESSING_KEY
    B, _, crop, _, scales = recipe
    batch = {'normal': torch.from_numpy(inp['target_s1']).to(device),
             'normal_fullres': torch.from_numpy(inp['target_fullres']).to(device),
             APPLIED_PREPROCESSING_KEY: [[{'type': 'Resize',
                                           'valid_region_slice_y': slice(crop[0], crop[1]),
                                           'valid_region_slice_x': slice(crop[2], crop[3])}]] * B}
    for s in scales[1:]:
        batch[f'_down_{s}'] = {'normal': torch.from_numpy(inp[f'target_s{s}']).to(device)}
    return batch


def _slices(recipe):
    crop = recipe[2]
    return slice(crop[0], crop[1]), slice(crop[2], crop[3])


def _masks(inp):
    """name -> (mask argument of update, mask argument of update_from_network_resolution, numpy mask)"""
    derived = _valid_np(inp['target_fullres'])
    return {'derived': (derived, 'target', derived), 'none': (None, None, None),
            'given': (inp['metric_mask'], inp['metric_mask'], inp['metric_mask'])}


# ------------------------------------------------------------------------------------ CPU tier
def test_imports_and_exports():
    from nicr_mt_scene_analysis_amd import metric, ops, task_helper
    from nicr_mt_scene_analysis_amd.model import postprocessing
    from nicr_mt_scene_analysis_amd.model.postprocessing.dense_base import DensePostprocessingBase
    assert issubclass(metric.RootMeanSquaredError, metric.Metric)
    assert issubclass(postprocessing.NormalPostprocessing, DensePostprocessingBase)
    assert issubclass(task_helper.NormalTaskHelper, task_helper.TaskHelperBase)
    assert callable(ops.normal_valid_mask) and callable(ops.rmse_update)
    from nicr_mt_scene_analysis_amd import _lib
    assert {'nmsa_normal_valid_mask', 'nmsa_rmse_update'} <= set(_lib.declared_symbols())
    assert {'nmsa_normal_valid_mask', 'nmsa_rmse_update'} <= set(_lib._SIGNATURES)


def test_training_pass_through_on_cpu_tensors():
    from nicr_mt_scene_analysis_amd.model.postprocessing import NormalPostprocessing
    out, side = torch.randn(1, 3, 4, 4), (torch.randn(1, 3, 2, 2),)
    r = NormalPostprocessing(unknown_kwarg=1).postprocess((out, side), {}, is_training=True)
    assert type(r) is dict and list(r) == ['normal_output', 'normal_side_outputs']
    assert r['normal_output'] is out and r['normal_side_outputs'] is side


def test_rmse_states_and_reset():
    from nicr_mt_scene_analysis_amd.metric import RootMeanSquaredError
    m = RootMeanSquaredError(device='cpu')
    assert m.state_names() == ['sum_root_mean_squared_error', 'n_observations']
    assert m.sum_root_mean_squared_error.dtype == torch.float64 and m.sum_root_mean_squared_error.ndim == 0
    assert m.n_observations.dtype == torch.int64 and m.n_observations.ndim == 0
    assert m._state_reduce == {'sum_root_mean_squared_error': 'sum', 'n_observations': 'sum'}
    assert torch.isnan(m.compute()) and m.compute().dtype == torch.float32       # 0 / 0
    m.sum_root_mean_squared_error += 3.0
    m.n_observations += 4
    assert float(m.compute()) == 0.75
    m.reset()
    assert float(m.sum_root_mean_squared_error) == 0 and int(m.n_observations) == 0
    from nicr_mt_scene_analysis_amd._lib import NmsaError
    with pytest.raises(NmsaError):
        m.update(torch.zeros(1, 3, 2, 2), torch.zeros(1, 3, 2, 2))


def test_helper_constructor():
    from nicr_mt_scene_analysis_amd.task_helper import NormalTaskHelper
    with pytest.raises(AssertionError):
        NormalTaskHelper('focal')
    h = NormalTaskHelper('l1', disable_multiscale_supervision=True)
    h.initialize(torch.device('cpu'))
    artifacts, examples, logs = h.validation_epoch_end()
    assert artifacts == {} and examples == {} and torch.isnan(logs['normal_rmse'])


def _gloo_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from nicr_mt_scene_analysis_amd.metric import RootMeanSquaredError
    m = RootMeanSquaredError(device='cpu')
    m.sum_root_mean_squared_error += 1.5 * (rank + 1)
    m.n_observations += 10 * (rank + 1)
    value = float(m.compute())                       # summed over the ranks inside compute()
    local = (float(m.sum_root_mean_squared_error), int(m.n_observations))
    with open(os.path.join(out_dir, f'rank{rank}.txt'), 'w') as f:
        f.write(repr((value, local)))
    dist.destroy_process_group()


def test_rmse_world2_gloo_sum(tmp_path):
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    mp.spawn(_gloo_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    for rank in range(2):
        value, local = eval((tmp_path / f'rank{rank}.txt').read_text())
        assert value == float(np.float32(4.5 / 30))
        assert local == (1.5 * (rank + 1), 10 * (rank + 1))      # rank-local again behind compute()


def test_cpu_tensor_and_dtype_errors():
    from nicr_mt_scene_analysis_amd import ops
    from nicr_mt_scene_analysis_amd._lib import NmsaError
    with pytest.raises(NmsaError):
        ops.normal_valid_mask(torch.zeros(1, 3, 4, 4))
    with pytest.raises(TypeError):
        ops.normal_valid_mask(torch.zeros(1, 3, 4, 4, dtype=torch.float16))
    s, n = torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.int64)
    with pytest.raises(NmsaError):
        ops.rmse_update(s, n, torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4))
    with pytest.raises(TypeError):
        ops.rmse_update(s, n, torch.zeros(1, 3, 4, 4, dtype=torch.float64), torch.zeros(1, 3, 4, 4))
    with pytest.raises(TypeError):
        ops.rmse_update(s, n, torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4, dtype=torch.float16))


@pytest.mark.parametrize('name', CASES)
def test_fixture_self_check(name):
    inp, recipe, g = _case(name)
    B, net, crop, full, scales = recipe
    for s in scales:
        mask = np.unpackbits(g[f'{name}__s{s}__mask'])[:B * (net[0] // s) * (net[1] // s)]
        assert int(mask.sum()) == int(g[f'{name}__s{s}__count']) > 0
        assert np.array_equal(mask.astype(bool), _valid_np(inp[f'target_s{s}']).reshape(-1))
    pred_full = _fullres_np(inp['pred_s1'], recipe)
    assert np.array_equal(pred_full.reshape(-1)[g[f'{name}__fullres_sample']], g[f'{name}__fullres_px'])
    for tag, (_, _, mask) in _masks(inp).items():
        st = jload(g[f'{name}__rmse__{tag}'])
        truth = _truth64(pred_full, inp['target_fullres'], mask)
        assert abs(st['sum'] - truth) <= st['e_ref'] * (1 + 1e-9) + 1e-12
        assert st['n'] == (int(mask.sum()) if mask is not None else mask_size(inp))
        assert st['e_ref'] <= RMSE_RTOL * truth          # the reference itself meets the bound
    if name == 'holes':
        t = inp['target_fullres']
        assert not _valid_np(t)[0].any() and np.signbit(t[0]).any()
        partial = _valid_np(t) & ((t == 0).sum(axis=1) > 0)
        assert partial.any()


def mask_size(inp):
    return inp['target_fullres'].shape[0] * inp['target_fullres'].shape[2] * inp['target_fullres'].shape[3]


# ------------------------------------------------------------------------------------ GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_valid_masks_bit_identical(name):
    from nicr_mt_scene_analysis_amd import ops
    inp, recipe, g = _case(name)
    for s in recipe[4]:
        t = inp[f'target_s{s}']
        mask = ops.normal_valid_mask(_dev(t))
        assert mask.dtype == torch.bool and tuple(mask.shape) == (t.shape[0],) + t.shape[2:]
        assert np.array_equal(np.packbits(mask.cpu().numpy().reshape(-1)), g[f'{name}__s{s}__mask'])
    t = inp['target_fullres']
    assert np.array_equal(ops.normal_valid_mask(_dev(t)).cpu().numpy(), _valid_np(t))
    # an unaligned view of the same data takes the per-pixel loads
    flat = torch.zeros(t.size + 1, dtype=torch.float32, device='cuda')
    flat[1:] = _dev(t).reshape(-1)
    assert np.array_equal(ops.normal_valid_mask(flat[1:].view(t.shape)).cpu().numpy(), _valid_np(t))


@pytest.mark.gpu
def test_nan_channel_is_valid():
    from nicr_mt_scene_analysis_amd import ops
    inp, _, _ = _case('holes')
    t = inp['target_fullres'].copy()
    assert not _valid_np(t)[0, 3, 5]
    t[0, 1, 3, 5] = np.nan
    t[0, 2, 4, 4] = np.nan
    got = ops.normal_valid_mask(_dev(t)).cpu().numpy()
    assert got[0, 3, 5] and got[0, 4, 4]
    assert np.array_equal(got, _valid_np(t))


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_postprocessing_inference(name):
    from nicr_mt_scene_analysis_amd.model.postprocessing import NormalPostprocessing
    inp, recipe, g = _case(name)
    pred = _dev(inp['pred_s1'])
    sides = tuple(_dev(inp[f'pred_s{s}']) for s in recipe[4][1:])
    r = NormalPostprocessing().postprocess((pred, sides), _batch(inp, recipe), is_training=False)
    assert list(r.keys()) == jload(g[f'{name}__keys'])
    assert r['normal_output'] is pred and r['normal_side_outputs'] is sides
    resized = tuple(recipe[3]) != (recipe[2][1] - recipe[2][0], recipe[2][3] - recipe[2][2])
    assert r.is_pending('normal_output_fullres') == resized
    full = r['normal_output_fullres']
    assert not r.is_pending('normal_output_fullres')
    assert tuple(full.shape) == (recipe[0], 3) + tuple(recipe[3]) and full.dtype == torch.float32
    assert np.array_equal(full.cpu().numpy().reshape(-1)[g[f'{name}__fullres_sample']],
                          g[f'{name}__fullres_px'])
    assert np.array_equal(full.cpu().numpy(), _fullres_np(inp['pred_s1'], recipe))
    if name == 'same':
        assert full.data_ptr() == pred.data_ptr() and full.shape == pred.shape      # a view
    src, crop = r.aux['normal_output_fullres_source']
    assert src is pred and crop == _slices(recipe)


@pytest.mark.gpu
def test_postprocessing_half_precision_output():
    from nicr_mt_scene_analysis_amd.model.postprocessing import NormalPostprocessing
    inp, recipe, _ = _case('up')
    for dtype in (torch.bfloat16, torch.float16):
        pred = _dev(inp['pred_s1']).to(dtype)
        r = NormalPostprocessing().postprocess((pred, None), _batch(inp, recipe), is_training=False)
        want = _fullres_np(pred.float().cpu().numpy(), recipe)
        assert r['normal_output_fullres'].dtype == dtype
        assert np.array_equal(r['normal_output_fullres'].float().cpu().numpy(), want)


def _metric():
    from nicr_mt_scene_analysis_amd.metric import RootMeanSquaredError
    return RootMeanSquaredError(device=torch.device('cuda'))


def _paths(inp, recipe, tag):
    """name -> callable(metric): the materialised-map update and the network-resolution update"""
    from nicr_mt_scene_analysis_amd import ops
    m_update, m_fused, _ = _masks(inp)[tag]
    pred, target = _dev(inp['pred_s1']), _dev(inp['target_fullres'])
    full = ops.resize_nearest(pred, recipe[3], _slices(recipe))
    as_dev = (lambda m: _dev(m) if isinstance(m, np.ndarray) else m)
    return {'update': lambda m: m.update(full, target, as_dev(m_update)),
            'fused': lambda m: m.update_from_network_resolution(pred, _slices(recipe), target,
                                                                mask=as_dev(m_fused))}


@pytest.mark.gpu
@pytest.mark.parametrize('tag', ('derived', 'none', 'given'))
@pytest.mark.parametrize('name', CASES)
def test_rmse_all_paths(name, tag):
    inp, recipe, g = _case(name)
    st = jload(g[f'{name}__rmse__{tag}'])
    mask = _masks(inp)[tag][2]
    truth = _truth64(_fullres_np(inp['pred_s1'], recipe), inp['target_fullres'], mask)
    sums = {}
    for path, update in _paths(inp, recipe, tag).items():
        m = _metric()
        update(m)
        s, n = float(m.sum_root_mean_squared_error), int(m.n_observations)
        print(f'{name}/{tag}/{path}: sum {s!r} truth64 {truth!r} rel {abs(s - truth) / truth:.3e} n {n}')
        assert n == st['n']
        assert abs(s - truth) <= RMSE_RTOL * truth
        value = m.compute()
        assert value.dtype == torch.float32
        ulp = float(np.spacing(np.float32(st['compute'])))
        assert abs(float(value) - st['compute']) <= st['e_ref'] / st['n'] + ulp
        sums[path] = s
        update(m)                                            # two updates accumulate
        assert int(m.n_observations) == 2 * n
        assert abs(float(m.sum_root_mean_squared_error) - 2 * truth) <= RMSE_RTOL * 2 * truth
        m.reset()
        assert int(m.n_observations) == 0 and torch.isnan(m.compute())
    assert abs(sums['update'] - sums['fused']) <= 2 * RMSE_RTOL * truth


@pytest.mark.gpu
def test_all_invalid_image_contributes_nothing():
    inp, recipe, _ = _case('holes')
    pred, target = inp['pred_s1'], inp['target_fullres']
    assert not _valid_np(target)[0].any()
    whole, rest = _metric(), _metric()
    whole.update_from_network_resolution(_dev(pred), _slices(recipe), _dev(target))
    rest.update_from_network_resolution(_dev(pred[1:]), _slices(recipe), _dev(target[1:]))
    assert int(whole.n_observations) == int(rest.n_observations) == int(_valid_np(target)[1:].sum())
    truth = _truth64(_fullres_np(pred[1:], recipe), target[1:], _valid_np(target[1:]))
    for m in (whole, rest):
        assert abs(float(m.sum_root_mean_squared_error) - truth) <= RMSE_RTOL * truth
    # what the masked-out pixels predict is irrelevant, a NaN included
    poisoned = pred.copy()
    poisoned[0] = np.nan
    m = _metric()
    m.update_from_network_resolution(_dev(poisoned), _slices(recipe), _dev(target))
    assert abs(float(m.sum_root_mean_squared_error) - truth) <= RMSE_RTOL * truth


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float16))
def test_rmse_half_precision_predictions(dtype):
    """the prediction is widened to float32 before the subtraction, as torch's type promotion does"""
    inp, recipe, _ = _case('up')
    pred = _dev(inp['pred_s1']).to(dtype)
    target = inp['target_fullres']
    mask = _valid_np(target)
    truth = _truth64(_fullres_np(pred.float().cpu().numpy(), recipe), target, mask)
    from nicr_mt_scene_analysis_amd import ops
    fused, plain = _metric(), _metric()
    fused.update_from_network_resolution(pred, _slices(recipe), _dev(target))
    full = ops.resize_nearest(pred.view(torch.int16), recipe[3], _slices(recipe)).view(dtype)
    plain.update(full, _dev(target), _dev(mask))
    for m in (fused, plain):
        assert int(m.n_observations) == int(mask.sum())
        assert abs(float(m.sum_root_mean_squared_error) - truth) <= RMSE_RTOL * truth


@pytest.mark.gpu
def test_rmse_other_channel_counts():
    """C = 1 and C = 8 (the ends of the supported range), odd plane size"""
    g = torch.Generator().manual_seed(3)
    for C in (1, 8):
        pred, target = torch.randn((2, C, 5, 7), generator=g), torch.randn((2, C, 5, 7), generator=g)
        m = _metric()
        m.update(pred.cuda(), target.cuda())
        truth = _truth64(pred.numpy(), target.numpy(), None)
        assert int(m.n_observations) == 70
        assert abs(float(m.sum_root_mean_squared_error) - truth) <= RMSE_RTOL * truth
    from nicr_mt_scene_analysis_amd._lib import NmsaError
    with pytest.raises((NmsaError, ValueError)):
        _metric().update(torch.zeros(1, 9, 2, 2).cuda(), torch.zeros(1, 9, 2, 2).cuda())


@pytest.mark.gpu
def test_rmse_update_in_a_graph_on_a_side_stream():
    inp, recipe, _ = _case('up')
    pred, target = _dev(inp['pred_s1']), _dev(inp['target_fullres'])
    mask = _valid_np(inp['target_fullres'])
    truth = _truth64(_fullres_np(inp['pred_s1'], recipe), inp['target_fullres'], mask)
    m = _metric()
    m.update_from_network_resolution(pred, _slices(recipe), target)          # eager
    eager_n = int(m.n_observations)
    m.reset()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        m.update_from_network_resolution(pred, _slices(recipe), target)
    torch.cuda.synchronize()
    assert int(m.n_observations) == 0                                        # captured, not run
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert int(m.n_observations) == 2 * eager_n == 2 * int(mask.sum())
    assert abs(float(m.sum_root_mean_squared_error) - 2 * truth) <= RMSE_RTOL * 2 * truth


def _helper(loss_name, no_ms):
    from nicr_mt_scene_analysis_amd.task_helper import NormalTaskHelper
    h = NormalTaskHelper(loss_name, disable_multiscale_supervision=no_ms)
    h.initialize(torch.device('cuda'))
    return h


def _training_post(inp, recipe):
    from nicr_mt_scene_analysis_amd.model.postprocessing import NormalPostprocessing
    scales = recipe[4]
    preds = {s: _dev(inp[f'pred_s{s}']).requires_grad_(True) for s in scales}
    post = NormalPostprocessing().postprocess((preds[1], tuple(preds[s] for s in scales[1:])),
                                              {}, is_training=True)
    return preds, post


@pytest.mark.gpu
@pytest.mark.parametrize('speculative', (True, False))
@pytest.mark.parametrize('tag', ('ms', 'main'))
@pytest.mark.parametrize('loss_name', ('mse', 'l1'))
@pytest.mark.parametrize('name', CASES)
def test_losses_and_gradients(monkeypatch, name, loss_name, tag, speculative):
    from nicr_mt_scene_analysis_amd.loss import _functional as F_
    if not speculative:
        monkeypatch.setattr(F_, '_SPECULATE', False)
    inp, recipe, g = _case(name)
    scales = recipe[4] if tag == 'ms' else recipe[4][:1]
    want = jload(g[f'{name}__{loss_name}__{tag}__losses'])
    preds, post = _training_post(inp, recipe)
    helper = _helper(loss_name, tag == 'main')
    losses, logs = helper.training_step(_batch(inp, recipe), 0, post)
    assert list(losses) == list(want)
    for k, v in want.items():
        np.testing.assert_allclose(float(losses[k]), v, rtol=LOSS_RTOL, err_msg=k)
        np.testing.assert_allclose(float(logs[k]), v, rtol=LOSS_RTOL, err_msg=k)
    assert sorted(logs) == jload(g[f'{name}__log_keys'])[f'training_{tag}']
    losses['normal_total_loss'].backward()
    for s in scales:
        grad = preds[s].grad.cpu().numpy()
        np.testing.assert_allclose(grad.reshape(-1)[g[f'{name}__grad_sample_s{s}']],
                                   g[f'{name}__{loss_name}__{tag}__grad_s{s}'], **GRAD_TOL)
        invalid = ~_valid_np(inp[f'target_s{s}'])
        assert (grad.transpose(0, 2, 3, 1)[invalid] == 0).all()      # exactly zero at invalid pixels
    for s in recipe[4]:
        if s not in scales:
            assert preds[s].grad is None


@pytest.mark.gpu
def test_scale_without_a_valid_pixel_is_nan_and_leaves_the_total():
    """what the helper's docstring states: the scale's key is 0 / 0 = NaN, the total is finite"""
    inp, recipe, _ = _case('same')
    inp = dict(inp)
    inp['target_s4'] = np.zeros_like(inp['target_s4'])
    for requires_grad in (True, False):
        preds, post = _training_post(inp, recipe)
        helper = _helper('mse', False)
        with torch.set_grad_enabled(requires_grad):
            losses, _ = helper.training_step(_batch(inp, recipe), 0, post)
        assert torch.isnan(losses['normal_loss_down_4'])
        assert torch.isfinite(losses['normal_loss_main']) and torch.isfinite(losses['normal_total_loss'])


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_task_helper_validation_end_to_end(name):
    from nicr_mt_scene_analysis_amd.model.postprocessing import NormalPostprocessing
    inp, recipe, g = _case(name)
    st = jload(g[f'{name}__rmse__derived'])
    want_losses = jload(g[f'{name}__mse__ms__losses'])
    log_keys = jload(g[f'{name}__log_keys'])
    batch = _batch(inp, recipe)
    pred = _dev(inp['pred_s1'])
    sides = tuple(_dev(inp[f'pred_s{s}']) for s in recipe[4][1:])
    lazy = NormalPostprocessing().postprocess((pred, sides), batch, is_training=False)
    plain = {k: lazy[k] for k in lazy.keys()}               # no .aux: the materialised map
    ulp = float(np.spacing(np.float32(st['compute'])))
    for post in (lazy, plain):
        helper = _helper('mse', False)
        with torch.no_grad():
            losses, logs = helper.validation_step(batch, 0, post)
        assert sorted(logs) == log_keys['validation']
        for k, v in want_losses.items():
            np.testing.assert_allclose(float(losses[k]), v, rtol=LOSS_RTOL, err_msg=k)
        assert int(helper._metric_rmse.n_observations) == st['n']
        artifacts, examples, epoch_logs = helper.validation_epoch_end()
        assert artifacts == {} and examples == {} and sorted(epoch_logs) == log_keys['epoch_end']
        assert abs(float(epoch_logs['normal_rmse']) - st['compute']) <= st['e_ref'] / st['n'] + ulp
        assert int(helper._metric_rmse.n_observations) == 0                  # reset afterwards
        assert float(helper._metric_rmse.sum_root_mean_squared_error) == 0.0


def _f32_chain(pred, target):
    """the kernel's per-pixel arithmetic in numpy float32, every step one IEEE rounding: subtract,
    square, sequential channel sum, divide by C, square root -> float32 [B,H,W]"""
    f32 = np.float32
    d = (pred.astype(f32) - target.astype(f32)).astype(f32)
    sq = (d * d).astype(f32)
    s = np.zeros_like(sq[:, 0])
    for c in range(sq.shape[1]):
        s = (s + sq[:, c]).astype(f32)
    return np.sqrt((s / f32(sq.shape[1])).astype(f32)).astype(f32)


@pytest.mark.gpu
@pytest.mark.parametrize('C', (1, 3))
def test_rmse_per_pixel_arithmetic_is_correctly_rounded(C):
    """Every per-pixel step is one IEEE rounding, the square root included: the state equals the
    sum of numpy's float32 chain BIT FOR BIT.  The roots lie in [2^-7, 8) (ulp >= 2^-30) and a
    chunk of 512 of them sums to less than 2^12, so the float64 sum of a chunk is exact in any
    order (42 bits) and a single root that is off by one float32 ulp changes it.  16 chunks, each
    its own update, so that two opposite errors cannot cancel unseen across the whole set."""
    rng = np.random.default_rng(77)
    H, W, chunks = 16, 32, 16
    mag = np.exp2(rng.uniform(-6.0, 2.0, (chunks, C, H, W))).astype(np.float32)
    sign = np.where(rng.random((chunks, C, H, W)) < 0.5, -1.0, 1.0).astype(np.float32)
    target = rng.standard_normal((chunks, C, H, W), dtype=np.float32)
    pred = (target + sign * mag).astype(np.float32)
    want_px = _f32_chain(pred, target)
    assert want_px.min() >= 2.0 ** -7 and want_px.max() < 8.0
    pred_d, target_d = _dev(pred), _dev(target)
    wrong = []
    for i in range(chunks):
        m = _metric()
        m.update(pred_d[i:i + 1], target_d[i:i + 1])
        want = float(want_px[i].astype(np.float64).sum())
        got = float(m.sum_root_mean_squared_error)
        assert int(m.n_observations) == H * W
        if got != want:
            wrong.append((i, got, want, (got - want) / 2.0 ** -30))
    print(f'C={C}: chunks that differ from the float32 chain: {wrong}')
    assert not wrong


@pytest.mark.gpu
@pytest.mark.parametrize('shift', ('pred', 'target', 'mask'))
def test_rmse_unaligned_pointers_take_the_per_pixel_loads(shift):
    """H*W % 4 == 0 but one pointer is off its 16-byte (mask: 4-byte) boundary: the per-pixel-load
    variants, same bits as the aligned call"""
    inp, recipe, _ = _case('holes')

    def off_by_one(t):
        flat = torch.zeros(t.numel() + 1, dtype=t.dtype, device='cuda')
        flat[1:] = t.reshape(-1)
        view = flat[1:].view(t.shape)
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        return view

    target = _dev(inp['target_fullres'])
    pred = _dev(_fullres_np(inp['pred_s1'], recipe))
    mask = _dev(inp['metric_mask'])
    aligned = _metric()
    aligned.update(pred, target, mask)
    if shift == 'pred':
        pred = off_by_one(pred)
    elif shift == 'target':
        target = off_by_one(target)
    else:
        mask = off_by_one(mask)
    m = _metric()
    m.update(pred, target, mask)
    assert int(m.n_observations) == int(aligned.n_observations) == int(inp['metric_mask'].sum())
    truth = _truth64(_fullres_np(inp['pred_s1'], recipe), inp['target_fullres'], inp['metric_mask'])
    assert abs(float(m.sum_root_mean_squared_error) - truth) <= RMSE_RTOL * truth
    # network-resolution source with an unaligned target / source
    fused = _metric()
    src = _dev(inp['pred_s1'])
    fused.update_from_network_resolution(off_by_one(src) if shift == 'pred' else src, _slices(recipe),
                                         target, mask=mask)
    assert int(fused.n_observations) == int(aligned.n_observations)
    assert abs(float(fused.sum_root_mean_squared_error) - truth) <= RMSE_RTOL * truth


@pytest.mark.gpu
def test_whole_map_crop_at_equal_resolution_reads_like_update():
    """`update_from_network_resolution` with nothing to crop or resize takes the direct source mode:
    the same bits as `update`"""
    inp, recipe, _ = _case('same')
    pred, target = _dev(inp['pred_s1']), _dev(inp['target_fullres'])
    a, b = _metric(), _metric()
    a.update(pred, target, _dev(_valid_np(inp['target_fullres'])))
    b.update_from_network_resolution(pred, _slices(recipe), target)
    assert int(a.n_observations) == int(b.n_observations)
    assert float(a.sum_root_mean_squared_error) == float(b.sum_root_mean_squared_error)
