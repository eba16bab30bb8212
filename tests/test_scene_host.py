"""CPU tier of the scene task: exports, construction without a device, the key names against
the fixture's recorded key lists (tests/golden/scene_task.npz), the unchanged factory."""
import numpy as np
import pytest
import torch

from _golden import load, jload


def test_exports():
    from nicr_mt_scene_analysis_amd import _lib, loss, metric, ops, task_helper
    from nicr_mt_scene_analysis_amd.model import postprocessing
    assert issubclass(metric.ConfusionMatrix, metric.Metric)
    assert issubclass(postprocessing.ScenePostprocessing, postprocessing.PostprocessingBase)
    assert issubclass(task_helper.SceneTaskHelper, task_helper.TaskHelperBase)
    assert issubclass(loss.CrossEntropyLossScene, torch.nn.Module)
    assert callable(ops.scene_step)
    # the two constants mirror include/nmsa.h
    header = open(_lib.HEADER_PATH).read()
    assert f'#define NMSA_SCENE_MAX_CLASSES {_lib.NMSA_SCENE_MAX_CLASSES}\n' in header
    assert f'#define NMSA_ST_VALUE_RANGE {_lib.NMSA_ST_VALUE_RANGE}\n' in header
    assert 'nmsa_scene_step' in _lib.declared_symbols() and 'nmsa_scene_step' in _lib._SIGNATURES


def test_factory_still_raises_for_scene():
    from nicr_mt_scene_analysis_amd.model.postprocessing import get_postprocessing_class
    with pytest.raises(NotImplementedError):
        get_postprocessing_class('scene')


def test_confusion_matrix_state():
    from nicr_mt_scene_analysis_amd._lib import NmsaError
    from nicr_mt_scene_analysis_amd.metric import ConfusionMatrix
    m = ConfusionMatrix(num_classes=7, device='cpu')
    assert m.state_names() == ['confmat'] and m._state_reduce == {'confmat': 'sum'}
    assert m.confmat.dtype == torch.int64 and tuple(m.confmat.shape) == (7, 7)
    m.confmat += 2
    assert int(m.compute().sum()) == 98
    m.reset()
    assert int(m.confmat.sum()) == 0
    with pytest.raises(NmsaError):                               # the states live on the GPU: no CPU fallback
        m.update(torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64))


def test_training_postprocessing_passes_through_on_cpu_tensors():
    from nicr_mt_scene_analysis_amd.model.postprocessing import ScenePostprocessing
    keys = jload(load('scene_task')['keys'])
    out = torch.randn(2, 5)
    r = ScenePostprocessing(unknown_kwarg=1).postprocess((out, None), {}, is_training=True)
    assert type(r) is dict and list(r) == keys['post_training'] and r['scene_output'] is out


def test_helper_keys_match_the_fixture():
    from nicr_mt_scene_analysis_amd.task_helper import SceneTaskHelper
    keys = jload(load('scene_task')['keys'])
    h = SceneTaskHelper(5, class_weights=np.arange(1, 6, dtype=np.float64), label_smoothing=0.1)
    h.initialize(torch.device('cpu'))
    assert keys['losses'] == [h.mark_as_total('scene')] == ['scene_total_loss']
    assert h._class_weights.dtype == torch.float32 and h._metric_cm.confmat.dtype == torch.int64
    h._metric_cm.confmat += torch.tensor([[2, 1, 0, 0, 0], [0, 3, 0, 0, 0], [0, 0, 0, 0, 0], [1, 0, 0, 0, 0],
                                          [0, 0, 0, 0, 4]])
    artifacts, examples, logs = h.validation_epoch_end()
    assert list(artifacts) == keys['artifacts'] and list(examples) == keys['examples']
    assert sorted(logs) == keys['epoch_end_logs']
    # empty classes are ignored: (2 + 3 + 0 + 4) / 11, mean(2/3, 1, 0, 1)
    assert float(logs['scene_acc']) == pytest.approx(9 / 11) and float(logs['scene_bacc']) == pytest.approx(2 / 3)
    assert int(artifacts['scene_cm'].sum()) == 11 and int(h._metric_cm.confmat.sum()) == 0


def test_the_steps_have_no_cpu_fallback():
    from nicr_mt_scene_analysis_amd._lib import NmsaError
    from nicr_mt_scene_analysis_amd.model.postprocessing import ScenePostprocessing
    from nicr_mt_scene_analysis_amd.task_helper import SceneTaskHelper
    h = SceneTaskHelper(5)
    h.initialize(torch.device('cpu'))
    batch, post = {'scene': torch.tensor([1, 0, 3])}, {'scene_output': torch.randn(3, 5)}
    for step in (h.training_step, h.validation_step):
        with pytest.raises(NmsaError):
            step(batch, 0, post)
    with pytest.raises(NmsaError):
        ScenePostprocessing().postprocess((post['scene_output'], None), batch, is_training=False)


def test_wrapper_argument_checks_come_before_the_device():
    from nicr_mt_scene_analysis_amd import ops
    with pytest.raises(TypeError):
        ops.scene_step(torch.zeros(2, 3, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.scene_step(torch.zeros(2, 3), want=('probabilities',))


def test_fixture_index_is_the_first_largest_logit():
    """what the kernel computes, stated on the fixture: wherever the reference's top-two
    probabilities differ or the top-two logits are equal, its index is numpy's first argmax"""
    from nicr_mt_scene_analysis_amd.testing import synthetic as syn
    g = load('scene_task')
    for name in jload(g['names']):
        inputs = syn.make_scene_inputs(name)
        assert syn.scene_input_digest(inputs) == jload(g[f'{name}__params'])['digest'], name
        logits = [x for epoch in inputs['batches'] for x, _ in epoch]
        first = np.concatenate([np.argmax(x, axis=1) for x in logits])
        assert len(first) == 2 * 25 and np.array_equal(first, g[f'{name}__idx']), name
