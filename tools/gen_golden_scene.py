"""Writes tests/golden/scene_task.npz: the reference's unmodified `model/postprocessing/scene.py`
and `task_helper/scene.py`, loaded through `oracle.ref_loader`, run on CPU on seeded batches.

`load_reference(task_helpers=True)` does not load these two files; they are loaded here with the
loader's own `_load`.  `task_helper/scene.py` imports `ConfusionMatrix` from torchmetrics, which
is not installed: the `ConfusionMatrix` below is added to the loader's stub `torchmetrics` module
first.  It is a stand-in written for this tool, NOT reference code — the state the helper touches
(`_defaults['confmat']`, `confmat`), `update(preds, target)` as one `bincount`, `reset()`.

The fixture holds recorded results only, a few KB.  The inputs are NOT stored: they are the seeded
cases of `testing.synthetic.SCENE_CASES` (`make_scene_inputs`), and a SHA-256 of their bytes is; the
tests regenerate them and fail on a mismatch.  Per case (`names`), with the batches of both epochs
in the order they ran (rows concatenated):
  <case>__params      JSON {n_classes, label_smoothing, weighted, epochs, batch_rows, digest}
  <case>__score, __idx              the reference's scene_class_score / scene_class_idx, all rows
  <case>__val_loss, __train_loss    scene_total_loss of validation_step / training_step, [epochs, batches]
  <case>__cm, __acc, __bacc         validation_epoch_end, [epochs, ...]
  keys                JSON: key lists of both postprocessing dicts, the loss dict, the logs of the
                      three steps, the artifacts and the examples
Batches: plain rows, rows with void labels, an all-void batch, and rows whose two largest logits
are exactly equal.  The generator asserts that no recorded row has DISTINCT top-two logits with
EQUAL float32 probabilities: there the reference's index would depend on the rounding of ATen's
softmax, which the kernel (argmax of the logits) does not mirror.

Usage: python tools/gen_golden_scene.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nicr_mt_scene_analysis_amd.testing import synthetic as syn      # noqa: E402
from oracle import ref_loader                                        # noqa: E402


def jdump(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


def load_scene_modules():
    ref = ref_loader.load_reference(task_helpers=True)
    tm = sys.modules['torchmetrics']

    class ConfusionMatrix(tm.Metric):
        """stand-in for torchmetrics.ConfusionMatrix (not reference code): row = target"""

        def __init__(self, num_classes):
            super().__init__()
            self.num_classes = num_classes
            self.add_state('confmat', torch.zeros(num_classes, num_classes), dist_reduce_fx='sum')

        def update(self, preds, target):
            n = self.num_classes
            flat = torch.bincount(target.long() * n + preds.long(), minlength=n * n)
            self.confmat = self.confmat + flat.reshape(n, n).to(self.confmat.dtype)

    tm.ConfusionMatrix = ConfusionMatrix
    post = ref_loader._load('model.postprocessing.scene', 'model/postprocessing/scene.py')
    helper = ref_loader._load('task_helper.scene', 'task_helper/scene.py')
    return ref, post, helper


def assert_index_rule_is_decided(logits):
    """no row with distinct top-two logits and equal float32 probabilities"""
    p = torch.softmax(torch.from_numpy(logits), dim=1).numpy()
    order = np.argsort(-logits, axis=1, kind='stable')
    rows = np.arange(len(logits))
    a, b = order[:, 0], order[:, min(1, logits.shape[1] - 1)]
    undecided = (logits[rows, a] != logits[rows, b]) & (p[rows, a] == p[rows, b])
    assert not undecided.any(), f'rows {np.nonzero(undecided)[0]}: index depends on softmax rounding'


def main():
    ref, post_mod, helper_mod = load_scene_modules()
    out = {'names': jdump(list(syn.SCENE_CASES))}
    keys = {}
    for name, (C, weighted, smoothing, seed) in syn.SCENE_CASES.items():
        inputs = syn.make_scene_inputs(name)
        weights = inputs['weights']
        out[f'{name}__params'] = jdump({'n_classes': C, 'label_smoothing': smoothing, 'weighted': weighted,
                                        'epochs': syn.SCENE_EPOCHS, 'batch_rows': [B for B, _ in syn.SCENE_BATCHES],
                                        'digest': syn.scene_input_digest(inputs)})
        helper = helper_mod.SceneTaskHelper(C, class_weights=weights, label_smoothing=smoothing)
        helper.initialize(torch.device('cpu'))
        post = post_mod.ScenePostprocessing()
        rec = {k: [] for k in ('score', 'idx', 'val_loss', 'train_loss', 'cm', 'acc', 'bacc')}
        for e, epoch in enumerate(inputs['batches']):
            for j, (logits, labels) in enumerate(epoch):
                assert_index_rule_is_decided(logits)
                batch = {'scene': torch.from_numpy(labels)}
                x = torch.from_numpy(logits)
                r_train = post.postprocess((x, None), batch, is_training=True)
                losses, logs = helper.training_step(batch, j, r_train)
                keys['post_training'], keys['losses'], keys['training_logs'] = \
                    list(r_train), list(losses), sorted(logs)
                rec['train_loss'].append(losses['scene_total_loss'].item())
                with torch.no_grad():
                    r = post.postprocess((x, None), batch, is_training=False)
                    losses, logs = helper.validation_step(batch, j, r)
                keys['post_inference'], keys['validation_logs'] = list(r), sorted(logs)
                rec['score'].append(r['scene_class_score'].numpy())
                rec['idx'].append(r['scene_class_idx'].numpy())
                rec['val_loss'].append(losses['scene_total_loss'].item())
            artifacts, examples, logs = helper.validation_epoch_end()
            keys['artifacts'], keys['examples'], keys['epoch_end_logs'] = \
                list(artifacts), list(examples), sorted(logs)
            cm = artifacts['scene_cm'].numpy()
            assert cm.dtype == np.int64 and cm.sum() > 0
            rec['cm'].append(cm)
            rec['acc'].append(logs['scene_acc'].item())
            rec['bacc'].append(logs['scene_bacc'].item())
            print(name, e, int(cm.sum()), float(logs['scene_acc']), float(logs['scene_bacc']))
        n = len(syn.SCENE_BATCHES)
        out[f'{name}__score'] = np.concatenate(rec['score']).astype(np.float32)
        out[f'{name}__idx'] = np.concatenate(rec['idx']).astype(np.int64)
        out[f'{name}__val_loss'] = np.asarray(rec['val_loss'], np.float32).reshape(-1, n)
        out[f'{name}__train_loss'] = np.asarray(rec['train_loss'], np.float32).reshape(-1, n)
        out[f'{name}__cm'] = np.stack(rec['cm'])
        out[f'{name}__acc'] = np.asarray(rec['acc'], np.float32)
        out[f'{name}__bacc'] = np.asarray(rec['bacc'], np.float32)
    out['keys'] = jdump(keys)
    path = os.path.join(ROOT, 'tests', 'golden', 'scene_task.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
