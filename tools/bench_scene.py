#!/usr/bin/env python3
"""The scene task's steps against the reference's formulation written as torch ops on the
device.  Same process, same tensors, HIP events.  Per pair of paths: 10 warm-up calls each, then 24
windows of 10 calls per path, the two paths ALTERNATING window by window (240 timed calls per
path); reported are the median of the window means and their minimum / maximum, in microseconds.
B = 32 / 64, C = 10 / 45, class weights and label smoothing 0.1, a quarter of the rows void.
  post        ScenePostprocessing (inference): one launch, score + idx
              vs  F.softmax + torch.max
  validation  SceneTaskHelper.validation_step: one launch (loss + confusion-matrix update), nothing
              awaited
              vs  the reference's step (task_helper/scene.py:90-110): CrossEntropyLoss on
              `scene.long() - 1`, `sum(mask) > 0` in Python, the two `.cpu()` copies and a
              bincount update of a host matrix (what torchmetrics' ConfusionMatrix.update does)
  training    SceneTaskHelper.training_step + backward: one launch (loss + gradient) and the
              scaling in backward
              vs  CrossEntropyLoss + backward
The windows end in an event synchronise; the reference's validation step also waits inside.
  python tools/bench_scene.py [--windows 24] [--calls 10]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nicr_mt_scene_analysis_amd.model.postprocessing import ScenePostprocessing   # noqa: E402
from nicr_mt_scene_analysis_amd.task_helper import SceneTaskHelper                # noqa: E402

SHAPES = ((32, 10), (32, 45), (64, 10), (64, 45))
SMOOTHING = 0.1


def window(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls * 1e3


def timed_alternating(paths, windows, calls):
    """{name: fn} -> {name: (median, min, max) of the window means in us}"""
    for fn in paths.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in paths}
    for _ in range(windows):
        for name, fn in paths.items():
            samples[name].append(window(fn, calls))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=24)
    ap.add_argument('--calls', type=int, default=10)
    args = ap.parse_args()
    assert args.windows * args.calls >= 200, 'at least 200 timed calls per path'
    dev = torch.device('cuda')
    g = torch.Generator(device=dev).manual_seed(0)
    for B, C in SHAPES:
        x = torch.randn((B, C), device=dev, generator=g) * 3.0
        scene = torch.randint(1, C + 1, (B,), device=dev, generator=g)
        scene[torch.rand((B,), device=dev, generator=g) < 0.25] = 0
        scene = scene.to(torch.uint8)
        weights = torch.rand((C,), device=dev, generator=g) + 0.25
        batch = {'scene': scene}
        helper = SceneTaskHelper(C, class_weights=weights.cpu().numpy(), label_smoothing=SMOOTHING)
        helper.initialize(dev)
        post = ScenePostprocessing()
        ref_loss = torch.nn.CrossEntropyLoss(weight=weights, label_smoothing=SMOOTHING, ignore_index=-1)
        ref_cm = torch.zeros((C, C), dtype=torch.int64)
        leaf = x.clone().requires_grad_(True)

        def post_hip():
            return post.postprocess((x, None), batch, is_training=False)

        def post_torch():
            score, idx = torch.max(F.softmax(x, dim=1), dim=1)
            return {'scene_class_score': score, 'scene_class_idx': idx, 'scene_output': x}

        predictions = post_torch()

        def validation_hip():
            helper.validation_step(batch, 0, predictions)

        def validation_torch():
            loss = ref_loss(predictions['scene_output'], batch['scene'].long() - 1)
            mask = batch['scene'] != 0
            if sum(mask) > 0:
                preds = predictions['scene_class_idx'][mask].cpu()
                target = (batch['scene'][mask] - 1).cpu().long()
                ref_cm.add_(torch.bincount(target * C + preds, minlength=C * C).reshape(C, C))
            return loss

        def training_hip():
            leaf.grad = None
            losses, _ = helper.training_step(batch, 0, {'scene_output': leaf})
            losses['scene_total_loss'].backward()

        def training_torch():
            leaf.grad = None
            ref_loss(leaf, batch['scene'].long() - 1).backward()

        row = {'B': B, 'C': C, 'calls_per_path': args.windows * args.calls}
        for leg, paths in (('post', {'hip': post_hip, 'torch': post_torch}),
                           ('validation', {'hip': validation_hip, 'torch': validation_torch}),
                           ('training', {'hip': training_hip, 'torch': training_torch})):
            t = timed_alternating(paths, args.windows, args.calls)
            for name, (med, lo, hi) in t.items():
                row[f'{leg}_{name}_us'] = {'median': round(med, 2), 'min': round(lo, 2), 'max': round(hi, 2)}
            row[f'{leg}_speedup'] = round(t['torch'][0] / t['hip'][0], 2)
        # both validation paths saw the same calls: the matrices must agree
        row['confmat_equal'] = bool(torch.equal(helper._metric_cm.confmat.cpu(), ref_cm))
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
