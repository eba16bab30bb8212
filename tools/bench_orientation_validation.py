#!/usr/bin/env python3
"""Validation steps of InstanceTaskHelper + PanopticTaskHelper with orientations in the batch: the
orientation metrics on device tables (`use_orientation_tables`, the default) against the same
build's dict path (host loops over Python dicts), in one process.  Protocol of tools/bench_normal.py:
HIP events, 10 warm-up calls per path, then windows of `--calls` calls per path, the two paths
ALTERNATING window by window; reported are the median of the window means and their minimum /
maximum.  B = 32, 40 classes, ~30 instances per image:
  480x640 (network = dataset resolution) and 768x1024 -> 960x1280.
  step        postprocess + both helpers' validation_step (a fresh postprocessing result per call:
              its lazy entries are built inside the timed region by whoever reads them)
  helpers     both validation_steps alone on a result whose entries both paths have read before
  wide sums   ops.instance_orientation_sums_wide on the ground-truth instance map with an id table
              of 1024 (the first try of the former retry loop) against 4096 (the one run of
              `_get_instance_orientation_table`)
  python tools/bench_orientation_validation.py [--windows 24] [--calls 10]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nicr_mt_scene_analysis_amd import ops                                                  # noqa: E402
from nicr_mt_scene_analysis_amd.data import preprocessing as pre                            # noqa: E402
from nicr_mt_scene_analysis_amd.data.preprocessing import APPLIED_PREPROCESSING_KEY         # noqa: E402
from nicr_mt_scene_analysis_amd.model.postprocessing import get_postprocessing_class        # noqa: E402
from nicr_mt_scene_analysis_amd.task_helper import InstanceTaskHelper, PanopticTaskHelper   # noqa: E402
from nicr_mt_scene_analysis_amd.testing import synthetic as syn                             # noqa: E402

B, N_CLASSES = 32, 41                   # with void
SHAPES = (((480, 640), (480, 640)), ((768, 1024), (960, 1280)))


def window(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def timed_alternating(paths, windows, calls):
    for fn in paths.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in paths}
    for _ in range(windows):
        for name, fn in paths.items():
            samples[name].append(window(fn, calls))
    return {name: {'median': statistics.median(v), 'min': min(v), 'max': max(v)} for name, v in samples.items()}


def nearest(t, shape):
    """label map [B,H,W] at another resolution (index arithmetic: ids survive)"""
    H, W = t.shape[-2:]
    ys = (torch.arange(shape[0], device=t.device) * H) // shape[0]
    xs = (torch.arange(shape[1], device=t.device) * W) // shape[1]
    return t[:, ys][:, :, xs].contiguous()


def targets(sem, ins, is_thing, rng, dev):
    batch = {'semantic': sem.clone(), 'instance': ins.clone()}
    pre.InstanceClearStuffIDs(semantic_classes_is_thing=is_thing)(batch)
    ids = [np.unique(i) for i in batch['instance'].cpu().numpy()]
    batch['orientations'] = [{int(k): float(rng.uniform(0, 2 * np.pi)) for k in i if k} for i in ids]
    pre.InstanceTargetGenerator(sigma=8, semantic_classes_is_thing=is_thing)(batch)
    pre.OrientationTargetGenerator(semantic_classes_estimate_orientation=is_thing)(batch)
    pre.PanopticTargetGenerator(semantic_classes_is_thing=is_thing)(batch)
    return batch


def make_case(H, W, FH, FW, dev, seed=0):
    rng = np.random.default_rng(seed)
    lab = syn.make_label_maps(B, N_CLASSES, H, W, n_instances=30, seed=seed)
    is_thing = tuple(bool(x) for x in lab['semantic_classes_is_thing'])
    sem, ins = torch.from_numpy(lab['semantic']).to(dev), torch.from_numpy(lab['instance']).to(dev)
    batch = targets(sem, ins, is_thing, rng, dev)
    full = batch if (H, W) == (FH, FW) else targets(nearest(sem, (FH, FW)), nearest(ins, (FH, FW)),
                                                    is_thing, rng, dev)
    for k in ('semantic', 'instance', 'panoptic'):
        batch[f'{k}_fullres'] = full[k]
    batch['panoptic_ids_to_instance_dict'] = full['panoptic_ids_to_instance_dict']
    batch['rgb_fullres'] = torch.zeros((B, 3, FH, FW))
    batch[APPLIED_PREPROCESSING_KEY] = [[{'type': 'Resize', 'valid_region_slice_y': slice(0, H),
                                          'valid_region_slice_x': slice(0, W)}]] * B
    # network-like outputs that mostly agree with the ground truth (testing.synthetic's recipe)
    g = torch.Generator(device=dev).manual_seed(seed)
    C = N_CLASSES - 1
    logits = torch.randn((B, C, H, W), device=dev, generator=g)
    logits += 3.0 * (torch.arange(C, device=dev).view(1, C, 1, 1) == (batch['semantic'].long() - 1).unsqueeze(1))
    center = (batch['instance_center'].reshape(B, 1, H, W)
              + 0.03 * torch.randn((B, 1, H, W), device=dev, generator=g)).clamp(0, 1)
    offset = batch['instance_offset'] + 0.004 * torch.randn((B, 2, H, W), device=dev, generator=g)
    ori = batch['orientation'] + 0.25 * torch.randn((B, 2, H, W), device=dev, generator=g)
    ori = ori / (ori.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-7)
    data = ((logits, (center, offset, ori)), ((None, None), (None, None)))
    return batch, data, is_thing


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=24)
    ap.add_argument('--calls', type=int, default=10)
    args = ap.parse_args()
    dev = torch.device('cuda')
    for (H, W), (FH, FW) in SHAPES:
        batch, data, is_thing = make_case(H, W, FH, FW, dev)
        post = get_postprocessing_class('panoptic')(
            semantic_postprocessing=get_postprocessing_class('semantic')(),
            instance_postprocessing=get_postprocessing_class('instance')(),
            semantic_classes_is_thing=is_thing[1:], semantic_class_has_orientation=is_thing[1:])
        helpers = {}
        for name, use_tables in (('tables', True), ('dicts', False)):
            pair = (InstanceTaskHelper(N_CLASSES, is_thing), PanopticTaskHelper(N_CLASSES, is_thing, None))
            for h in pair:
                h.use_orientation_tables = use_tables
                h.initialize(dev)
            helpers[name] = pair

        def step(name):
            r = post.postprocess(data, batch, is_training=False)
            for h in helpers[name]:
                h.validation_step(batch, 0, r)

        shared = post.postprocess(data, batch, is_training=False)
        for name in helpers:                               # every lazy entry either path reads
            for h in helpers[name]:
                h.validation_step(batch, 0, shared)

        def helpers_only(name):
            for h in helpers[name]:
                h.validation_step(batch, 0, shared)

        row = {'shape': f'{B}x{H}x{W}->{FH}x{FW}', 'launches_per_path': args.windows * args.calls,
               'orientations_per_image': float(np.mean([len(d) for d in batch['orientations_present']]))}
        row['step_ms'] = timed_alternating({n: (lambda n=n: step(n)) for n in helpers}, args.windows, args.calls)
        row['helpers_ms'] = timed_alternating({n: (lambda n=n: helpers_only(n)) for n in helpers},
                                              args.windows, args.calls)
        row['step_speedup'] = row['step_ms']['dicts']['median'] / row['step_ms']['tables']['median']
        row['helpers_speedup'] = row['helpers_ms']['dicts']['median'] / row['helpers_ms']['tables']['median']
        ori, ins, fg = data[0][1][2], batch['instance'], batch['orientation_foreground']
        row['wide_sums_ms'] = timed_alternating(
            {str(n): (lambda n=n: ops.instance_orientation_sums_wide(ori, ins, fg, n)) for n in (1024, 4096)},
            args.windows, args.calls)
        # both paths saw the same calls: the epoch logs must agree
        logs = {n: {**helpers[n][0].validation_epoch_end()[2], **helpers[n][1].validation_epoch_end()[2]}
                for n in helpers}
        row['mae'] = {n: {k: float(v) for k, v in logs[n].items() if 'mae' in k and k.endswith('rad')}
                      for n in helpers}
        print(json.dumps(row), flush=True)
        del batch, data, shared
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
