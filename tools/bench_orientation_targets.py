#!/usr/bin/env python3
"""`ops.orientation_targets` against `ops.instance_targets` (the yardstick: the same scan and a
heavier paint) and against a torch composition of the reference's loop on the device.  Same
process, same tensors, HIP events.  10 warm-up calls per path, then 24 windows of 10 calls per
path, the paths ALTERNATING window by window (240 timed launches per path); reported are the
median of the window means and their minimum / maximum.  B = 32, 480x640, 41 classes, 60 instances
per image, angles for two thirds of them.
  orientation_list / orientation_none   with / without the class list (probe of the scan's id table)
  orientation_list_search               NMSA_OT_LOOKUP=search: binary search over the keys in LDS
  instance                              ops.instance_targets, sigma 8, normalised offsets
  composition                           per image and id: a mask, `bincount(semantic[mask]).argmax()`,
                                        a masked assignment of each channel and of the foreground
                                        (2 warm-up calls, 5 windows of 1 call: it takes ~0.2 s)
Model traffic of the orientation paint: 4 B/px read + 9 B/px written (the scan reads 5 B/px).
  python tools/bench_orientation_targets.py [--windows 24] [--calls 10]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nicr_mt_scene_analysis_amd import ops                                    # noqa: E402
from nicr_mt_scene_analysis_amd.testing import synthetic as syn               # noqa: E402

B, NC, H, W, N_INST, SIGMA = 32, 41, 480, 640, 60, 8


def window(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def timed_alternating(paths, windows, calls, warmup=10):
    """{name: fn} -> {name: (median, min, max) of the window means in ms}"""
    for fn in paths.values():
        for _ in range(warmup):
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
    assert args.windows * args.calls >= 200, 'at least 200 timed launches per path'
    dev = torch.device('cuda')
    maps = syn.make_label_maps(B, NC, H, W, n_instances=N_INST, seed=5)
    rng = np.random.default_rng(6)
    ids = [[int(i) for i in np.unique(maps['instance'][b]) if i > 0] for b in range(B)]
    with_angle = [[i for i in img if rng.random() < 0.67] for img in ids]
    K = 64
    keys = np.zeros((B, K), np.int32)
    bit = np.zeros((B, K, 2), np.float32)
    for b, img in enumerate(with_angle):
        keys[b, :len(img)] = img
        rad = rng.uniform(-np.pi, np.pi, len(img))
        bit[b, :len(img)] = np.stack([np.cos(rad), np.sin(rad)], axis=1).astype(np.float32)
    n_keys = np.array([len(img) for img in with_angle], np.int32)
    estimate = np.arange(NC) % 2 == 1
    is_thing = maps['semantic_classes_is_thing']
    stuff = np.zeros((NC,), np.uint8)
    stuff[np.where(~is_thing)[0][1:]] = 1
    sem, ins = torch.from_numpy(maps['semantic']).to(dev), torch.from_numpy(maps['instance']).to(dev)
    d_keys, d_n, d_bit = (torch.from_numpy(a).to(dev) for a in (keys, n_keys, bit))
    d_est = torch.from_numpy(estimate.astype(np.uint8)).to(dev)
    d_th, d_st = torch.from_numpy(is_thing.astype(np.uint8)).to(dev), torch.from_numpy(stuff).to(dev)
    last = {}

    def orientation(est, lookup):
        def fn():
            if lookup:
                os.environ['NMSA_OT_LOOKUP'] = lookup
            else:
                os.environ.pop('NMSA_OT_LOOKUP', None)
            last[(est is not None, lookup)] = ops.orientation_targets(sem, ins, NC, est, d_keys, d_n, d_bit)
        return fn

    def instance():
        ops.instance_targets(sem, ins, NC, d_th, d_st, SIGMA, True)

    def composition():
        ori = torch.zeros((B, 2, H, W), dtype=torch.float32, device=dev)
        fg = torch.zeros((B, H, W), dtype=torch.bool, device=dev)
        flagged = d_est.bool()
        for b in range(B):
            for k, iid in enumerate(with_angle[b]):
                mask = ins[b] == iid
                accept = flagged[torch.bincount(sem[b][mask].long()).argmax()]
                paint = mask & accept
                ori[b, 0][paint] = d_bit[b, k, 0]
                ori[b, 1][paint] = d_bit[b, k, 1]
                fg[b] |= paint
        last['composition'] = (ori, fg)

    t = timed_alternating({'orientation_list': orientation(d_est, None),
                           'orientation_none': orientation(None, None),
                           'orientation_list_search': orientation(d_est, 'search'),
                           'instance': instance}, args.windows, args.calls)
    os.environ.pop('NMSA_OT_LOOKUP', None)
    t.update(timed_alternating({'composition': composition}, 5, 1, warmup=2))
    row = {'shape': f'{B}x{H}x{W}', 'classes': NC, 'instances_per_image': N_INST,
           'keys_per_image': float(n_keys.mean()), 'launches_per_path': args.windows * args.calls}
    for name, (med, lo, hi) in t.items():
        row[f'{name}_us'] = {'median': 1e3 * med, 'min': 1e3 * lo, 'max': 1e3 * hi}
    row['orientation_model_GBps'] = B * H * W * (5 + 4 + 9) / t['orientation_list'][0] / 1e6
    torch.cuda.synchronize()
    ori, fg = last['composition']
    for key in ((True, None), (True, 'search')):
        r = last[key]
        assert int(r['status'].item()) == 0
        assert torch.equal(r['orientation'], ori) and torch.equal(r['foreground'], fg), key
    row['painted_fraction'] = float(fg.float().mean())
    print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
