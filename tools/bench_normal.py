#!/usr/bin/env python3
"""The surface-normal task's two kernels against the torch ops they replace.  Same process, same
tensors, HIP events.  Per pair of paths: 10 warm-up calls each, then 24 windows of 10 calls per
path, the two paths ALTERNATING window by window (240 timed launches per path); reported are the
median of the window means and their minimum / maximum.  B = 16, 3 channels:
  480x640 -> 480x640 (no resize) and 768x1024 -> 960x1280 (nearest resize, 1.25x).
  rmse   RootMeanSquaredError.update_from_network_resolution (crop + nearest resize + mask + RMSE in
         one pass; at equal resolutions the plain one-pass update)
         vs  `composed`: ops.resize_nearest (only where the resolutions differ) + the valid mask as
         six torch ops + the RMSE as five torch ops + the two state updates
         vs  `composed_nomask`: the same without the mask ops (resize + five ops, every pixel)
  mask   ops.normal_valid_mask  vs  the six torch ops
Model traffic of the fused RMSE: 12 B per target pixel + 12 B per prediction pixel read.
  python tools/bench_normal.py [--windows 24] [--calls 10]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nicr_mt_scene_analysis_amd import ops                                    # noqa: E402
from nicr_mt_scene_analysis_amd.metric import RootMeanSquaredError            # noqa: E402

B = 16
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
    """{name: fn} -> {name: (median, min, max) of the window means in ms}"""
    for fn in paths.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in paths}
    for _ in range(windows):
        for name, fn in paths.items():
            samples[name].append(window(fn, calls))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in samples.items()}


def has_normal(t):
    """bool [B,H,W]: some channel of the [B,3,H,W] map differs from zero — six torch ops"""
    zero = t == 0
    return ~(zero[:, 0] & zero[:, 1] & zero[:, 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=24)
    ap.add_argument('--calls', type=int, default=10)
    args = ap.parse_args()
    assert args.windows * args.calls >= 200, 'at least 200 timed launches per path'
    dev = torch.device('cuda')
    g = torch.Generator(device=dev).manual_seed(0)
    for (H, W), (FH, FW) in SHAPES:
        pred = torch.randn((B, 3, H, W), device=dev, generator=g)
        target = torch.nn.functional.normalize(torch.randn((B, 3, FH, FW), device=dev, generator=g), dim=1)
        target *= (torch.rand((B, 1, FH, FW), device=dev, generator=g) > 0.3)
        crop = (slice(0, H), slice(0, W))
        resized = (H, W) != (FH, FW)
        metric = RootMeanSquaredError(device=dev)
        acc = {k: [torch.zeros((), dtype=torch.float64, device=dev),
                   torch.zeros((), dtype=torch.int64, device=dev)] for k in ('masked', 'all')}

        def fused():
            metric.update_from_network_resolution(pred, crop, target, mask='target')

        def error_map():
            up = ops.resize_nearest(pred, (FH, FW), crop) if resized else pred
            return (up - target).pow(2).mean(dim=1).sqrt()

        def composed():
            err, keep = error_map(), has_normal(target)
            acc['masked'][0] += err[keep].sum()
            acc['masked'][1] += keep.sum()

        def composed_nomask():
            err = error_map()
            acc['all'][0] += err.sum()
            acc['all'][1] += err.numel()

        row = {'shape': f'{B}x3x{H}x{W}->{FH}x{FW}', 'composition_resizes': resized,
               'launches_per_path': args.windows * args.calls}
        t = timed_alternating({'fused': fused, 'composed': composed, 'composed_nomask': composed_nomask},
                              args.windows, args.calls)
        for name, (med, lo, hi) in t.items():
            row[f'rmse_{name}_ms'] = {'median': med, 'min': lo, 'max': hi}
        row['rmse_speedup'] = t['composed'][0] / t['fused'][0]
        row['rmse_speedup_nomask'] = t['composed_nomask'][0] / t['fused'][0]
        row['rmse_fused_model_GBps'] = B * 12 * (FH * FW + H * W) / t['fused'][0] / 1e6
        t = timed_alternating({'hip': lambda: ops.normal_valid_mask(target),
                               'torch': lambda: has_normal(target)}, args.windows, args.calls)
        for name, (med, lo, hi) in t.items():
            row[f'mask_{name}_ms'] = {'median': med, 'min': lo, 'max': hi}
        row['mask_speedup'] = t['torch'][0] / t['hip'][0]
        row['mask_hip_model_GBps'] = B * 13 * FH * FW / t['hip'][0] / 1e6
        # the fused and the masked composition saw the same calls: the metrics must agree
        row['rmse_fused'] = float(metric.compute())
        row['rmse_composed'] = float(acc['masked'][0] / acc['masked'][1])
        print(json.dumps(row), flush=True)
        del pred, target
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
