"""Batch augmentation behind a resize: the one-launch path (`ops.batch_augment_resized`,
nmsa_batch_augment_resized) next to its floor and to what torch offers, on the MI355X.

Five keys of a raw training batch (rgb u8 [B,H,W,3], depth u16, semantic u8, instance i32 [B,H,W],
normal f32 [B,H,W,3]), B = 32, crop 480 x 640, half of the samples flipped, two configurations:

  up_1.0_1.4     480 x 640 sources, scales U(1.0, 1.4): every training recipe's RandomResize
  any_0.5_2.0    960 x 1280 sources, scales U(0.5, 2.0): down- and upscaling in one batch (on
                 480 x 640 sources a scale below 1 leaves an image smaller than the crop, which is
                 the double resize `BatchAugmentation` refuses)

and these paths, which write the same number of output bytes from the same sources:

  resized   host tables + one asynchronous copy + ONE kernel for all keys and samples
  floor     `ops.batch_augment` (nmsa_batch_augment): crop, flip, normalise without a resize.  It
            reads one source pixel per output pixel, contiguously: what the output stream costs.
  resized_replay, floor_replay   the two launches replayed from a captured graph: the staging copy
            and the kernel without any host work
  torch     what a user can do on the device without this path: per sample `F.interpolate` of the
            whole image (bilinear for rgb, nearest for the rest, through float32), then slice,
            flip, normalise, permute, one stack per key.  Its rgb is float bilinear, NOT OpenCV's
            8-bit fixed point: it is timed, not compared.

Per path the time of each of `--calls` eager calls between two HIP events after `--warmup` calls;
the paths alternate call by call.  Reported: median, 10th and 90th percentile per call, the host
time of `ops.augment_window_tables` alone (median of the same number of calls), the output bytes and
`out_TB_per_s` = output bytes over the median time.  One JSON line per configuration.

Usage: python tools/bench_augment_resize.py [--calls 200] [--warmup 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nicr_mt_scene_analysis_amd import ops                                      # noqa: E402
from nicr_mt_scene_analysis_amd.data.preprocessing.augmentation import RGB_MEAN, RGB_STD      # noqa: E402

B, CROP_H, CROP_W = 32, 480, 640
CONFIGS = {'up_1.0_1.4': ((480, 640), (1.0, 1.4)), 'any_0.5_2.0': ((960, 1280), (0.5, 2.0))}
DEPTH_MEAN, DEPTH_STD = 2841.94941272766, 1417.2594281672277


def make_batch(H, W, dev):
    g = torch.Generator(device=dev).manual_seed(11)
    return {
        'rgb': torch.randint(0, 256, (B, H, W, 3), device=dev, generator=g).to(torch.uint8),
        'depth': torch.randint(0, 65536, (B, H, W), device=dev, generator=g).to(torch.uint16),
        'semantic': torch.randint(0, 41, (B, H, W), device=dev, generator=g).to(torch.uint8),
        'instance': torch.randint(0, 65536, (B, H, W), device=dev, generator=g).to(torch.int32),
        'normal': torch.randn((B, H, W, 3), device=dev, generator=g),
    }


def draw_table(H, W, scales, rng):
    """(y0, x0, flip, rh, rw) per sample, as RandomResize -> RandomCrop -> RandomHorizontalFlip draw them"""
    table = np.zeros((B, 5), np.int64)
    for b in range(B):
        s = rng.uniform(*scales)
        rh, rw = int(round(s * H)), int(round(s * W))
        table[b] = (rng.randint(0, rh - CROP_H) if rh > CROP_H else 0, rng.randint(0, rw - CROP_W) if rw > CROP_W else 0,
                    b % 2, rh, rw)
    return table


def percentiles(t):
    t = sorted(t)
    return {'median': round(statistics.median(t), 2), 'p10': round(t[len(t) // 10], 2), 'p90': round(t[-1 - len(t) // 10], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    dev = torch.device('cuda:0')
    mean, std = (torch.from_numpy(a).to(dev)[:, None, None] for a in (RGB_MEAN, RGB_STD))
    dmean, dstd = (torch.tensor(v, dtype=torch.float32, device=dev) for v in (DEPTH_MEAN, DEPTH_STD))
    norm = {'rgb': ('rgb_norm', RGB_MEAN, RGB_STD), 'depth': ('depth_norm', DEPTH_MEAN, DEPTH_STD, False, 0.0)}
    for name, ((H, W), scales) in CONFIGS.items():
        batch = make_batch(H, W, dev)
        table = draw_table(H, W, scales, np.random.RandomState(3))
        # the floor crops the same number of pixels out of the sources themselves
        plain = np.stack([table[:, 0] * (H - CROP_H) // np.maximum(table[:, 3] - CROP_H, 1),
                          table[:, 1] * (W - CROP_W) // np.maximum(table[:, 4] - CROP_W, 1), table[:, 2]], axis=1)
        # torch has few kernels for uint16: its path moves the depth bits as int16
        as_torch = dict(batch, depth=batch['depth'].view(torch.int16))

        def resized():
            return ops.batch_augment_resized(batch, table, (CROP_H, CROP_W), norm)

        def floor():
            return ops.batch_augment(batch, plain, (CROP_H, CROP_W), norm)

        def with_torch():
            out = {k: [] for k in as_torch}
            for b, (y0, x0, flip, rh, rw) in enumerate(table.tolist()):
                for k, v in as_torch.items():
                    t = v[b].view(torch.uint16).float() if k == 'depth' else v[b].float()
                    t = t.movedim(-1, 0) if t.ndim == 3 else t[None]
                    t = F.interpolate(t[None], size=(rh, rw), **(dict(mode='bilinear', align_corners=False)
                                                                 if k == 'rgb' else dict(mode='nearest')))[0]
                    t = t[:, y0:y0 + CROP_H, x0:x0 + CROP_W]
                    t = t.flip(2) if flip else t
                    if k == 'rgb':
                        t = (t - mean) / std
                    elif k == 'depth':
                        t = (t - dmean) / dstd
                    elif k != 'normal':
                        t = t[0].to(batch[k].dtype)
                    out[k].append(t)
            return {k: torch.stack(v) for k, v in out.items()}

        paths = {'resized': resized, 'floor': floor, 'torch': with_torch}
        results = {p: fn() for p, fn in paths.items()}
        torch.cuda.synchronize()
        # the device's share alone: the staging copy and the kernel replayed from a captured graph
        graphs = {}
        for p in ('resized', 'floor'):
            graphs[p] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[p]):
                kept = paths[p]()
            paths[p]()                              # a staging of its own again for the eager calls
            paths[p + '_replay'] = graphs[p].replay
        torch.cuda.synchronize()
        for k in batch:
            for p in ('floor', 'torch'):
                assert results[p][k].shape == results['resized'][k].shape and \
                    results[p][k].dtype == results['resized'][k].dtype, (p, k)
        out_bytes = sum(t.numel() * t.element_size() for t in results['resized'].values())
        del results
        for _ in range(args.warmup):
            for fn in paths.values():
                fn()
        torch.cuda.synchronize()
        times, host = {p: [] for p in paths}, []
        for _ in range(args.calls):
            for p, fn in paths.items():
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                fn()
                stop.record()
                stop.synchronize()
                times[p].append(start.elapsed_time(stop) * 1e3)
            t0 = time.perf_counter()
            ops.augment_window_tables(table, (H, W), (CROP_H, CROP_W))
            host.append((time.perf_counter() - t0) * 1e6)
        print(json.dumps({
            'config': name, 'B': B, 'source': [H, W], 'crop': [CROP_H, CROP_W], 'scales': list(scales),
            'resized_sizes': [int(table[:, 3].min()), int(table[:, 3].max())], 'keys': list(batch),
            'calls': args.calls, 'warmup': args.warmup, 'out_bytes': out_bytes,
            'table_words': 3 * B * (CROP_H + CROP_W),
            'us_per_call': {p: percentiles(t) for p, t in times.items()},
            'host_tables_us': percentiles(host),
            'resized_over_floor': round(statistics.median(times['resized']) / statistics.median(times['floor']), 3),
            'replay_over_replay': round(statistics.median(times['resized_replay']) /
                                        statistics.median(times['floor_replay']), 3),
            'out_TB_per_s': {p: round(out_bytes / statistics.median(t) * 1e-6, 3) for p, t in times.items()}}),
            flush=True)


if __name__ == '__main__':
    main()
