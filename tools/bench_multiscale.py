"""Side-output targets: the one-launch gather (`ops.multiscale_nearest`, nmsa_multiscale_nearest)
against the torch indexing callers used before it, on the MI355X.

Per shape, five keys of a training batch (semantic u8, instance i32, normal f32 [B,3,H,W], a bool
mask, dense_visual_embedding_indices i32) at the downscales (8, 16, 32), three paths:

  hip      one asynchronous table copy + ONE kernel for all keys and scales
  slice    `v[..., ::d, ::d].contiguous()`: one kernel per key and scale (right only where d
           divides both sides, which holds for the shapes timed here)
  select   `v.index_select(-2, rows).index_select(-1, cols)` with the maps of `cv2_nearest_map`
           already on the device: two kernels per key and scale (right for every shape)

Wall time between two HIP events around `--iters` back-to-back calls, so host-side launch cost
counts where the path is host-bound; the paths alternate within every one of `--rounds` rounds and
the median and the range over the rounds are reported, per call.  Every path's outputs are compared
with each other once before timing.  One JSON line per shape.

Usage: python tools/bench_multiscale.py [--iters 200] [--rounds 9]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nicr_mt_scene_analysis_amd import ops      # noqa: E402

DOWNSCALES = (8, 16, 32)
SHAPES = {'B32_480x640': (32, 480, 640), 'configs2_B64_480x640': (64, 480, 640)}


def make_batch(B, H, W, dev):
    g = torch.Generator(device=dev).manual_seed(11)
    return {
        'semantic': torch.randint(0, 41, (B, H, W), device=dev, generator=g).to(torch.uint8),
        'instance': torch.randint(0, 65536, (B, H, W), device=dev, generator=g).to(torch.int32),
        'normal': torch.randn((B, 3, H, W), device=dev, generator=g),
        'valid': torch.rand((B, H, W), device=dev, generator=g) < 0.5,
        'dense_visual_embedding_indices': torch.randint(0, 300, (B, H, W), device=dev, generator=g).to(torch.int32),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    dev = torch.device('cuda:0')
    for name, (B, H, W) in SHAPES.items():
        batch = make_batch(B, H, W, dev)
        maps = {d: (torch.from_numpy(ops.cv2_nearest_map(H, int(H / d))).to(dev),
                    torch.from_numpy(ops.cv2_nearest_map(W, int(W / d))).to(dev)) for d in DOWNSCALES}

        def hip():
            return ops.multiscale_nearest(batch, DOWNSCALES, (H, W))

        def sliced():
            return {d: {k: v[..., ::d, ::d].contiguous() for k, v in batch.items()} for d in DOWNSCALES}

        def select():
            return {d: {k: v.index_select(-2, maps[d][0]).index_select(-1, maps[d][1])
                        for k, v in batch.items()} for d in DOWNSCALES}

        paths = {'hip': hip, 'slice': sliced, 'select': select}
        results = {p: fn() for p, fn in paths.items()}
        torch.cuda.synchronize()
        for d in DOWNSCALES:
            for k in batch:
                a = results['hip'][d][k].view(torch.uint8)
                assert torch.equal(a, results['select'][d][k].contiguous().view(torch.uint8)), (d, k)
                assert torch.equal(a, results['slice'][d][k].view(torch.uint8)), (d, k)
        for fn in paths.values():                   # warm-up of every path at this shape
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        times = {p: [] for p in paths}
        for _ in range(args.rounds):
            for p, fn in paths.items():
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(args.iters):
                    fn()
                stop.record()
                stop.synchronize()
                times[p].append(start.elapsed_time(stop) * 1e3 / args.iters)
        n = len(batch) * len(DOWNSCALES)
        out_bytes = sum(t.numel() * t.element_size() for r in results['hip'].values() for t in r.values())
        print(json.dumps({
            'shape': name, 'keys': len(batch), 'downscales': DOWNSCALES, 'iters': args.iters,
            'rounds': args.rounds, 'output_bytes': out_bytes,
            'launches_per_call': {'hip': '1 kernel + 1 table copy', 'slice': f'{n} kernels',
                                  'select': f'{2 * n} kernels'},
            'us_per_call': {p: {'median': round(statistics.median(t), 2), 'min': round(min(t), 2),
                                'max': round(max(t), 2)} for p, t in times.items()}}), flush=True)


if __name__ == '__main__':
    main()
