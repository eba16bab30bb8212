"""Batch augmentation: the one-launch path (`ops.batch_augment`, nmsa_batch_augment) against the
torch formulations of the same chain (crop -> flip -> normalise -> CHW), on the MI355X.

Per shape, five keys of a raw training batch (rgb u8 [B,H,W,3], depth u16, semantic u8, instance
i32 [B,H,W], normal f32 [B,H,W,3]), 480 x 640 crops out of 488 x 648 sources, half of the samples
flipped, three paths:

  hip          one asynchronous table copy + ONE kernel for all keys and samples
  per_sample   what a caller writes first: per key and sample a slice, a flip, a permute, a float
               conversion, a subtract and a divide, then one stack per key
  batched      one advanced-indexing gather per key with index tensors built from the parameter
               table, then permute / float / subtract / divide per key

Wall time between two HIP events around `--iters` back-to-back calls, so host-side launch cost
counts where the path is host-bound; the paths alternate within every one of `--rounds` rounds and
the median and the range over the rounds are reported, per call.  Every path's outputs are compared
bit for bit once before timing.  `bytes` are the bytes the step has to move (every cropped source
element read once, every result element written once); `TB_per_s` is bytes over the median time,
next to the plane-copy ceiling of 5.1-5.4 TB/s reading and writing.  One JSON line per shape.

Usage: python tools/bench_augment.py [--iters 50] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nicr_mt_scene_analysis_amd import ops                                      # noqa: E402
from nicr_mt_scene_analysis_amd.data.preprocessing.augmentation import RGB_MEAN, RGB_STD      # noqa: E402

SHAPES = {'B32_480x640': 32, 'configs2_B64_480x640': 64}
H, W, CROP_H, CROP_W = 488, 648, 480, 640
DEPTH_MEAN, DEPTH_STD = 2841.94941272766, 1417.2594281672277


def make_batch(B, dev):
    g = torch.Generator(device=dev).manual_seed(11)
    return {
        'rgb': torch.randint(0, 256, (B, H, W, 3), device=dev, generator=g).to(torch.uint8),
        'depth': torch.randint(0, 65536, (B, H, W), device=dev, generator=g).to(torch.uint16),
        'semantic': torch.randint(0, 41, (B, H, W), device=dev, generator=g).to(torch.uint8),
        'instance': torch.randint(0, 65536, (B, H, W), device=dev, generator=g).to(torch.int32),
        'normal': torch.randn((B, H, W, 3), device=dev, generator=g),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    dev = torch.device('cuda:0')
    mean, std = (torch.from_numpy(a).to(dev)[:, None, None] for a in (RGB_MEAN, RGB_STD))
    dmean, dstd = (torch.tensor(v, dtype=torch.float32, device=dev) for v in (DEPTH_MEAN, DEPTH_STD))
    norm = {'rgb': ('rgb_norm', RGB_MEAN, RGB_STD), 'depth': ('depth_norm', DEPTH_MEAN, DEPTH_STD, False, 0.0)}
    for name, B in SHAPES.items():
        batch = make_batch(B, dev)
        rng = np.random.RandomState(3)
        table = np.stack([rng.randint(0, H - CROP_H, B), rng.randint(0, W - CROP_W, B), np.arange(B) % 2], axis=1)
        # torch has few kernels for uint16: its paths move the depth bits as int16 and convert at the end
        as_torch = dict(batch, depth=batch['depth'].view(torch.int16))

        def finish(k, t):
            """t: the cropped, flipped [..., h, w, C] / [..., h, w] of key k -> the collated entry"""
            if k == 'rgb':
                return (t.movedim(-1, -3).float() - mean) / std
            if k == 'depth':
                return ((t.contiguous().view(torch.uint16).float() - dmean) / dstd).unsqueeze(-3)
            return t.movedim(-1, -3).contiguous() if k == 'normal' else t.contiguous()

        def hip():
            return ops.batch_augment(batch, table, (CROP_H, CROP_W), norm)

        def per_sample():
            out = {k: [] for k in as_torch}
            for b, (y0, x0, flip) in enumerate(table.tolist()):
                for k, v in as_torch.items():
                    t = v[b, y0:y0 + CROP_H, x0:x0 + CROP_W]
                    out[k].append(finish(k, t.flip(1) if flip else t))
            return {k: torch.stack(v) for k, v in out.items()}

        def batched():
            t = torch.from_numpy(table).to(dev, non_blocking=True)
            rows = t[:, 0, None] + torch.arange(CROP_H, device=dev)
            ramp = torch.arange(CROP_W, device=dev)
            cols = torch.where(t[:, 2, None] != 0, t[:, 1, None] + (CROP_W - 1) - ramp, t[:, 1, None] + ramp)
            b = torch.arange(B, device=dev)[:, None, None]
            return {k: finish(k, v[b, rows[:, :, None], cols[:, None, :]]) for k, v in as_torch.items()}

        paths = {'hip': hip, 'per_sample': per_sample, 'batched': batched}
        results = {p: fn() for p, fn in paths.items()}
        torch.cuda.synchronize()
        for k in batch:
            a = results['hip'][k]
            for p in ('per_sample', 'batched'):
                assert a.shape == results[p][k].shape and a.dtype == results[p][k].dtype, (p, k)
                assert torch.equal(a.view(torch.uint8), results[p][k].contiguous().view(torch.uint8)), (p, k)
        moved = sum(t.numel() * t.element_size() for t in results['hip'].values()) + \
            sum(B * CROP_H * CROP_W * (v.numel() // (B * H * W)) * v.element_size() for v in batch.values())
        del results
        for fn in paths.values():                   # warm-up of every path at this shape
            for _ in range(5):
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
        print(json.dumps({
            'shape': name, 'source': [H, W], 'crop': [CROP_H, CROP_W], 'keys': list(batch), 'iters': args.iters,
            'rounds': args.rounds, 'bytes': moved, 'plane_copy_ceiling_TB_per_s': [5.1, 5.4],
            'us_per_call': {p: {'median': round(statistics.median(t), 2), 'min': round(min(t), 2),
                                'max': round(max(t), 2)} for p, t in times.items()},
            'TB_per_s': {p: round(moved / statistics.median(t) * 1e-6, 3) for p, t in times.items()}}), flush=True)


if __name__ == '__main__':
    main()
