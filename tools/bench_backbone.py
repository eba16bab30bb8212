"""The stem max pool (`model.pooling.MaxPool2d`: one HIP launch forward, one backward, a one-byte code in place
of ATen's int64 index) against `F.max_pool2d`, and one training step of the EMSANet encoder against the same
module with every fused path off, on the MI355X, in the manner of tools/bench_block.py.

(a) the pool alone: B = 8, C = 64, 240x320 and 256x512 (the stem's map of a 480x640 and a 512x1024 input), float32
    / bfloat16 / float16.  `fwd`: forward under `no_grad` (no code, no index); `train_fwd`: forward with a
    gradient wanted (code / index written); `fwd_bwd`: forward + backward.  torch's side is `F.max_pool2d` on
    the same tensors, not code of this package.
    `derived_bytes`: what each side has to move per call.  Per output pixel and training direction the HIP path
    moves 4 input (gx) elements, 1 output (gy) element and 1 byte of code: 11 B for a half, 21 B for float32;
    ATen moves the same maps and an 8-byte index: 18 B / 28 B.  `TB_per_s` is the derived traffic over the
    median time of the same side.
(b) one training step (forward, backward to the inputs and all parameters) of a resnet34 / NonBottleneck1D
    `FusedRGBDEncoder` ('se-add-uni-rgb') on B x 480x640 rgb + depth in float32 and under bfloat16 autocast,
    against the same module inside `backbone_cases.fused_paths_off()`.

Both sides run eagerly in this process with warm-up; the paths alternate within every one of `--rounds` rounds
of `--iters` back-to-back calls between two HIP events (rounds * iters >= 200 calls for the pool), and the
median and the range over the rounds are reported per call.  `faster` says whether the HIP path's slowest round
beats torch's fastest one; `slower` the reverse.  One JSON line per shape and dtype.

Usage: python tools/bench_backbone.py [--iters 20] [--rounds 10] [--encoder-iters 3] [--batch 8]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nicr_mt_scene_analysis_amd import model                              # noqa: E402
from nicr_mt_scene_analysis_amd.testing import backbone_cases as BC       # noqa: E402

B, C = 8, 64
POOL_SHAPES = ((240, 320), (256, 512))
DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def no_grad(fn):
    def run():
        with torch.no_grad():
            return fn()
    return run


def plain(fn):
    def run():
        with BC.fused_paths_off():
            return fn()
    return run


def measure(paths, iters, rounds, warmup=5):
    for fn in paths.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {p: [] for p in paths}
    for _ in range(rounds):
        for p, fn in paths.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(iters):
                fn()
            stop.record()
            stop.synchronize()
            times[p].append(start.elapsed_time(stop) * 1e3 / iters)
    return times


def report(times, pairs):
    med = {p: statistics.median(t) for p, t in times.items()}
    return med, {
        'us_per_call': {p: {'median': round(med[p], 1), 'min': round(min(t), 1), 'max': round(max(t), 1)}
                        for p, t in times.items()},
        'torch_over_hip': {s: round(med[f'torch_{s}'] / med[f'hip_{s}'], 2) for s in pairs},
        'faster': {s: max(times[f'hip_{s}']) < min(times[f'torch_{s}']) for s in pairs},
        'slower': {s: min(times[f'hip_{s}']) > max(times[f'torch_{s}']) for s in pairs},
    }


def bench_pool(dev, args):
    pool = model.MaxPool2d(3, 2, 1)
    gen = torch.Generator(device=dev).manual_seed(5)
    for (H, W) in POOL_SHAPES:
        for dtype in DTYPES:
            x = torch.relu(torch.randn((B, C, H, W), device=dev, generator=gen)).to(dtype).requires_grad_(True)
            xn = x.detach()
            gy = torch.randn((B, C, H // 2, W // 2), device=dev, generator=gen).to(dtype)
            assert pool.takes_hip_path(x)
            paths = {
                'hip_fwd': no_grad(lambda: pool(xn)), 'torch_fwd': no_grad(lambda: F.max_pool2d(xn, 3, 2, 1)),
                'hip_train_fwd': lambda: pool(x), 'torch_train_fwd': lambda: F.max_pool2d(x, 3, 2, 1),
                'hip_fwd_bwd': lambda: torch.autograd.grad(pool(x), x, gy),
                'torch_fwd_bwd': lambda: torch.autograd.grad(F.max_pool2d(x, 3, 2, 1), x, gy),
            }
            times = measure(paths, args.iters, args.rounds)
            pairs = ('fwd', 'train_fwd', 'fwd_bwd')
            med, out = report(times, pairs)
            e, n_out = x.element_size(), gy.numel()
            moved = {'hip_fwd': 5 * e * n_out, 'torch_fwd': 5 * e * n_out,
                     'hip_train_fwd': (5 * e + 1) * n_out, 'torch_train_fwd': (5 * e + 8) * n_out,
                     'hip_fwd_bwd': 2 * (5 * e + 1) * n_out, 'torch_fwd_bwd': 2 * (5 * e + 8) * n_out}
            out.update({'part': 'pool', 'shape': [B, C, H, W], 'dtype': str(dtype).replace('torch.', ''),
                        'iters': args.iters, 'rounds': args.rounds, 'derived_bytes': moved,
                        'TB_per_s': {p: round(moved[p] / med[p] * 1e-6, 3) for p in moved}})
            print(json.dumps(out), flush=True)
            del x, xn, gy
            torch.cuda.empty_cache()


def bench_encoder(dev, args):
    enc = model.get_encoder(model.get_backbone('resnet34', 'nonbottleneck1d', 3, pretrained=False),
                            model.get_backbone('resnet34', 'nonbottleneck1d', 1, pretrained=False),
                            fusion='se-add-uni-rgb').to(dev).train()
    BC.fill_parameters(enc)
    gen = torch.Generator(device=dev).manual_seed(7)
    rgb = torch.randn((args.batch, 3, 480, 640), device=dev, generator=gen).requires_grad_(True)
    depth = torch.randn((args.batch, 1, 480, 640), device=dev, generator=gen).requires_grad_(True)
    leaves = (rgb, depth) + tuple(enc.parameters())
    for name, dtype in (('float32', None), ('autocast_bfloat16', torch.bfloat16)):
        def step():
            with torch.autocast('cuda', dtype=dtype, enabled=dtype is not None):
                feats, skips = enc({'rgb': rgb, 'depth': depth})
                loss = feats['rgb'].float().sum() + sum(s['rgb'].float().sum() for s in skips.values())
            return torch.autograd.grad(loss, leaves, allow_unused=True)

        times = measure({'hip_step': step, 'torch_step': plain(step)}, args.encoder_iters, args.rounds, warmup=2)
        _, out = report(times, ('step',))
        out.update({'part': 'encoder', 'input': [args.batch, 480, 640], 'precision': name,
                    'iters': args.encoder_iters, 'rounds': args.rounds})
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--encoder-iters', type=int, default=3)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--part', choices=('pool', 'encoder', 'both'), default='both')
    args = ap.parse_args()
    assert args.iters * args.rounds >= 200, 'the median is over at least 200 calls'
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    dev = torch.device('cuda:0')
    if args.part in ('pool', 'both'):
        bench_pool(dev, args)
    if args.part in ('encoder', 'both'):
        bench_encoder(dev, args)


if __name__ == '__main__':
    main()
