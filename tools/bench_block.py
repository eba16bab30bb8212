"""The fused batch-norm tail of the residual blocks (`model.block.batch_norm_tail`: two HIP launches forward,
two backward) and a whole `NonBottleneck1D` against the reference's composition as torch ops
(`nn.BatchNorm2d`, `nn.Dropout2d`, add, activation: the path the same modules take when the fused path is
switched off), on the MI355X.

Shapes: B = 8, the ResNet34 stages / EMSANet decoder modules at 640x480: 64 x 120x160 (1/4), 128 x 60x80,
256 x 30x40, 512 x 15x20 (1/32); float32 and bfloat16 (inputs and convolutions cast, the norms stay float32);
ReLU; training mode;
dropout_p = 0.2.  `tail` is the last segment of a NonBottleneck1D on its own (norm2 -> dropout ->
+ identity -> act2_2), `block` the whole block with its four torch convolutions on both sides.

Both sides run eagerly in this process through autograd with the same parameters, with warm-up; the
paths alternate within every one of `--rounds` rounds of `--iters` back-to-back calls between two HIP
events (rounds * iters >= 200 calls), and the median and the range over the rounds are reported per call.
Forward runs under `no_grad`; forward + backward takes the gradients of the input (the tail: of x and
of the identity) and of all parameters.  `faster` says whether the fused path's slowest round beats
torch's fastest one; `slower` the reverse.  `kernel_us` is the sum of the durations of the library's own
kernels (k_bntail_*) in one forward + backward of the tail, from the profiler's device trace (null when
the profiler gives no device trace): the kernels' own time beside the end-to-end figure.

`algorithmic_bytes` are what the tail has to move at least: forward 4 maps' worth (x read for the
statistics; x and the identity read, y written), backward 8 more (gy, x, y read for the sums; gy, x, y
read, two gradients written).  `TB_per_s` is that over the fused tail's median.  One JSON line per stage
and dtype.

Usage: python tools/bench_block.py [--iters 20] [--rounds 10]
"""
import argparse
import json
import os
import statistics
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nicr_mt_scene_analysis_amd import model                         # noqa: E402
from nicr_mt_scene_analysis_amd.model import block as block_module   # noqa: E402

B = 8
STAGES = ((64, 120, 160), (128, 60, 80), (256, 30, 40), (512, 15, 20))
DROPOUT_P = 0.2


class Tail(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.norm, self.act, self.dropout = nn.BatchNorm2d(C), nn.ReLU(inplace=True), nn.Dropout2d(DROPOUT_P)

    def forward(self, x, identity):
        return block_module.batch_norm_tail(self.norm, self.act, x, identity, self.dropout)


def torch_path(fn):
    """`fn` with the fused path switched off: the same modules run the reference's composition"""
    def run():
        saved = block_module._fused_act
        block_module._fused_act = lambda *a: None
        try:
            return fn()
        finally:
            block_module._fused_act = saved
    return run


def no_grad(fn):
    def run():
        with torch.no_grad():
            return fn()
    return run


def kernel_time_us(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        total = sum(e.device_time_total for e in prof.key_averages() if 'k_bntail' in e.key)
        return round(total, 1) if total > 0 else None
    except Exception:                                               # no device trace on this installation
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=10)
    args = ap.parse_args()
    assert args.iters * args.rounds >= 200, 'the median is over at least 200 calls'
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    dev = torch.device('cuda:0')
    block_module.FUSED_MIN_ELEMENTS = 0         # every shape on the fused path: this table is what sets the threshold
    gen = torch.Generator(device=dev).manual_seed(5)
    for (C, H, W) in STAGES:
        for dtype in (torch.float32, torch.bfloat16):
            def rand(grad=False):
                return (0.3 + torch.randn((B, C, H, W), device=dev, generator=gen)).to(dtype).requires_grad_(grad)

            x, identity, gy = rand(True), rand(True), rand()
            tail = Tail(C).to(dev).train()
            blk = model.NonBottleneck1D(C, C, dropout_p=DROPOUT_P).to(dev).to(dtype).train()
            for m in blk.modules():                     # mixed precision as it is trained: the norms stay float32
                if isinstance(m, nn.BatchNorm2d):
                    m.float()
            tail_leaves = (x, identity) + tuple(tail.parameters())
            blk_leaves = (x,) + tuple(blk.parameters())

            def tail_fwd():
                return tail(x, identity)

            def blk_fwd():
                return blk(x)

            def tail_both():
                return torch.autograd.grad(tail_fwd(), tail_leaves, gy)

            def blk_both():
                return torch.autograd.grad(blk_fwd(), blk_leaves, gy)

            paths = {
                'fused_tail_fwd': no_grad(tail_fwd), 'torch_tail_fwd': torch_path(no_grad(tail_fwd)),
                'fused_tail_fwd_bwd': tail_both, 'torch_tail_fwd_bwd': torch_path(tail_both),
                'fused_block_fwd': no_grad(blk_fwd), 'torch_block_fwd': torch_path(no_grad(blk_fwd)),
                'fused_block_fwd_bwd': blk_both, 'torch_block_fwd_bwd': torch_path(blk_both),
            }
            for fn in paths.values():                   # warm-up of every path at this shape
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            kernel_us = kernel_time_us(tail_both)
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
            one_map = x.numel() * x.element_size()
            moved = {'fwd': 4 * one_map, 'fwd_bwd': 12 * one_map}
            med = {p: statistics.median(t) for p, t in times.items()}
            pairs = [f'{what}_{s}' for what in ('tail', 'block') for s in ('fwd', 'fwd_bwd')]
            print(json.dumps({
                'stage': [C, H, W], 'B': B, 'dtype': str(dtype).replace('torch.', ''), 'iters': args.iters,
                'rounds': args.rounds,
                'us_per_call': {p: {'median': round(med[p], 1), 'min': round(min(t), 1), 'max': round(max(t), 1)}
                                for p, t in times.items()},
                'torch_over_fused': {s: round(med[f'torch_{s}'] / med[f'fused_{s}'], 2) for s in pairs},
                'faster': {s: max(times[f'fused_{s}']) < min(times[f'torch_{s}']) for s in pairs},
                'slower': {s: min(times[f'fused_{s}']) > max(times[f'torch_{s}']) for s in pairs},
                'kernel_us': {'tail_fwd_bwd': kernel_us},
                'algorithmic_bytes': moved,
                'TB_per_s': {s: round(moved[s] / med[f'fused_tail_{s}'] * 1e-6, 3) for s in moved},
                'kernel_TB_per_s': None if not kernel_us else round(moved['fwd_bwd'] / kernel_us * 1e-6, 3),
            }), flush=True)
            del x, identity, gy, tail, blk, tail_leaves, blk_leaves
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
