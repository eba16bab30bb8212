"""Encoder RGB-D fusion 'se-add' (`model.EncoderRGBDFusionWeightedAdd`: three HIP launches forward,
three backward) against the reference's composition as torch ops (`testing.encoder_fusion_ref.
torch_formulation`: two poolings, four 1x1 convolutions, two activations, two sigmoids, two broadcast
multiplies and an add), on the MI355X.

Shapes: B = 8, the five stages of a ResNet34 encoder at 640x480 (64 x 240x320, 64 x 120x160,
128 x 60x80, 256 x 30x40, 512 x 15x20) and at 1024x512 (64 x 256x512 ... 512 x 16x32); float32 and
bfloat16 (module and inputs cast); ReLU.

Both sides run eagerly in this process through autograd with the same parameters, with warm-up; the
paths alternate within every one of `--rounds` rounds of `--iters` back-to-back calls between two
HIP events (rounds * iters >= 200 calls), and the median and the range over the rounds are reported per
call.  Forward runs under `no_grad`; forward + backward takes the gradients of both maps and of all
eight parameters.  `faster` says whether the fused path's slowest round beats torch's fastest one;
`slower` the reverse.

`algorithmic_bytes` are what the fusion has to move at least: forward 5 maps' worth (two read for the
squeeze, two read and one written by the weighted add), backward 6 more (gy and both maps read for
the weight gradient, gy read and two gradients written).  `TB_per_s` is that over the fused median.
One JSON line per stage and dtype.

Usage: python tools/bench_encoder_fusion.py [--iters 20] [--rounds 10] [--only 640x480]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nicr_mt_scene_analysis_amd import model                                                # noqa: E402
from nicr_mt_scene_analysis_amd.testing.encoder_fusion_ref import torch_formulation         # noqa: E402

B = 8
STAGES = {
    '640x480': ((64, 240, 320), (64, 120, 160), (128, 60, 80), (256, 30, 40), (512, 15, 20)),
    '1024x512': ((64, 256, 512), (64, 128, 256), (128, 64, 128), (256, 32, 64), (512, 16, 32)),
}
ACT = 'relu'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--only', default='')
    args = ap.parse_args()
    assert args.iters * args.rounds >= 200, 'the median is over at least 200 calls'
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(5)
    configs = ((inp, stage, d) for inp, stages in STAGES.items() for stage in stages
               for d in (torch.float32, torch.bfloat16))
    for inp, (C, H, W), dtype in configs:
        if args.only and args.only != inp:
            continue

        def rand(grad=False):
            return (0.3 + torch.randn((B, C, H, W), device=dev, generator=gen)).to(dtype).requires_grad_(grad)

        x_rgb, x_depth, gy = rand(True), rand(True), rand()
        module = model.get_encoder_fusion_class('se-add')(
            n_channels_in=C, input_memory_layout='nchw',
            activation=model.activation.get_activation_class(ACT)).to(dev).to(dtype).train()
        params = tuple((se.layers[0].weight, se.layers[0].bias, se.layers[2].weight, se.layers[2].bias)
                       for se in (module.weighting_rgb, module.weighting_depth))
        leaves = (x_rgb, x_depth) + params[0] + params[1]

        def fused():
            return module({'rgb': x_rgb, 'depth': x_depth})['rgb']

        def composed():
            return torch_formulation(x_rgb, x_depth, params, ACT)

        def no_grad(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run

        paths = {
            'fused_fwd': no_grad(fused), 'torch_fwd': no_grad(composed),
            'fused_fwd_bwd': lambda: torch.autograd.grad(fused(), leaves, gy),
            'torch_fwd_bwd': lambda: torch.autograd.grad(composed(), leaves, gy),
        }
        for fn in paths.values():                   # warm-up of every path at this shape
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        with torch.no_grad():
            diff = float((fused().float() - composed().float()).abs().max())
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
        one_map = x_rgb.numel() * x_rgb.element_size()
        moved = {'fwd': 5 * one_map, 'fwd_bwd': 11 * one_map}
        med = {p: statistics.median(t) for p, t in times.items()}
        print(json.dumps({
            'input': inp, 'stage': [C, H, W], 'B': B, 'dtype': str(dtype).replace('torch.', ''), 'act': ACT,
            'iters': args.iters, 'rounds': args.rounds,
            'us_per_call': {p: {'median': round(med[p], 1), 'min': round(min(t), 1), 'max': round(max(t), 1)}
                            for p, t in times.items()},
            'torch_over_fused': {s: round(med[f'torch_{s}'] / med[f'fused_{s}'], 2) for s in moved},
            'faster': {s: max(times[f'fused_{s}']) < min(times[f'torch_{s}']) for s in moved},
            'slower': {s: min(times[f'fused_{s}']) > max(times[f'torch_{s}']) for s in moved},
            'launches': {'fused': {'fwd': 3, 'bwd': 3}, 'torch': {'fwd': 13}},
            'algorithmic_bytes': moved,
            'TB_per_s': {s: round(moved[s] / med[f'fused_{s}'] * 1e-6, 3) for s in moved},
            'max_abs_diff_fwd': diff,
        }), flush=True)
        del x_rgb, x_depth, gy, module, params, leaves
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
