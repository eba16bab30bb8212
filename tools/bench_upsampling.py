"""Learned x2 upsampling: the fused op (`ops.upsample2x_dw3x3`, one launch forward, one pass plus a
small reduction backward) against the reference's formulation as torch ops (`interpolate` ->
`ReplicationPad2d` -> depthwise `conv2d`, and the zero-pad form), on the MI355X.

Shapes: the two x2 stages of the bench configuration's heads (120x160 -> 240x320 and 240x320 ->
480x640, B = 32) for the semantic (C = 40), instance (C = 5) and normal (C = 3) head, in float32
and bfloat16, both pad modes, forward and forward + backward.  Both paths run eagerly in this
process through autograd (`torch.autograd.grad` for x, weight and bias), with warm-up; the paths
alternate within every one of `--rounds` rounds of `--iters` back-to-back calls between two HIP
events (rounds * iters >= 200 launches), and the median and the range over the rounds are reported
per call.  `faster` says whether the fused path's slowest round beats torch's fastest one, i.e. the
difference exceeds the run-to-run spread of the two.

`algorithmic_bytes` are 5 units forward (x read, y written) and 6 more backward (gy and x read, gx
written), one unit being the input tensor's size; `TB_per_s` is that over the fused median, and
`of_plane_copy` its fraction of the project's plane-copy rate (5.1 TB/s, the lower end of
tools/ceiling/plane_copy.hip's 5.1-5.4).  One JSON line per shape.

Usage: python tools/bench_upsampling.py [--iters 20] [--rounds 10] [--only C40]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nicr_mt_scene_analysis_amd.model.upsampling import LearnedUpsamplingFunction      # noqa: E402
from nicr_mt_scene_analysis_amd.testing.upsampling_ref import torch_formulation          # noqa: E402

B = 32
HEADS = {'semantic_C40': 40, 'instance_C5': 5, 'normal_C3': 3}
STAGES = ((120, 160), (240, 320))
PLANE_COPY_TB_PER_S = 5.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--only', default='')
    args = ap.parse_args()
    assert args.iters * args.rounds >= 200, 'the median is over at least 200 launches'
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(5)
    for (head, C), (h, w), dtype, zeropad in ((a, b, c, d) for a in HEADS.items() for b in STAGES
                                              for c in (torch.float32, torch.bfloat16) for d in (False, True)):
        if args.only not in head:
            continue
        x = torch.randn((B, C, h, w), device=dev, generator=gen).to(dtype).requires_grad_(True)
        gy = torch.randn((B, C, 2 * h, 2 * w), device=dev, generator=gen).to(dtype)
        wt = (torch.randn((C, 1, 3, 3), device=dev, generator=gen) * 0.25).requires_grad_(True)
        bias = torch.randn((C,), device=dev, generator=gen).requires_grad_(True)
        # torch's convolution wants one dtype: its parameters in the activations' (what autocast does)
        wt_t, bias_t = (t.detach().to(dtype).requires_grad_(True) for t in (wt, bias))

        def fused_fwd():
            with torch.no_grad():
                return LearnedUpsamplingFunction.apply(x, wt, bias, zeropad)

        def torch_fwd():
            with torch.no_grad():
                return torch_formulation(x, wt_t, bias_t, zeropad)

        def fused_fwd_bwd():
            return torch.autograd.grad(LearnedUpsamplingFunction.apply(x, wt, bias, zeropad), (x, wt, bias), gy)

        def torch_fwd_bwd():
            return torch.autograd.grad(torch_formulation(x, wt_t, bias_t, zeropad), (x, wt_t, bias_t), gy)

        paths = {'fused_fwd': fused_fwd, 'torch_fwd': torch_fwd, 'fused_fwd_bwd': fused_fwd_bwd,
                 'torch_fwd_bwd': torch_fwd_bwd}
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
        unit = x.numel() * x.element_size()
        moved = {'fwd': 5 * unit, 'fwd_bwd': 11 * unit}
        med = {p: statistics.median(t) for p, t in times.items()}
        print(json.dumps({
            'head': head, 'shape': [B, C, h, w], 'dtype': str(dtype).replace('torch.', ''),
            'pad': 'zero' if zeropad else 'replicate', 'iters': args.iters, 'rounds': args.rounds,
            'us_per_call': {p: {'median': round(med[p], 1), 'min': round(min(t), 1), 'max': round(max(t), 1)}
                            for p, t in times.items()},
            'torch_over_fused': {k: round(med[f'torch_{k}'] / med[f'fused_{k}'], 2) for k in moved},
            'faster': {k: max(times[f'fused_{k}']) < min(times[f'torch_{k}']) for k in moved},
            'algorithmic_bytes': moved,
            'TB_per_s': {k: round(moved[k] / med[f'fused_{k}'] * 1e-6, 3) for k in moved},
            'of_plane_copy': {k: round(moved[k] / med[f'fused_{k}'] * 1e-6 / PLANE_COPY_TB_PER_S, 3) for k in moved},
        }), flush=True)
        del x, gy


if __name__ == '__main__':
    main()
