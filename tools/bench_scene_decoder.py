"""Scene classification decoder: the fused node (`SceneHeadFunction`: one launch forward, one backward) against
the reference's composition as torch ops (`adaptive_avg_pool2d -> flatten -> linear`), on the MI355X.

Shapes: the map the decoder pools, [B, 128, 1, 1] (the pyramid pooling module's bin-1 branch), [B, 128, 2, 3]
(the adaptive module at a larger validation input) and [B, 512, 15, 20] (no context module: the encoder's output
at 640x480), B in {8, 64}, K in {10, 45} classes, float32 and bfloat16.  In bfloat16 the torch side runs a module
cast to bfloat16 (no cast kernels in the timed region: torch's best case), the fused side reads the bfloat16
map and its float32 master weights.  The fused side is the node itself (`SceneHeadFunction`), also at shapes the
module routes to torch (`module_routes_to`), so that the routing constant stays measurable.

Both sides run eagerly in this process through autograd, with warm-up, and forward + backward once more as a
captured `torch.cuda.graph` that is replayed (`graph_fwd_bwd`); the paths alternate within every one of
`--rounds` rounds of `--iters` back-to-back calls between two HIP events (rounds * iters >= 200 calls), and the
median and the range over the rounds are reported per call.  `faster` says whether the fused path's slowest
round beats torch's fastest one; `slower` the reverse.  One JSON line per shape, class count and dtype.

Usage: python tools/bench_scene_decoder.py [--iters 20] [--rounds 10] [--only 512x15x20]
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nicr_mt_scene_analysis_amd import model                                                # noqa: E402
from nicr_mt_scene_analysis_amd.testing.scene_head_ref import torch_composition             # noqa: E402

MAPS = ((128, 1, 1), (128, 2, 3), (512, 15, 20))
BATCHES = (8, 64)
CLASSES = (10, 45)


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
    configs = ((m, B, K, d) for m in MAPS for B in BATCHES for K in CLASSES for d in (torch.float32, torch.bfloat16))
    for (C, H, W), B, K, dtype in configs:
        if args.only and args.only != f'{C}x{H}x{W}':
            continue
        x = torch.randn((B, C, H, W), device=dev, generator=gen).to(dtype).requires_grad_(True)
        g = torch.randn((B, K), device=dev, generator=gen).to(dtype)
        fused = model.SceneClassificationDecoder(C, K).to(dev).train()
        plain = copy.deepcopy(fused).to(dtype)
        head = plain._task_head
        routed = 'hip' if fused.takes_hip_path(x) else 'torch'
        fused_leaves = (x,) + tuple(fused.parameters())
        plain_leaves = (x,) + tuple(plain.parameters())
        fused_head = fused._task_head

        def run_fused():
            # the node itself, so that shapes the module routes to torch stay measured
            return model.SceneHeadFunction.apply(x, fused_head.weight, fused_head.bias, dtype, torch.is_grad_enabled())

        def run_torch():
            return torch_composition(x, head.weight, head.bias)

        def no_grad(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run

        paths = {
            'fused_fwd': no_grad(run_fused),
            'torch_fwd': no_grad(run_torch),
            'fused_fwd_bwd': lambda: torch.autograd.grad(run_fused(), fused_leaves, g),
            'torch_fwd_bwd': lambda: torch.autograd.grad(run_torch(), plain_leaves, g),
        }
        for fn in paths.values():                   # warm-up of every path at this shape
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        # the same forward + backward as a captured graph: what the device does without the host's eager cost
        graphs = []
        for p in ('fused_fwd_bwd', 'torch_fwd_bwd'):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                kept = paths[p]()
            graphs.append((graph, kept))
            paths[p.replace('fwd_bwd', 'graph_fwd_bwd')] = graph.replay
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
        med = {p: statistics.median(t) for p, t in times.items()}
        steps = ('fwd', 'fwd_bwd', 'graph_fwd_bwd')
        print(json.dumps({
            'map': [B, C, H, W], 'K': K, 'dtype': str(dtype).replace('torch.', ''), 'iters': args.iters,
            'rounds': args.rounds,
            'us_per_call': {p: {'median': round(med[p], 1), 'min': round(min(t), 1), 'max': round(max(t), 1)}
                            for p, t in times.items()},
            'torch_over_fused': {s: round(med[f'torch_{s}'] / med[f'fused_{s}'], 2) for s in steps},
            'faster': {s: max(times[f'fused_{s}']) < min(times[f'torch_{s}']) for s in steps},
            'slower': {s: min(times[f'fused_{s}']) > max(times[f'torch_{s}']) for s in steps},
            'map_bytes': x.numel() * x.element_size(), 'module_routes_to': routed,
        }), flush=True)
        del x, g, fused, plain, graphs, paths
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
