"""Context module: the two fused steps (`ops.ppm_pool`, `ops.ppm_upsample_concat` and their backward
kernels behind `PyramidPoolFunction` / `UpsampleConcatFunction`) and the whole module against the
reference's formulation as torch ops (n `adaptive_avg_pool2d`, n `interpolate`, one `cat`), on the
MI355X.

Shapes: the sizes a user runs, all at B = 8 with C = 512 (and 256 output channels for the module):
640x480 -> 15x20 'ppm-1-5', 1024x512 -> 16x32 'ppm-1-2-4-8', 1280x960 -> 30x40 'ppm-1-5-10',
2048x1024 -> 32x64 'appm-1-2-4-8' built for 1024x512; float32 and bfloat16 (module and input cast),
bilinear.  Both sides run eagerly in this process through autograd, with warm-up; the paths
alternate within every one of `--rounds` rounds of `--iters` back-to-back calls between two HIP
events (rounds * iters >= 200 calls), and the median and the range over the rounds are reported per
call.  `faster` says whether the fused path's slowest round beats torch's fastest one, i.e. the
difference exceeds the run-to-run spread of the two.

`launches` are counted from the formulation, not traced: fused 1 per step and direction; torch n
pools and n resizes + 1 cat forward, and backward n resize-backwards + n pool-backwards + the n + 1
slice copies of cat's backward + n accumulations into the gradient of x.
`algorithmic_bytes` are what each step has to move at least (pool: x read, the pooled maps written;
backward the reverse.  upcat: x and the branch maps read, the concatenation written; backward the
branch channels of its gradient read, the branch gradients written); `TB_per_s` is that over the
fused median.  One JSON line per shape and dtype.

Usage: python tools/bench_context_module.py [--iters 20] [--rounds 10] [--only ppm-1-5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nicr_mt_scene_analysis_amd import ops                                                  # noqa: E402
from nicr_mt_scene_analysis_amd.model import context_module as cm                           # noqa: E402
from nicr_mt_scene_analysis_amd.model.context_module.ppm import PyramidPoolFunction        # noqa: E402
from nicr_mt_scene_analysis_amd.model.context_module.ppm import UpsampleConcatFunction     # noqa: E402
from nicr_mt_scene_analysis_amd.testing.context_ref import torch_pool, torch_upcat          # noqa: E402

B, C, C_OUT = 8, 512, 256
# (input, feature map, name, input_size of the module)
SHAPES = (('640x480', (15, 20), 'ppm-1-5', (15, 20)), ('1024x512', (16, 32), 'ppm-1-2-4-8', (16, 32)),
          ('1280x960', (30, 40), 'ppm-1-5-10', (30, 40)), ('2048x1024', (32, 64), 'appm-1-2-4-8', (16, 32)))
MODE = 'bilinear'


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
    for (inp, (H, W), name, input_size), dtype in ((s, d) for s in SHAPES for d in (torch.float32, torch.bfloat16)):
        if args.only and args.only != name:
            continue
        module = cm.get_context_module(name, C, C_OUT, input_size, upsampling=MODE).to(dev).to(dtype)
        sizes = module.pool_sizes(H, W) if name.startswith('appm') else ops._ppm_sizes(module._bins)
        n, cr = len(sizes), module.n_channels_reduction

        def rand(shape, grad=False):
            return torch.randn(shape, device=dev, generator=gen).to(dtype).requires_grad_(grad)

        x = rand((B, C, H, W), True)
        ys = tuple(rand((B, cr, ph, pw), True) for ph, pw in sizes)
        gps = tuple(rand((B, C, ph, pw)) for ph, pw in sizes)
        g_cat = rand((B, C + n * cr, H, W))
        gy = rand((B, C_OUT, H, W))
        params = tuple(module.parameters())

        def twin(t):
            feats = tuple(f[1](p) for f, p in zip(module.features, torch_pool(t, sizes)))
            return module.final_conv(torch_upcat(t, feats, MODE))

        def no_grad(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run

        paths = {
            'pool_fused_fwd': no_grad(lambda: PyramidPoolFunction.apply(x, sizes)),
            'pool_torch_fwd': no_grad(lambda: torch_pool(x, sizes)),
            'pool_fused_fwd_bwd': lambda: torch.autograd.grad(PyramidPoolFunction.apply(x, sizes), (x,), gps),
            'pool_torch_fwd_bwd': lambda: torch.autograd.grad(torch_pool(x, sizes), (x,), gps),
            'upcat_fused_fwd': no_grad(lambda: UpsampleConcatFunction.apply(MODE, x, *ys)),
            'upcat_torch_fwd': no_grad(lambda: torch_upcat(x, ys, MODE)),
            'upcat_fused_fwd_bwd': lambda: torch.autograd.grad(UpsampleConcatFunction.apply(MODE, x, *ys),
                                                               (x,) + ys, g_cat),
            'upcat_torch_fwd_bwd': lambda: torch.autograd.grad(torch_upcat(x, ys, MODE), (x,) + ys, g_cat),
            'module_fused_fwd': no_grad(lambda: module(x)[0]),
            'module_torch_fwd': no_grad(lambda: twin(x)),
            'module_fused_fwd_bwd': lambda: torch.autograd.grad(module(x)[0], (x,) + params, gy),
            'module_torch_fwd_bwd': lambda: torch.autograd.grad(twin(x), (x,) + params, gy),
        }
        module.train()
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
        e = x.element_size()
        nx, npool = x.numel(), sum(B * C * ph * pw for ph, pw in sizes)
        ny, ncat = sum(y.numel() for y in ys), g_cat.numel()
        moved = {'pool_fwd': e * (nx + npool), 'pool_fwd_bwd': 2 * e * (nx + npool),
                 'upcat_fwd': e * (nx + ny + ncat), 'upcat_fwd_bwd': e * (nx + ny + ncat + (ncat - nx) + ny)}
        med = {p: statistics.median(t) for p, t in times.items()}
        steps = ('pool_fwd', 'pool_fwd_bwd', 'upcat_fwd', 'upcat_fwd_bwd', 'module_fwd', 'module_fwd_bwd')

        def pair(step):
            part, _, direction = step.partition('_')
            return f'{part}_fused_{direction}', f'{part}_torch_{direction}'

        print(json.dumps({
            'input': inp, 'name': name, 'x': [B, C, H, W], 'pools': [list(s) for s in sizes], 'cr': cr,
            'dtype': str(dtype).replace('torch.', ''), 'iters': args.iters, 'rounds': args.rounds,
            'us_per_call': {p: {'median': round(med[p], 1), 'min': round(min(t), 1), 'max': round(max(t), 1)}
                            for p, t in times.items()},
            'torch_over_fused': {s: round(med[pair(s)[1]] / med[pair(s)[0]], 2) for s in steps},
            'faster': {s: max(times[pair(s)[0]]) < min(times[pair(s)[1]]) for s in steps},
            'slower': {s: min(times[pair(s)[0]]) > max(times[pair(s)[1]]) for s in steps},
            'launches': {'fused': {'pool_fwd': 1, 'pool_bwd': 1, 'upcat_fwd': 1, 'upcat_bwd': 1},
                         'torch': {'pool_fwd': n, 'pool_bwd': 2 * n, 'upcat_fwd': n + 1, 'upcat_bwd': 2 * n + 1}},
            'algorithmic_bytes': moved,
            'TB_per_s': {s: round(moved[s] / med[pair(s)[0]] * 1e-6, 3) for s in moved},
        }), flush=True)
        del x, ys, gps, g_cat, gy, module


if __name__ == '__main__':
    main()
