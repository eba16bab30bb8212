"""MLP decoder: the fused resize + concatenation step (`ops.mlpdec_upsample_concat` and its backward
kernel behind `MlpUpsampleConcatFunction`) and the whole `SemanticMLPDecoder` against the reference's
composition as torch ops (one `interpolate` per branch, one `cat`), on the MI355X.

Shapes: B = 8 at 640x480 (the 1/4-resolution grid is 120x160, the main map 15x20) and at 1024x512
(128x256, 16x32); branch channels `n_channels` (256, 128, 64, 64) and (256, 256, 256, 256) at factors
(8, 4, 2, 1); float32 and bfloat16 (module and inputs cast); bilinear.  The channel tuples are this
tool's choice, not a measured user configuration.  The decoder reads a 512-channel main map and
NHWC skips of (384, 192, 96) channels through 'swin-ln-select', 40 classes.

Both sides run eagerly in this process through autograd, with warm-up; the paths alternate within
every one of `--rounds` rounds of `--iters` back-to-back calls between two HIP events (rounds * iters
>= 200 calls), and the median and the range over the rounds are reported per call.  `faster` says
whether the fused path's slowest round beats torch's fastest one; `slower` the reverse.

`algorithmic_bytes` are what the step has to move at least: forward the branch maps read and the
concatenation written; backward the channels of its gradient that belong to a resized branch read and
those branches' gradients written (the gradient of the factor-1 branch is a view).  `TB_per_s` is that
over the fused median.  One JSON line per shape, channel tuple and dtype.

Usage: python tools/bench_mlp_decoder.py [--iters 20] [--rounds 10] [--only 640x480]
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
from nicr_mt_scene_analysis_amd.model.decoder import MlpUpsampleConcatFunction              # noqa: E402
from nicr_mt_scene_analysis_amd.model.decoder import mlp_base                               # noqa: E402
from nicr_mt_scene_analysis_amd.testing.mlp_decoder_ref import torch_upcat                  # noqa: E402

B, N_IN, N_CLASSES = 8, 512, 40
SKIP_CHANNELS, SKIP_DOWNS, FACTORS = (384, 192, 96), (16, 8, 4), (8, 4, 2, 1)
# (input, the 1/4-resolution grid)
SHAPES = (('640x480', (120, 160)), ('1024x512', (128, 256)))
CHANNELS = ((256, 128, 64, 64), (256, 256, 256, 256))
MODE = 'bilinear'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--only', default='')
    ap.add_argument('--skip-module', action='store_true', help='time the fused step only')
    args = ap.parse_args()
    assert args.iters * args.rounds >= 200, 'the median is over at least 200 calls'
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(5)
    configs = ((s, c, d) for s in SHAPES for c in CHANNELS for d in (torch.float32, torch.bfloat16))
    for (inp, (H, W)), channels, dtype in configs:
        if args.only and args.only != inp:
            continue

        def rand(shape, grad=False):
            return torch.randn(shape, device=dev, generator=gen).to(dtype).requires_grad_(grad)

        ys = tuple(rand((B, c, H // f, W // f), True) for c, f in zip(channels, FACTORS))
        g_cat = rand((B, sum(channels), H, W))
        module = model.SemanticMLPDecoder(
            n_channels_in=N_IN, downsampling_in=32, n_channels=channels,
            fusion=model.get_encoder_decoder_fusion_class('swin-ln-select'), fusion_n_channels=SKIP_CHANNELS,
            fusion_downsamplings=SKIP_DOWNS, n_classes=N_CLASSES,
            upsampling=model.get_upsampling_class(MODE)).to(dev).to(dtype).train()
        x = rand((B, N_IN, H // 8, W // 8), True)
        skips = {str(d): {'rgb': rand((B, H * 4 // d, W * 4 // d, c), True)} for c, d in zip(SKIP_CHANNELS, SKIP_DOWNS)}
        leaves = (x,) + tuple(s['rgb'] for s in skips.values()) + tuple(module.parameters())
        gy = rand((B, N_CLASSES, 4 * H, 4 * W))
        fused_mode = mlp_base._fused_mode

        def decoder(fused):
            mlp_base._fused_mode = fused_mode if fused else (lambda *a: None)
            try:
                return module((x, ()), skips, {}, do_postprocessing=False)[0]
            finally:
                mlp_base._fused_mode = fused_mode

        def no_grad(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run

        paths = {
            'upcat_fused_fwd': no_grad(lambda: MlpUpsampleConcatFunction.apply(MODE, *ys)),
            'upcat_torch_fwd': no_grad(lambda: torch_upcat(ys, MODE)),
            'upcat_fused_fwd_bwd': lambda: torch.autograd.grad(MlpUpsampleConcatFunction.apply(MODE, *ys), ys, g_cat),
            'upcat_torch_fwd_bwd': lambda: torch.autograd.grad(torch_upcat(ys, MODE), ys, g_cat),
        }
        if not args.skip_module:
            paths.update({
                'module_fused_fwd': no_grad(lambda: decoder(True)),
                'module_torch_fwd': no_grad(lambda: decoder(False)),
                'module_fused_fwd_bwd': lambda: torch.autograd.grad(decoder(True), leaves, gy),
                'module_torch_fwd_bwd': lambda: torch.autograd.grad(decoder(False), leaves, gy),
            })
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
        e = g_cat.element_size()
        ny, ncat = sum(y.numel() for y in ys), g_cat.numel()
        resized = sum(y.numel() for y, f in zip(ys, FACTORS) if f > 1)
        g_resized = sum(B * c * H * W for c, f in zip(channels, FACTORS) if f > 1)
        moved = {'upcat_fwd': e * (ny + ncat), 'upcat_fwd_bwd': e * (ny + ncat + g_resized + resized)}
        med = {p: statistics.median(t) for p, t in times.items()}
        steps = sorted({p.replace('_fused', '').replace('_torch', '') for p in paths})

        def pair(step):
            part, _, direction = step.partition('_')
            return f'{part}_fused_{direction}', f'{part}_torch_{direction}'

        print(json.dumps({
            'input': inp, 'grid': [H, W], 'n_channels': list(channels), 'factors': list(FACTORS), 'B': B,
            'dtype': str(dtype).replace('torch.', ''), 'iters': args.iters, 'rounds': args.rounds,
            'us_per_call': {p: {'median': round(med[p], 1), 'min': round(min(t), 1), 'max': round(max(t), 1)}
                            for p, t in times.items()},
            'torch_over_fused': {s: round(med[pair(s)[1]] / med[pair(s)[0]], 2) for s in steps},
            'faster': {s: max(times[pair(s)[0]]) < min(times[pair(s)[1]]) for s in steps},
            'slower': {s: min(times[pair(s)[0]]) > max(times[pair(s)[1]]) for s in steps},
            'launches': {'fused': {'upcat_fwd': 1, 'upcat_bwd': 1},
                         'torch': {'upcat_fwd': len(ys) + 1, 'upcat_bwd': 2 * len(ys)}},
            'algorithmic_bytes': moved,
            'TB_per_s': {s: round(moved[s] / med[pair(s)[0]] * 1e-6, 3) for s in moved},
        }), flush=True)
        del ys, g_cat, module, x, skips, leaves, gy
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
