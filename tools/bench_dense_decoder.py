"""Dense decoder: the fused x2 upsampling + skip addition (`ops.up2x_add` behind `UpsampleAddFunction`) and a whole
`SemanticDecoder` training step against the reference's composition as torch ops (`Upsampling`, then `torch.add`),
on the MI355X.

Shapes: the three fused steps of a 480x640 EMSANet decoder, x [B, 512, 15, 20], [B, 256, 30, 40] and
[B, 128, 60, 80] with skips of twice the size, B = 8 and 32; float32 and bfloat16; all four upsampling modes.
The decoder reads a 512-channel main map at 1/32 and NCHW skips of (256, 128, 64) channels through 'add-rgb' (the
ResNet34 NonBottleneck1D encoder's: every skip passes the 1x1 adapter), n_channels (512, 256, 128), n_blocks 1,
40 classes, learned-3x3 head upsampling.

Both sides run eagerly in this process through autograd, with warm-up; the paths alternate within every one of
`--rounds` rounds of `--iters` back-to-back calls between two HIP events (rounds * iters >= 200 calls), and the
median and the range over the rounds are reported per call.  `faster` says whether the fused path's slowest round
beats torch's fastest one; `slower` the reverse.

`model_bytes` is the forward step's byte model: x read, skip read, y written: 9 units of the low-resolution map
(the composition moves 17).  `TB_per_s` is that over the fused forward median.  One JSON line per shape, mode and
dtype, then one per decoder configuration.

Usage: python tools/bench_dense_decoder.py [--iters 20] [--rounds 10] [--batch 8] [--skip-module] [--skip-step]
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
from nicr_mt_scene_analysis_amd.model.decoder import UpsampleAddFunction                    # noqa: E402
from nicr_mt_scene_analysis_amd.model.decoder import dense_base                             # noqa: E402
from nicr_mt_scene_analysis_amd.testing import up_add_ref as R                              # noqa: E402

STEPS = ((512, 15, 20), (256, 30, 40), (128, 60, 80))
MODES = R.MODES
N_IN, N_CLASSES, MAIN_HW = 512, 40, (15, 20)
SKIP_CHANNELS, SKIP_DOWNS = (256, 128, 64), (16, 8, 4)


def measure(paths, iters, rounds):
    for fn in paths.values():                       # warm-up of every path at this shape
        for _ in range(5):
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


def report(times, head, extra=None):
    med = {p: statistics.median(t) for p, t in times.items()}
    steps = sorted({p.replace('fused_', '') for p in times if p.startswith('fused_')})
    out = dict(head)
    out['us_per_call'] = {p: {'median': round(med[p], 1), 'min': round(min(t), 1), 'max': round(max(t), 1)}
                          for p, t in times.items()}
    out['torch_over_fused'] = {s: round(med[f'torch_{s}'] / med[f'fused_{s}'], 2) for s in steps}
    out['faster'] = {s: max(times[f'fused_{s}']) < min(times[f'torch_{s}']) for s in steps}
    out['slower'] = {s: min(times[f'fused_{s}']) > max(times[f'torch_{s}']) for s in steps}
    if extra is not None:
        out.update(extra(med))
    print(json.dumps(out), flush=True)


def no_grad(fn):
    def run():
        with torch.no_grad():
            return fn()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--batch', type=int, action='append', help='default: 8 and 32')
    ap.add_argument('--skip-module', action='store_true', help='time the fused step only')
    ap.add_argument('--skip-step', action='store_true', help='time the decoder only')
    args = ap.parse_args()
    assert args.iters * args.rounds >= 200, 'the median is over at least 200 calls'
    assert torch.cuda.is_available(), 'this measurement needs the MI355X'
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(5)
    batches = tuple(args.batch or (8, 32))

    def rand(shape, dtype, grad=False):
        return torch.randn(shape, device=dev, generator=gen).to(dtype).requires_grad_(grad)

    for B in batches:
        for dtype in (torch.float32, torch.bfloat16):
            name = str(dtype).replace('torch.', '')
            for (C, h, w) in (() if args.skip_step else STEPS):
                x, skip = rand((B, C, h, w), dtype, True), rand((B, C, 2 * h, 2 * w), dtype, True)
                gy = rand((B, C, 2 * h, 2 * w), dtype)
                for mode in MODES:
                    learned = R.is_learned(mode)
                    wt = rand((C, 1, 3, 3), torch.float32, True) if learned else None
                    b = rand((C,), torch.float32, True) if learned else None
                    up = model.Upsampling(mode, n_channels=C).to(dev)       # the composition's module
                    leaves = (x, skip) + tuple(up.parameters())
                    fused_leaves = (x, skip) + ((wt, b) if learned else ())
                    paths = {
                        'fused_fwd': no_grad(lambda: UpsampleAddFunction.apply(x, skip, wt, b, mode)),
                        'torch_fwd': no_grad(lambda: torch.add(skip, up(x))),
                        'fused_fwd_bwd': lambda: torch.autograd.grad(UpsampleAddFunction.apply(x, skip, wt, b, mode),
                                                                     fused_leaves, gy),
                        'torch_fwd_bwd': lambda: torch.autograd.grad(torch.add(skip, up(x)), leaves, gy),
                    }
                    times = measure(paths, args.iters, args.rounds)
                    model_bytes = 9 * x.numel() * x.element_size()
                    report(times, {'what': 'step', 'x': [B, C, h, w], 'mode': mode, 'dtype': name, 'iters': args.iters,
                                   'rounds': args.rounds, 'elements_y': skip.numel()},
                           lambda med: {'model_bytes': model_bytes,
                                        'TB_per_s': round(model_bytes / med['fused_fwd'] * 1e-6, 3)})
                del x, skip, gy
                torch.cuda.empty_cache()
            if args.skip_module:
                continue
            for mode in ('bilinear', 'learned-3x3'):
                block = model.get_block_class('nonbottleneck1d')
                module = model.SemanticDecoder(
                    n_channels_in=N_IN, downsampling_in=32, n_channels=tuple(c for c, _, _ in STEPS),
                    downsamplings=SKIP_DOWNS, block=block, n_blocks=1,
                    fusion=model.get_encoder_decoder_fusion_class('add-rgb'), fusion_n_channels=SKIP_CHANNELS,
                    fusion_downsamplings=SKIP_DOWNS, n_classes=N_CLASSES, upsampling=model.get_upsampling_class(mode),
                    prediction_upsampling=model.get_upsampling_class('learned-3x3')).to(dev).to(dtype).train()
                H, W = MAIN_HW
                x = rand((B, N_IN, H, W), dtype, True)
                skips = {str(d): {'rgb': rand((B, c, H * 32 // d, W * 32 // d), dtype, True)}
                         for c, d in zip(SKIP_CHANNELS, SKIP_DOWNS)}
                leaves = (x,) + tuple(s['rgb'] for s in skips.values()) + tuple(module.parameters())
                gys = None
                fused_mode = dense_base._fused_mode

                def decoder(fused):
                    dense_base._fused_mode = fused_mode if fused else (lambda *a: None)
                    try:
                        out, sides = module((x, ()), skips, {}, do_postprocessing=False)
                        return (out,) + tuple(sides)
                    finally:
                        dense_base._fused_mode = fused_mode

                gys = tuple(torch.randn_like(t) for t in decoder(True))
                paths = {
                    'fused_fwd': no_grad(lambda: decoder(True)),
                    'torch_fwd': no_grad(lambda: decoder(False)),
                    'fused_fwd_bwd': lambda: torch.autograd.grad(decoder(True), leaves, gys),
                    'torch_fwd_bwd': lambda: torch.autograd.grad(decoder(False), leaves, gys),
                }
                times = measure(paths, args.iters, args.rounds)
                report(times, {'what': 'SemanticDecoder', 'B': B, 'main': [N_IN, H, W], 'mode': mode, 'dtype': name,
                               'iters': args.iters, 'rounds': args.rounds})
                del module, x, skips, leaves, gys
                torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
