"""Swin encoder-decoder fusion: the fused op (`model.encoder_decoder_fusion.SwinFusionFunction`, one
launch forward, one pass plus a small reduction backward) against the reference's formulation as
torch ops (`layer_norm -> permute -> contiguous` for 'select', `layer_norm -> permute -> add` for
'add'; `testing.fusion_ref.torch_formulation`), on the MI355X.

Shapes: the four Swin-T stage outputs of a 640x480 input at B = 16:
[16, 120*160, 96], [16, 60*80, 192], [16, 30*40, 384], [16, 15*20, 768]; dtypes bf16 -> bf16,
bf16 -> f32 (the autocast training case: torch's side runs under `torch.autocast`) and f32 -> f32;
'select' and 'add'; forward and forward + backward (gradients of x, gamma, beta and, for 'add', of
the decoder tensor).  Both paths run eagerly in this process through autograd, with warm-up; the
paths alternate within every one of `--rounds` rounds of `--iters` back-to-back calls between two
HIP events (rounds * iters >= 200 launches), and the median and the range over the rounds are
reported per call.

`algorithmic_bytes`: forward x once, y once, add once, plus 8 B per row of statistics when they are
saved (fwd_bwd); backward gy, x and the statistics read and gx written.  `TB_per_s` is that over
the fused median.  ONE JSON line: `rows` (one entry per shape, dtypes and mode; `beyond_spread` says
whether the fused path's slowest round beats torch's fastest one), `total` (the medians summed over
the four shapes per dtypes and mode, and `fused_faster_in_sum`, the acceptance: the fused sum below
torch's) and `slower_rows` (every single row whose fused median is not below torch's).

Usage: python tools/bench_fusion.py [--iters 20] [--rounds 10] [--only 96]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nicr_mt_scene_analysis_amd.model.encoder_decoder_fusion import SwinFusionFunction      # noqa: E402
from nicr_mt_scene_analysis_amd.testing.fusion_ref import torch_formulation                  # noqa: E402

B = 16
SHAPES = ((120, 160, 96), (60, 80, 192), (30, 40, 384), (15, 20, 768))
DTYPES = (('bf16_bf16', torch.bfloat16, torch.bfloat16), ('bf16_f32', torch.bfloat16, torch.float32),
          ('f32_f32', torch.float32, torch.float32))
EPS = 1e-5


def algorithmic_bytes(H, W, C, dx, dy, add):
    rows, n = B * H * W, B * H * W * C
    ex, ey = torch.empty((), dtype=dx).element_size(), torch.empty((), dtype=dy).element_size()
    fwd = n * ex + n * ey * (2 if add else 1)
    bwd = n * ey + 2 * n * ex + 8 * rows
    return {'fwd': fwd, 'fwd_bwd': fwd + 8 * rows + bwd}


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
    totals, slower, rows = {}, [], []
    for (H, W, C), (dname, dx, dy), add in ((s, d, a) for s in SHAPES for d in DTYPES for a in (False, True)):
        if args.only and args.only != str(C):
            continue
        x = torch.randn((B, H, W, C), device=dev, generator=gen).to(dx).requires_grad_(True)
        gy = torch.randn((B, C, H, W), device=dev, generator=gen).to(dy)
        x_dec = torch.randn((B, C, H, W), device=dev, generator=gen).to(dy).requires_grad_(True) if add else None
        gamma = (1 + 0.25 * torch.randn((C,), device=dev, generator=gen)).requires_grad_(True)
        beta = torch.randn((C,), device=dev, generator=gen).requires_grad_(True)
        # torch's layer_norm wants one dtype outside autocast: parameters in the activations' dtype there
        autocast = dx != dy
        gamma_t, beta_t = ((gamma, beta) if autocast or dx == torch.float32 else
                           tuple(t.detach().to(dx).requires_grad_(True) for t in (gamma, beta)))
        wrt = (x, gamma, beta) + ((x_dec,) if add else ())
        wrt_t = (x, gamma_t, beta_t) + ((x_dec,) if add else ())

        def fused():
            return SwinFusionFunction.apply(x, gamma, beta, x_dec, EPS, dy)

        def formulation():
            with torch.autocast('cuda', dtype=dx, enabled=autocast):
                return torch_formulation(x, gamma_t, beta_t, EPS, x_dec)

        def fused_fwd():
            with torch.no_grad():
                return fused()

        def torch_fwd():
            with torch.no_grad():
                return formulation()

        def fused_fwd_bwd():
            return torch.autograd.grad(fused(), wrt, gy)

        def torch_fwd_bwd():
            return torch.autograd.grad(formulation(), wrt_t, gy)

        paths = {'fused_fwd': fused_fwd, 'torch_fwd': torch_fwd, 'fused_fwd_bwd': fused_fwd_bwd,
                 'torch_fwd_bwd': torch_fwd_bwd}
        assert torch_fwd().dtype == dy and fused_fwd().dtype == dy
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
        moved = algorithmic_bytes(H, W, C, dx, dy, add)
        med = {p: statistics.median(t) for p, t in times.items()}
        mode = 'add' if add else 'select'
        for p in paths:
            totals.setdefault((dname, mode), {}).setdefault(p, 0.0)
            totals[(dname, mode)][p] += med[p]
        for k in moved:
            if med[f'fused_{k}'] >= med[f'torch_{k}']:
                slower.append({'shape': [B, H * W, C], 'dtypes': dname, 'mode': mode, 'path': k})
        rows.append({
            'shape': [B, H * W, C], 'dtypes': dname, 'mode': mode, 'iters': args.iters, 'rounds': args.rounds,
            'us_per_call': {p: {'median': round(med[p], 1), 'min': round(min(t), 1), 'max': round(max(t), 1)}
                            for p, t in times.items()},
            'torch_over_fused': {k: round(med[f'torch_{k}'] / med[f'fused_{k}'], 2) for k in moved},
            'beyond_spread': {k: max(times[f'fused_{k}']) < min(times[f'torch_{k}']) for k in moved},
            'algorithmic_bytes': moved,
            'TB_per_s': {k: round(moved[k] / med[f'fused_{k}'] * 1e-6, 3) for k in moved},
        })
        print(rows[-1]['shape'], dname, mode, rows[-1]['us_per_call'], file=sys.stderr, flush=True)
        del x, gy, x_dec
    print(json.dumps({
        'rows': rows,
        'total': {f'{d}_{m}': {'us': {p: round(v, 1) for p, v in t.items()},
                               'fused_faster_in_sum': {k: t[f'fused_{k}'] < t[f'torch_{k}'] for k in ('fwd', 'fwd_bwd')}}
                  for (d, m), t in totals.items()},
        'slower_rows': slower}), flush=True)


if __name__ == '__main__':
    main()
