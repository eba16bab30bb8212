#!/usr/bin/env python3
"""`DenseVisualEmbeddingPostprocessing.postprocess` (inference) against what a user of this package
had to write before it existed: torch `norm` / `div_` / `F.conv2d`, followed by the same
`SemanticPostprocessing` class-map entries (`ops.semantic_argmax(_resized)`).  Same process, same
tensors, HIP events, 5 warm-up calls, 4 repetitions of N calls, best repetition.
B = 16, D = 512, one head of C = 40:
  480x640 -> 480x640 (no resize) and 768x1024 -> 960x1280 (bilinear resize).
  python tools/bench_dve_postprocess.py [--heads 2] [--n 10] [--only new|torch] [--shape 0|1]
`--only` / `--shape` restrict the run to one path and one shape (counter collection)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nicr_mt_scene_analysis_amd.data.preprocessing import APPLIED_PREPROCESSING_KEY   # noqa: E402
from nicr_mt_scene_analysis_amd.model.postprocessing import get_postprocessing_class  # noqa: E402
from nicr_mt_scene_analysis_amd.model.postprocessing import SemanticPostprocessing    # noqa: E402
from nicr_mt_scene_analysis_amd.model.postprocessing._lazy import LazyDict            # noqa: E402

B, D, C = 16, 512, 40
SHAPES = (((480, 640), (480, 640)), ((768, 1024), (960, 1280)))
PREFIXES = ('dense_visual_embedding_text_based_', 'dense_visual_embedding_visual_mean_based_')


def timed(fn, n):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(4):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(n):
            fn()
        end.record()
        end.synchronize()
        ms = start.elapsed_time(end) / n
        best = ms if best is None else min(best, ms)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--heads', type=int, default=1, choices=(1, 2))
    ap.add_argument('--n', type=int, default=10)
    ap.add_argument('--only', choices=('new', 'torch'))
    ap.add_argument('--shape', type=int, choices=(0, 1))
    args = ap.parse_args()
    dev = torch.device('cuda')
    g = torch.Generator(device=dev).manual_seed(0)
    weights = [F.normalize(torch.randn((C, D), device=dev, generator=g), dim=1) for _ in range(args.heads)]
    results = []
    for si, ((H, W), (FH, FW)) in enumerate(SHAPES):
        if args.shape is not None and si != args.shape:
            continue
        emb = torch.randn((B, D, H, W), device=dev, generator=g)
        batch = {'rgb_fullres': torch.zeros((B, 3, FH, FW)),
                 APPLIED_PREPROCESSING_KEY: [[{'type': 'Resize', 'valid_region_slice_y': slice(0, H),
                                               'valid_region_slice_x': slice(0, W)}]] * B}
        post = get_postprocessing_class('dense-visual-embedding')(
            with_text_embeddings_per_class=True, text_embeddings_per_class=weights[0],
            with_mean_visual_embedding_per_class=args.heads == 2,
            mean_visual_embedding_per_class=weights[-1])
        w4 = [w[:, :, None, None].contiguous() for w in weights]

        def new():
            return post.postprocess((emb, None), batch, is_training=False)

        def composed():
            r = LazyDict(dense_visual_embedding_output=emb, dense_visual_embedding_side_outputs=None)
            emb.div_(emb.norm(dim=1, keepdim=True))
            for prefix, w in zip(PREFIXES, w4):
                logits = F.conv2d(emb, w)
                r[prefix + 'semantic_output'] = logits
                SemanticPostprocessing._argmax_entries(r, logits, prefix=prefix, stem='semantic')
                SemanticPostprocessing._fullres_entries(r, logits, batch, prefix=prefix, stem='semantic')
            return r

        row = {'shape': f'{B}x{D}x{H}x{W}->{FH}x{FW}', 'heads': args.heads, 'classes': C}
        if args.only != 'torch':
            row['new_ms'] = timed(new, args.n)
            # read 4D + re-read 4D + write 4D + the logits; class maps not counted
            row['new_model_GBps'] = B * H * W * (12 * D + 4 * C * args.heads) / row['new_ms'] / 1e6
        if args.only != 'new':
            row['torch_ms'] = timed(composed, args.n)
        if 'new_ms' in row and 'torch_ms' in row:
            row['speedup'] = row['torch_ms'] / row['new_ms']
        print(json.dumps(row), flush=True)
        results.append(row)
        del emb
        torch.cuda.empty_cache()
    return results


if __name__ == '__main__':
    main()
