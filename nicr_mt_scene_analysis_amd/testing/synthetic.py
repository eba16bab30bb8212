"""
Deterministic synthetic inputs of the shapes in SURVEY.md §8d.

Everything is generated with numpy (PCG64) in float64 using only + - * / and
one `exp` per heatmap pixel, then rounded once to float32, so that the same
seed gives bit-identical arrays in the build container and on the GPU box
(`input_digest` lets a test verify that before trusting a committed golden).

Layouts/dtypes follow what the reference's decoders/targets produce:
  semantic logits  [B,C,H,W] f32          (model/decoder: raw, pre-softmax)
  instance center  [B,1,H,W] f32 in [0,1] (sigmoid head; targets are Gaussians,
                                            data/preprocessing/instance.py:143-150)
  instance offset  [B,2,H,W] f32, (dy,dx) normalised by (H,W)
                                           (data/preprocessing/instance.py:252-256)
  orientation      [B,2,H,W] f32 unit biternion (cos, sin)
"""
import hashlib
import json
from typing import Dict

import numpy as np


def _bilinear_up(coarse: np.ndarray, H: int, W: int) -> np.ndarray:
    """align_corners=False bilinear upsample of [..., h, w] -> [..., H, W] (f64)."""
    h, w = coarse.shape[-2:]
    ys = (np.arange(H, dtype=np.float64) + 0.5) * (h / H) - 0.5
    xs = (np.arange(W, dtype=np.float64) + 0.5) * (w / W) - 0.5
    ys = np.clip(ys, 0, h - 1)
    xs = np.clip(xs, 0, w - 1)
    y0 = np.floor(ys).astype(np.int64)
    x0 = np.floor(xs).astype(np.int64)
    y1 = np.minimum(y0 + 1, h - 1)
    x1 = np.minimum(x0 + 1, w - 1)
    wy = (ys - y0)[:, None]
    wx = (xs - x0)[None, :]
    a = coarse[..., y0[:, None], x0[None, :]]
    b = coarse[..., y0[:, None], x1[None, :]]
    c = coarse[..., y1[:, None], x0[None, :]]
    d = coarse[..., y1[:, None], x1[None, :]]
    return (a * (1 - wx) + b * wx) * (1 - wy) + (c * (1 - wx) + d * wx) * wy


def make_panoptic_inputs(
    batch_size: int,
    n_classes: int = 40,
    height: int = 480,
    width: int = 640,
    n_centers: int = 24,
    seed: int = 0,
    quantize_offsets: bool = True,
    sigma: float = 8.0,
    offset_noise_px: float = 2.0,
    with_orientation: bool = False,
) -> Dict[str, np.ndarray]:
    rng = np.random.default_rng(seed)
    B, Cn, H, W = batch_size, n_classes, height, width
    gh, gw = max(H // 32, 2), max(W // 32, 2)

    logits = np.empty((B, Cn, H, W), np.float32)
    center = np.empty((B, 1, H, W), np.float32)
    offset = np.empty((B, 2, H, W), np.float32)
    planted = np.empty((B, n_centers, 2), np.int32)
    orientation = np.empty((B, 2, H, W), np.float32) if with_orientation else None

    yy = np.arange(H, dtype=np.float64)[:, None]
    xx = np.arange(W, dtype=np.float64)[None, :]
    border = int(min(8, H // 4, W // 4))

    for b in range(B):
        coarse = rng.standard_normal((Cn, gh, gw))
        logits[b] = (4.0 * _bilinear_up(coarse, H, W)).astype(np.float32)

        cy = rng.integers(border, H - border, size=n_centers)
        cx = rng.integers(border, W - border, size=n_centers)
        planted[b, :, 0] = cy
        planted[b, :, 1] = cx

        heat = np.zeros((H, W), np.float64)
        best_d2 = np.full((H, W), np.inf)
        near_y = np.zeros((H, W), np.float64)
        near_x = np.zeros((H, W), np.float64)
        for k in range(n_centers):
            dy = cy[k] - yy
            dx = cx[k] - xx
            d2 = dy * dy + dx * dx
            heat = np.maximum(heat, np.exp(-d2 / (2.0 * sigma * sigma)))
            closer = d2 < best_d2
            best_d2 = np.where(closer, d2, best_d2)
            near_y = np.where(closer, dy, near_y)
            near_x = np.where(closer, dx, near_x)
        center[b, 0] = heat.astype(np.float32)

        oy = near_y + offset_noise_px * rng.standard_normal((H, W))
        ox = near_x + offset_noise_px * rng.standard_normal((H, W))
        if quantize_offsets:
            oy = np.round(oy * 2.0) / 2.0
            ox = np.round(ox * 2.0) / 2.0
        offset[b, 0] = (oy / H).astype(np.float32)
        offset[b, 1] = (ox / W).astype(np.float32)

        if with_orientation:
            # smooth angle field -> unit biternion (cos, sin) via rational
            # parametrisation (no trig: keeps generation platform-stable)
            t = _bilinear_up(rng.standard_normal((1, gh, gw)), H, W)[0] * 2.0
            den = 1.0 + t * t
            orientation[b, 0] = ((1.0 - t * t) / den).astype(np.float32)
            orientation[b, 1] = ((2.0 * t) / den).astype(np.float32)

    is_thing = tuple(bool(c >= Cn // 2) for c in range(Cn))
    out = {
        'semantic_logits': logits,
        'instance_center': center,
        'instance_offset': offset,
        'planted_centers': planted,
        'semantic_classes_is_thing': np.array(is_thing, dtype=bool),
    }
    if with_orientation:
        out['instance_orientation'] = orientation
    return out


def make_metric_inputs(
    pred_panoptic: np.ndarray,
    n_classes_with_void: int,
    seed: int = 0,
    shift_px: int = 3,
) -> Dict[str, np.ndarray]:
    """GT for the metric accumulators: target_pan = roll(pred_pan, shift_px)
    with a void band, target_sem uniform in [0, C]."""
    rng = np.random.default_rng(seed + 1000)
    target_pan = np.roll(pred_panoptic, shift=(shift_px, shift_px), axis=(-2, -1)).copy()
    target_pan[..., :shift_px, :] = 0          # void band
    target_sem = rng.integers(0, n_classes_with_void, size=pred_panoptic.shape,
                              dtype=np.int64).astype(np.uint8)
    return {'panoptic_target': target_pan.astype(np.int64),
            'semantic_target': target_sem}


def make_loss_inputs(
    batch_size: int,
    n_classes: int = 40,
    height: int = 480,
    width: int = 640,
    seed: int = 0,
    embedding_dim: int = 0,
    n_lut: int = 64,
) -> Dict[str, np.ndarray]:
    rng = np.random.default_rng(seed + 2000)
    B, Cn, H, W = batch_size, n_classes, height, width
    base = make_panoptic_inputs(B, Cn, H, W, seed=seed, with_orientation=True)
    out = {
        'semantic_logits': base['semantic_logits'],
        'semantic_target': rng.integers(0, Cn + 1, size=(B, H, W)).astype(np.uint8),
        'class_weights': (rng.random(Cn) + 0.5).astype(np.float32),
        # predictions: noisy versions of the targets
        'center_target': base['instance_center'][:, 0].copy(),
        'center_pred': np.clip(base['instance_center'][:, 0]
                               + 0.1 * rng.standard_normal((B, H, W)), 0, 1).astype(np.float32),
        'center_mask': rng.random((B, H, W)) < 0.7,
        'offset_target': base['instance_offset'],
        'offset_pred': (base['instance_offset']
                        + 0.01 * rng.standard_normal((B, 2, H, W))).astype(np.float32),
        'offset_mask': rng.random((B, H, W)) < 0.5,
        'orientation_target': base['instance_orientation'],
        'orientation_mask': rng.random((B, H, W)) < 0.3,
    }
    # unit-length noisy orientation prediction (normalised with sqrt only)
    op = base['instance_orientation'].astype(np.float64) + 0.3 * rng.standard_normal((B, 2, H, W))
    op = op / (np.sqrt((op * op).sum(axis=1, keepdims=True)) + 1e-7)
    out['orientation_pred'] = op.astype(np.float32)
    if embedding_dim:
        D = embedding_dim
        lut = rng.standard_normal((B, n_lut, D))
        lut = lut / np.sqrt((lut * lut).sum(axis=-1, keepdims=True))
        out['embedding_lut'] = lut.astype(np.float32)
        out['embedding_indices'] = rng.integers(0, n_lut + 1, size=(B, H, W)).astype(np.int32)
        out['embedding_pred'] = rng.standard_normal((B, D, H, W)).astype(np.float32)
    return out


def round_to_bf16(a: np.ndarray) -> np.ndarray:
    """float32 array rounded to the nearest bfloat16 (ties to even), returned as float32 —
    what a bf16 network output holds; integer arithmetic only, platform-stable"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(a.shape)


def make_embedding_inputs(batch_size: int, embedding_dim: int, height: int, width: int,
                          n_lut: int, seed: int = 0, block: int = 4, bf16: bool = False
                          ) -> Dict[str, np.ndarray]:
    """Dense visual-embedding loss inputs (SURVEY §8d, configs[4]): prediction [B,D,H,W],
    per-image LUT [B,L,D] of unit rows, index map [B,H,W] int32 in [0, L] (0 = no target) made
    of `block` x `block` segments with ~15 % of the pixels re-drawn individually, so that lanes
    of a wave see both shared and distinct LUT rows.  `bf16`: the prediction holds
    bf16-representable values (as float32)."""
    rng = np.random.default_rng(seed + 4000)
    B, D, H, W, L = batch_size, embedding_dim, height, width, n_lut
    lut = rng.standard_normal((B, L, D))
    lut = lut / np.sqrt((lut * lut).sum(axis=-1, keepdims=True))
    coarse = rng.integers(0, L + 1, size=(B, (H + block - 1) // block, (W + block - 1) // block))
    idx = np.kron(coarse, np.ones((block, block), np.int64))[:, :H, :W]
    redraw = rng.random((B, H, W)) < 0.15
    idx = np.where(redraw, rng.integers(0, L + 1, size=(B, H, W)), idx)
    # prediction: the target row plus noise for most pixels (cosine ~0.5), pure noise elsewhere
    tgt = np.take_along_axis(lut, np.clip(idx - 1, 0, L - 1).reshape(B, -1, 1), axis=1)
    tgt = tgt.reshape(B, H, W, D).transpose(0, 3, 1, 2)
    pred = (tgt * (rng.random((B, 1, H, W)) < 0.8)
            + rng.standard_normal((B, D, H, W)) / np.sqrt(D)) * 3.0
    pred = pred.astype(np.float32)
    if bf16:
        pred = round_to_bf16(pred)
    return {'embedding_pred': pred, 'embedding_lut': lut.astype(np.float32),
            'embedding_indices': idx.astype(np.int32)}


def make_training_case(batch_size=2, n_classes=9, height=64, width=96, seed=0,
                       embedding_dim=16, n_lut=9, scales=(2, 4)):
    """One training batch for the task helpers (numpy): main output + side outputs at `scales`
    (every s-th pixel of the main prediction, scaled by 0.9) and the targets of the matching
    resolutions under the '_down_<s>' batch keys.  -> (batch, preds); per-image LUTs have
    different row counts (not stackable, like the reference's batches)."""
    d = make_loss_inputs(batch_size, n_classes, height, width, seed=seed,
                         embedding_dim=embedding_dim, n_lut=n_lut)
    rng = np.random.default_rng(seed + 3000)
    rows = [int(r) for r in rng.integers(max(n_lut // 2, 1), n_lut + 1, size=batch_size)]
    idx = d['embedding_indices'].copy()
    for b, r in enumerate(rows):
        idx[b][idx[b] > r] = 0                           # indices beyond the image's rows: no target
    batch = {
        'semantic': d['semantic_target'], 'instance_center': d['center_target'],
        'instance_center_mask': d['center_mask'], 'instance_offset': d['offset_target'],
        'instance_foreground': d['offset_mask'], 'orientation': d['orientation_target'],
        'orientation_foreground': d['orientation_mask'],
        'dense_visual_embedding_indices': idx,
    }

    def down(a, s):
        return np.ascontiguousarray(a[..., ::s, ::s])
    for s in scales:
        batch[f'_down_{s}'] = {k: down(v, s) for k, v in batch.items() if isinstance(v, np.ndarray)}
    luts = [np.ascontiguousarray(d['embedding_lut'][b, :r]) for b, r in enumerate(rows)]
    batch['dense_visual_embedding_lut'] = luts
    for s in scales:
        batch[f'_down_{s}']['dense_visual_embedding_lut'] = luts
    main = (d['center_pred'][:, None], d['offset_pred'], d['orientation_pred'])
    f32 = np.float32
    preds = {
        'semantic_output': d['semantic_logits'],
        'semantic_side_outputs': tuple((down(d['semantic_logits'], s) * f32(0.9)) for s in scales),
        'instance_output': main,
        'instance_side_outputs': tuple(tuple(down(x, s) * f32(0.9) for x in main) for s in scales),
        'dense_visual_embedding_output': d['embedding_pred'],
        'dense_visual_embedding_side_outputs': tuple(down(d['embedding_pred'], s) * f32(0.9)
                                                     for s in scales),
    }
    return batch, preds, d['class_weights']


def make_predictions_from_targets(semantic, center, offset, orientation, n_classes, seed=0):
    """Network-like outputs that mostly agree with the ground truth (so that validation metrics
    are neither 0 nor 1): logits = 3 * onehot(label - 1) + N(0, 1) (void pixels: pure noise),
    center / offset / orientation = target + noise.  numpy only, float32 results."""
    rng = np.random.default_rng(seed + 5000)
    B, H, W = semantic.shape
    logits = rng.standard_normal((B, n_classes, H, W))
    lab = semantic.astype(np.int64) - 1
    onehot = (np.arange(n_classes)[None, :, None, None] == lab[:, None]).astype(np.float64)
    logits = logits + 3.0 * onehot
    c = np.clip(center + 0.03 * rng.standard_normal(center.shape), 0.0, 1.0)
    o = offset + 0.004 * rng.standard_normal(offset.shape)
    q = orientation.astype(np.float64) + 0.25 * rng.standard_normal(orientation.shape)
    q = q / (np.sqrt((q * q).sum(axis=1, keepdims=True)) + 1e-7)
    return (logits.astype(np.float32), c.astype(np.float32)[:, None], o.astype(np.float32),
            q.astype(np.float32))


def make_label_maps(batch_size, n_classes=41, height=480, width=640, n_instances=30, seed=0,
                    max_id=65535, mixed_fraction=0.3, max_radius=None):
    """Ground-truth style label maps for the target generators.

    semantic u8 [B,H,W] in [0, n_classes) (0 = void): blocky regions; instance int32 [B,H,W]:
    `n_instances` random ellipses with sparse ids in [1, max_id] (uint16 range, as the datasets
    store them), later ones painted over earlier ones.  A `mixed_fraction` of the instances keeps
    the underlying (mixed) semantic labels, the others get one thing class painted in.
    is_thing = class index >= n_classes // 2 (void and the lower half are stuff)."""
    rng = np.random.default_rng(seed)
    is_thing = np.arange(n_classes) >= max(1, n_classes // 2)
    thing_ids = np.where(is_thing)[0]
    sem = np.empty((batch_size, height, width), np.uint8)
    ins = np.zeros((batch_size, height, width), np.int32)
    yy, xx = np.mgrid[0:height, 0:width]
    for b in range(batch_size):
        coarse = rng.integers(0, n_classes, ((height + 31) // 32, (width + 31) // 32))
        sem[b] = np.kron(coarse, np.ones((32, 32), np.int64))[:height, :width]
        ids = rng.choice(np.arange(1, max_id + 1), size=n_instances, replace=False)
        for k, iid in enumerate(ids):
            cy, cx = rng.integers(0, height), rng.integers(0, width)
            ry = rng.integers(3, max_radius or max(4, height // 5))
            rx = rng.integers(3, max_radius or max(4, width // 5))
            m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
            ins[b][m] = iid
            if rng.random() >= mixed_fraction:
                sem[b][m] = rng.choice(thing_ids)
    return {'semantic': sem, 'instance': ins, 'semantic_classes_is_thing': is_thing}


WORD_EDGES = (64, 128, 192)           # class words of the thing LUT as ballot masks (C > 64)


def wide_edge_classes(n_classes: int) -> np.ndarray:
    """the classes next to the 64-class word edges (63/64, 127/128, 191/192), the last one and 0"""
    near = {c for e in WORD_EDGES + (256,) for c in (e - 2, e - 1, e, e + 1)}
    return np.array(sorted(c for c in near | {0, n_classes - 1} if 0 <= c < n_classes))


def make_wide_class_inputs(batch_size: int, n_classes: int, height: int, width: int,
                           n_centers, seed: int, levels: int = 4, p_edge: float = 0.5,
                           p_tie: float = 0.3, p_thing: float = 0.5, p_far: float = 0.2
                           ) -> Dict[str, np.ndarray]:
    """Panoptic inputs for 49..256 classes, aimed at the class-word edges.

    Logits are small integer levels (int8; exact in bf16 / f16, and equal logits give equal
    probabilities, so the first index wins under any softmax).  The winning class of a pixel is
    drawn with a bias toward the word edges; with probability `p_tie` it is tied with the class
    on the other side of an edge (63/64, 127/128, 191/192).  The two classes of an edge pair are
    one thing and one stuff class.  The heat map holds `n_centers` (an int or one per image)
    isolated peaks of distinct heights on a 2-pixel lattice inside the border: a 3x3 NMS keeps
    every one and the top-k has no tie.  Every offset points exactly at the pixel's nearest
    peak, or with probability `p_far` at a random one."""
    rng = np.random.default_rng(seed)
    B, C, H, W = batch_size, n_classes, height, width
    logits = rng.integers(0, levels, (B, C, H, W)).astype(np.int8)
    edge = wide_edge_classes(C)
    top = np.where(rng.random((B, H, W)) < p_edge, rng.choice(edge, (B, H, W)),
                   rng.integers(0, C, (B, H, W)))
    edges = [e for e in WORD_EDGES if e < C]
    tie = (rng.random((B, H, W)) < p_tie) if edges else np.zeros((B, H, W), bool)
    if edges:
        top = np.where(tie, rng.choice(edges, (B, H, W)) - 1, top)
    np.put_along_axis(logits, top[:, None], np.int8(levels + 1), axis=1)
    partner = np.where(tie, top + 1, top)
    np.put_along_axis(logits, partner[:, None], np.int8(levels + 1), axis=1)

    is_thing = rng.random(C) < p_thing
    for e in edges:
        is_thing[e - 1] = rng.random() < 0.5
        is_thing[e] = not is_thing[e - 1]
    if C == 256:
        is_thing[255] = True

    heat = np.zeros((B, 1, H, W), np.float32)
    offset = np.zeros((B, 2, H, W), np.float32)
    # (the reference's NMS pads the pooled map with zeros: a peak on the border is never kept)
    sites = np.stack(np.meshgrid(np.arange(1, H - 1, 2), np.arange(1, W - 1, 2), indexing='ij'), -1)
    sites = sites.reshape(-1, 2)
    yy = np.arange(H)[:, None]
    xx = np.arange(W)[None, :]
    per_image = np.broadcast_to(np.asarray(n_centers), (B,))
    for b in range(B):
        n = int(min(per_image[b], len(sites)))
        if n == 0:
            continue
        cyx = sites[rng.choice(len(sites), n, replace=False)]
        heights = 0.15 + 0.85 * (rng.permutation(n) + 1) / n
        heat[b, 0, cyx[:, 0], cyx[:, 1]] = heights.astype(np.float32)
        d2 = (cyx[:, 0, None, None] - yy) ** 2 + (cyx[:, 1, None, None] - xx) ** 2
        k = d2.argmin(0)
        k = np.where(rng.random((H, W)) < p_far, rng.integers(0, n, (H, W)), k)
        offset[b, 0] = ((cyx[k, 0] - yy) / H).astype(np.float32)
        offset[b, 1] = ((cyx[k, 1] - xx) / W).astype(np.float32)
    return {'semantic_logits': logits, 'instance_center': heat, 'instance_offset': offset,
            'semantic_classes_is_thing': is_thing}


def input_digest(*arrays: np.ndarray) -> str:
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode())
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def make_panoptic_inputs_torch(batch_size, n_classes=40, height=480, width=640,
                               n_centers=24, seed=0, device='cuda', sigma=8.0,
                               offset_noise_px=2.0, quantize_offsets=True,
                               logits_dtype=None, chunk=8):
    """Same recipe as `make_panoptic_inputs`, generated on `device` with torch
    (for bench.py / full-size property tests: fast, not bit-reproducible
    across devices — parity there is checked against the oracle on the very
    tensors that were generated)."""
    import torch
    B, Cn, H, W = batch_size, n_classes, height, width
    g = torch.Generator(device=device).manual_seed(seed)
    gh, gw = max(H // 32, 2), max(W // 32, 2)
    coarse = torch.randn((B, Cn, gh, gw), device=device, generator=g)
    logits = 4.0 * torch.nn.functional.interpolate(coarse, size=(H, W), mode='bilinear',
                                                   align_corners=False)
    if logits_dtype is not None:
        logits = logits.to(logits_dtype)
    border = int(min(8, H // 4, W // 4))
    cy = torch.randint(border, H - border, (B, n_centers), device=device, generator=g)
    cx = torch.randint(border, W - border, (B, n_centers), device=device, generator=g)
    yy = torch.arange(H, device=device, dtype=torch.float32).view(1, 1, H, 1)
    xx = torch.arange(W, device=device, dtype=torch.float32).view(1, 1, 1, W)
    center = torch.empty((B, 1, H, W), device=device)
    offset = torch.empty((B, 2, H, W), device=device)
    for b0 in range(0, B, chunk):
        b1 = min(b0 + chunk, B)
        dy = cy[b0:b1].float().view(-1, n_centers, 1, 1) - yy
        dx = cx[b0:b1].float().view(-1, n_centers, 1, 1) - xx
        d2 = dy * dy + dx * dx
        center[b0:b1, 0] = torch.exp(-d2 / (2.0 * sigma * sigma)).amax(dim=1)
        near = d2.argmin(dim=1, keepdim=True)
        oy = torch.gather(dy.expand_as(d2), 1, near)[:, 0]
        ox = torch.gather(dx.expand_as(d2), 1, near)[:, 0]
        oy = oy + offset_noise_px * torch.randn(oy.shape, device=device, generator=g)
        ox = ox + offset_noise_px * torch.randn(ox.shape, device=device, generator=g)
        if quantize_offsets:
            oy = torch.round(oy * 2.0) / 2.0
            ox = torch.round(ox * 2.0) / 2.0
        offset[b0:b1, 0] = oy / H
        offset[b0:b1, 1] = ox / W
    is_thing = torch.arange(Cn, device=device) >= Cn // 2
    return {'semantic_logits': logits.contiguous(), 'instance_center': center,
            'instance_offset': offset, 'semantic_classes_is_thing': is_thing}


# ---- dense-visual-embedding postprocessing cases (tests/golden/dve_postprocess.npz) ----------
# name -> (B, D, H, W, Ca, Cb or 0, crop (y0, y1, x0, x1), full-resolution shape)
DVE_POST_RECIPES = {
    'clean': (2, 512, 120, 160, 40, 40, (4, 116, 0, 160), (150, 200)),
    'noise': (2, 512, 120, 160, 40, 0, (0, 120, 0, 160), (120, 160)),
    'wide': (2, 768, 96, 128, 150, 0, (0, 96, 0, 128), (96, 200)),
    'odd': (1, 66, 45, 61, 37, 300, (2, 43, 3, 60), (41, 57)),
}


def make_dve_post_inputs(recipe: str, seed: int) -> Dict[str, np.ndarray]:
    """Embedding map, class embeddings and a full-resolution semantic target of one recipe.  Only
    generator draws and elementwise float32 arithmetic (no reductions), so the bytes are the same
    on every host.  'clean': 8x8 blocks of one class each, pixel = (class row + 0.08 noise) * a
    per-pixel scale in 0.5-4.5; the others: pure N(0, 1); 'odd' has one all-zero pixel and one inf."""
    B, D, H, W, Ca, Cb, crop, full = DVE_POST_RECIPES[recipe]
    rng = np.random.default_rng(seed)
    f32 = np.float32
    w_a = rng.standard_normal((Ca, D), dtype=f32) * f32(1.0 / np.sqrt(D))
    w_b = None
    if Cb:
        if recipe == 'clean':       # "visual mean" rows: the text rows, perturbed
            w_b = w_a + rng.standard_normal((Cb, D), dtype=f32) * f32(0.3 / np.sqrt(D))
        else:
            w_b = rng.standard_normal((Cb, D), dtype=f32) * f32(1.0 / np.sqrt(D))
    n_classes = Ca
    if recipe == 'clean':
        cls = rng.integers(0, Ca, (B, (H + 7) // 8, (W + 7) // 8))
        cls = np.repeat(np.repeat(cls, 8, axis=1), 8, axis=2)[:, :H, :W]
        noise = rng.standard_normal((B, D, H, W), dtype=f32)
        scale = f32(0.5) + f32(4.0) * rng.random((B, 1, H, W), dtype=f32)
        emb = (np.moveaxis(w_a[cls], -1, 1) + f32(0.08) * noise) * scale
        # target: the block's class (+1; 0 = void on a sparse grid) seen from the full resolution
        yy = crop[0] + (np.arange(full[0]) * (crop[1] - crop[0])) // full[0]
        xx = crop[2] + (np.arange(full[1]) * (crop[3] - crop[2])) // full[1]
        target = (cls[:, yy][:, :, xx] + 1).astype(np.uint8)
        target[:, ::7, ::5] = 0
    else:
        emb = rng.standard_normal((B, D, H, W), dtype=f32)
        target = rng.integers(0, n_classes + 1, (B,) + tuple(full)).astype(np.uint8)
    if recipe == 'odd':
        emb[0, :, 7, 11] = 0.0
        emb[0, 5, 20, 33] = np.inf
    out = {'emb': np.ascontiguousarray(emb, dtype=f32), 'weight_a': w_a, 'semantic_fullres': target}
    if w_b is not None:
        out['weight_b'] = np.ascontiguousarray(w_b, dtype=f32)
    return out


# ---- surface-normal task cases (tests/golden/normal_task.npz) ---------------------------------
# name -> (B, network resolution (H, W), crop (y0, y1, x0, x1), full resolution, supervision scales)
NORMAL_RECIPES = {
    'same': (2, (8, 12), (0, 8, 0, 12), (8, 12), (1, 2, 4)),
    'up': (2, (6, 8), (1, 6, 0, 7), (9, 13), (1, 2)),
    'holes': (3, (8, 8), (0, 8, 0, 8), (16, 16), (1,)),
    'wide': (1, (4, 260), (0, 4, 2, 258), (4, 512), (1,)),
}


def _normal_target(rng, B: int, H: int, W: int, holes: bool) -> np.ndarray:
    """unit normals [B,3,H,W] with exact zeros in 4x4-block blobs of about 30 % of the image; the
    last image keeps its first block valid.  `holes`: image 0 entirely invalid, some invalid
    pixels carry -0.0, some valid ones have one or two zero channels."""
    f32 = np.float32
    v = rng.standard_normal((B, 3, H, W), dtype=f32)
    norm = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    t = (v / np.maximum(norm, f32(1e-6))[:, None]).astype(f32)
    blob = rng.random((B, (H + 3) // 4, (W + 3) // 4)) < 0.3
    blob[-1, 0, 0] = False
    invalid = np.repeat(np.repeat(blob, 4, axis=1), 4, axis=2)[:, :H, :W].copy()
    if holes:
        invalid[0] = True
    t = np.where(invalid[:, None], f32(0.0), t).astype(f32)
    if holes:
        b = B - 1
        t[0, 1, ::2, ::3] = f32(-0.0)               # invalid pixels, some channels -0.0
        t[0, :, 1, 1] = f32(-0.0)
        t[b, :, 0, 0] = (0.0, 0.0, 1.0)             # two zero channels: valid
        t[b, :, 0, 1] = (0.0, 0.6, 0.8)             # one zero channel: valid
        t[b, :, 0, 2] = (-0.0, 0.0, -1.0)
    return np.ascontiguousarray(t)


def make_normal_inputs(recipe: str, seed: int) -> Dict[str, np.ndarray]:
    """Predictions and targets of every supervision scale ('pred_s<k>', 'target_s<k>'), the
    full-resolution target and an explicit metric mask of one recipe.  Generator draws and
    elementwise float32 arithmetic only, so the bytes are the same on every host.  Predictions are
    finite everywhere: target + 0.3 N(0, 1)."""
    B, (Hn, Wn), crop, (H, W), scales = NORMAL_RECIPES[recipe]
    rng = np.random.default_rng(seed)
    f32 = np.float32
    holes = recipe == 'holes'
    out = {}
    for s in scales:
        h, w = Hn // s, Wn // s
        t = _normal_target(rng, B, h, w, holes)
        out[f'target_s{s}'] = t
        out[f'pred_s{s}'] = (t + f32(0.3) * rng.standard_normal((B, 3, h, w), dtype=f32)).astype(f32)
    out['target_fullres'] = _normal_target(rng, B, H, W, holes)
    out['metric_mask'] = rng.random((B, H, W)) < 0.6
    return out


# ---- orientation targets (data/preprocessing/orientation.py) ------------------------------------
# recipe -> (B, n_classes, H, W, random instances per image)
ORIENTATION_RECIPES = {
    'ragged': (3, 5, 37, 53, 8),          # W % 4 != 0: the per-pixel path
    'wire': (3, 41, 96, 128, 12),         # the on-wire layout; one instance over half of image 0
}
# ids of the crafted instances of image 0 (2 x 4 pixel blocks unless noted)
ORI_VOID, ORI_UNFLAGGED, ORI_TIE_FLAGGED, ORI_TIE_UNFLAGGED, ORI_NO_ANGLE, ORI_NOT_IN_MAP, ORI_BIG = \
    60001, 60002, 60003, 60004, 60005, 60006, 60007


def make_orientation_inputs(recipe: str, seed: int) -> Dict:
    """Label maps of `make_label_maps` plus per-image {instance id: angle in rad} dicts for the
    orientation target generator.  Odd classes are the ones whose orientation is estimated (void
    is not).  Image 0 holds crafted instances: majority class void; majority class not flagged;
    an exact vote tie between classes 1 (flagged) and 2 (not), which class 1 wins; a tie between
    classes 2 and 3, which class 2 wins; an instance without an angle; an angle for an id that is
    not in the map; and (maps of 96 rows or more) one instance over the upper 60 rows, whose vote
    is spread over several workgroups.  Image 1 has angles for about two thirds of its random
    instances, image 2 an empty dict.  The angles include 0, pi, a negative one and one above 2 pi."""
    B, C, H, W, n_inst = ORIENTATION_RECIPES[recipe]
    maps = make_label_maps(B, C, H, W, n_instances=n_inst, seed=seed)
    sem, ins = maps['semantic'], maps['instance']
    rng = np.random.default_rng(seed + 7919)
    assert not np.isin(ins, np.arange(ORI_VOID, ORI_BIG + 1)).any()
    if H >= 96:
        ins[0, :60, :] = ORI_BIG

    def block(y, x, iid, left, right):
        ins[0, y:y + 2, x:x + 4] = iid
        sem[0, y:y + 2, x:x + 2] = left
        sem[0, y:y + 2, x + 2:x + 4] = right

    block(1, 1, ORI_VOID, 0, 0)
    block(1, 8, ORI_UNFLAGGED, 2, 2)
    block(5, 1, ORI_TIE_FLAGGED, 2, 1)
    block(5, 8, ORI_TIE_UNFLAGGED, 3, 2)
    block(9, 1, ORI_NO_ANGLE, 1, 1)
    orientations = []
    for b in range(B):
        d = {}
        if b < 2:
            for iid in np.unique(ins[b]):
                if iid != 0 and iid < ORI_VOID and rng.random() < 0.67:
                    d[int(iid)] = float(rng.uniform(-np.pi, 3.0 * np.pi))
        if b == 0:
            d.update({ORI_VOID: 0.0, ORI_UNFLAGGED: float(np.pi), ORI_TIE_FLAGGED: -1.25,
                      ORI_TIE_UNFLAGGED: 7.0, ORI_NOT_IN_MAP: 1.0})
            if H >= 96:
                d[ORI_BIG] = 2.5
        if b == 1:
            d[int(ins[b].max()) + 1] = 0.5                  # an angle without an instance
        orientations.append(d)
    return {'semantic': sem, 'instance': ins, 'estimate': np.arange(C) % 2 == 1,
            'orientations': orientations}


# ---- side-output targets (data/preprocessing/multiscale_supervision.py) -------------------------
# recipe -> (B, n_classes, H, W, random instances per image, downscales, sigma, sigma per downscale)
MULTISCALE_RECIPES = {
    'A': (2, 9, 58, 116, 16, (4, 8), 4, {4: 2, 8: 1}),         # 116 -> 14 and 58 -> 14: floor(x / scale) is not x * src // dst
    'B': (3, 9, 50, 70, 14, (8, 16, 32), 4, {8: 2, 16: 1, 32: 1}),      # the last scale is 1 x 2
    'C': (1, 9, 48, 64, 12, (2, 4), 4, {2: 3, 4: 2}),          # divisible: equals [::d, ::d]
}
MULTISCALE_SPATIAL_KEYS = ('semantic', 'instance', 'depth', 'normal', 'valid', 'segment_ids')
MULTISCALE_KEYS = MULTISCALE_SPATIAL_KEYS + ('orientations', 'scene')


def make_multiscale_inputs(recipe: str, seed: int) -> Dict:
    """A collated batch for the side-output target chain, one entry per element size and layout:
    `semantic` u8 and `instance` i32 [B,H,W] of `make_label_maps`, `depth` i16 [B,H,W] over the
    whole int16 range, `normal` f32 [B,3,H,W] with NaNs of several payloads, -0.0, +-inf and
    denormals strewn in, `valid` bool [B,H,W], `segment_ids` u32 [B,H,W] above 2^16 (the
    reference's uint32 path; the device batch holds it as i64), `orientations` one dict {instance
    id: angle} per image and `scene` i64 [B] (not spatial: copied).  Odd classes are the ones
    whose orientation is estimated."""
    B, C, H, W, n_inst, _, _, _ = MULTISCALE_RECIPES[recipe]
    maps = make_label_maps(B, C, H, W, n_instances=n_inst, seed=seed)
    sem, ins = maps['semantic'], maps['instance']
    rng = np.random.default_rng(seed + 104729)
    depth = rng.integers(-32768, 32768, (B, H, W)).astype(np.int16)
    normal = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    bits = normal.view(np.uint32)
    special = np.array([0x7fc00000, 0xffc00001, 0x7f800123, 0x80000000, 0x00000000, 0x7f800000,
                        0xff800000, 0x00000001, 0x807fffff], np.uint32)
    strewn = rng.random(normal.shape) < 0.2
    bits[strewn] = rng.choice(special, size=int(strewn.sum()))
    valid = rng.random((B, H, W)) < 0.5
    segment_ids = (sem.astype(np.uint32) << 16) + ins.astype(np.uint32) + np.uint32(0x80000000) * \
        (rng.random((B, H, W)) < 0.25)
    orientations = []
    for b in range(B):
        orientations.append({int(i): float(rng.uniform(-np.pi, 3.0 * np.pi))
                             for i in np.unique(ins[b]) if i != 0 and rng.random() < 0.8})
    return {'semantic': sem, 'instance': ins, 'depth': depth, 'normal': normal, 'valid': valid,
            'segment_ids': segment_ids, 'orientations': orientations,
            'scene': rng.integers(0, 5, (B,)).astype(np.int64),
            'semantic_classes_is_thing': maps['semantic_classes_is_thing'],
            'estimate': np.arange(C) % 2 == 1}


def multiscale_input_digest(inp: Dict) -> str:
    """SHA-256 over everything `make_multiscale_inputs` returns (fixture and tests compare it)"""
    angles = json.dumps([[[int(k), float(v)] for k, v in d.items()] for d in inp['orientations']])
    return input_digest(*(inp[k] for k in MULTISCALE_SPATIAL_KEYS), inp['scene'],
                        inp['semantic_classes_is_thing'], inp['estimate'],
                        np.frombuffer(angles.encode(), dtype=np.uint8))


# ---- batch augmentation (data/preprocessing/{crop,flip,normalize,torch}.py) ----------------------
# recipe -> (B, n_classes, H, W, random instances per image, crop h, crop w, flip p, depth dtype,
#            depth mean, depth std, raw_depth, inputs of)
AUGMENT_RECIPES = {
    'A': (4, 9, 41, 67, 10, 37, 50, 0.5, 'uint16', 2841.94941272766, 1417.2594281672277, False, 'A'),  # w % 4 == 2
    'B': (2, 9, 33, 64, 8, 33, 64, 1.0, 'uint16', 2841.94941272766, 1417.2594281672277, True, 'B'),    # crop == image, all flipped
    'C': (3, 9, 20, 23, 6, 5, 7, 0.0, 'float32', 1.5, 0.75, True, 'C'),       # float32 depth with invalid values kept
    'C1': (3, 9, 20, 23, 6, 1, 1, 0.0, 'float32', 1.5, 0.75, True, 'C'),      # the same inputs, a 1 x 1 crop
    'D': (2, 9, 40, 301, 12, 33, 263, 0.5, 'uint16', 2841.94941272766, 1417.2594281672277, False, 'D'),  # long odd rows
    'E': (4, 9, 21, 76, 8, 16, 68, 0.5, 'uint16', 2841.94941272766, 1417.2594281672277, True, 'E'),    # w % 4 == 0, offsets of any parity
}
AUGMENT_SPATIAL_KEYS = ('rgb', 'depth', 'semantic', 'instance', 'normal', 'valid', 'segment_ids')


def make_augment_inputs(recipe: str, seed: int) -> Dict:
    """A collated RAW batch as the dataset yields it, channels last: `rgb` u8 [B,H,W,3] covering 0
    and 255, `depth` [B,H,W] — u16 covering 0 and 65535, or f32 with 0.0, -0.0, the recipe's
    mean (normalises to 0) and NaN strewn in —, `semantic` u8, `instance` i32 and `valid` bool
    [B,H,W], `normal` f32 [B,H,W,3] with the NaN payloads, -0.0, infinities and denormals of
    `make_multiscale_inputs`, `segment_ids` u32 [B,H,W] above 2^16 (the device batch holds it as
    i64) and `orientations`, one dict {instance id: angle} per image."""
    B, C, H, W, n_inst, _, _, _, depth_dtype, depth_mean = AUGMENT_RECIPES[AUGMENT_RECIPES[recipe][12]][:10]
    return _make_raw_batch(B, C, H, W, n_inst, depth_dtype, depth_mean, seed)


def _make_raw_batch(B: int, C: int, H: int, W: int, n_inst: int, depth_dtype: str, depth_mean: float, seed: int) -> Dict:
    maps = make_label_maps(B, C, H, W, n_instances=n_inst, seed=seed, max_radius=max(4, min(H, W) // 3))
    sem, ins = maps['semantic'], maps['instance']
    rng = np.random.default_rng(seed + 15485863)
    rgb = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    rgb[rng.random(rgb.shape) < 0.05] = 0
    rgb[rng.random(rgb.shape) < 0.05] = 255
    if depth_dtype == 'uint16':
        depth = rng.integers(0, 65536, (B, H, W)).astype(np.uint16)
        depth[rng.random(depth.shape) < 0.1] = 0
        depth[rng.random(depth.shape) < 0.05] = 65535
    else:
        depth = (rng.random((B, H, W)) * 4.0).astype(np.float32)
        kind = rng.integers(0, 10, depth.shape)
        for k, bits in enumerate((0x00000000, 0x80000000, np.float32(depth_mean).view(np.uint32), 0x7fc00000)):
            depth.view(np.uint32)[kind == k] = bits
    normal = rng.standard_normal((B, H, W, 3)).astype(np.float32)
    bits = normal.view(np.uint32)
    special = np.array([0x7fc00000, 0xffc00001, 0x7f800123, 0x80000000, 0x00000000, 0x7f800000,
                        0xff800000, 0x00000001, 0x807fffff], np.uint32)
    strewn = rng.random(normal.shape) < 0.2
    bits[strewn] = rng.choice(special, size=int(strewn.sum()))
    valid = rng.random((B, H, W)) < 0.5
    segment_ids = (sem.astype(np.uint32) << 16) + ins.astype(np.uint32) + np.uint32(0x80000000) * \
        (rng.random((B, H, W)) < 0.25)
    orientations = [{int(i): float(rng.uniform(0.0, 2.0 * np.pi)) for i in np.unique(ins[b]) if i != 0}
                    for b in range(B)]
    return {'rgb': rgb, 'depth': depth, 'semantic': sem, 'instance': ins, 'normal': normal, 'valid': valid,
            'segment_ids': segment_ids, 'orientations': orientations,
            'semantic_classes_is_thing': maps['semantic_classes_is_thing']}


def augment_input_digest(inp: Dict) -> str:
    """SHA-256 over everything `make_augment_inputs` returns (fixture and tests compare it)"""
    angles = json.dumps([[[int(k), float(v)] for k, v in d.items()] for d in inp['orientations']])
    return input_digest(*(inp[k] for k in AUGMENT_SPATIAL_KEYS), inp['semantic_classes_is_thing'],
                        np.frombuffer(angles.encode(), dtype=np.uint8))


# ---- batch augmentation behind a resize (data/preprocessing/{resize,crop,flip,normalize,torch}.py) ----
# recipe -> B, n_classes, H, W, random instances per image, crop, flip p, depth (dtype, mean, std,
# raw_depth), then ONE of: scales (min, max) of RandomResize; sizes [(rh, rw)] per sample, applied
# with the reference's resize() in RandomResize's place; upscale (RandomCrop resizes the image that
# is smaller than the crop).  The keys are AUGMENT_SPATIAL_KEYS.
_U16_DEPTH = ('uint16', 2841.94941272766, 1417.2594281672277, False)
AUGMENT_RESIZE_RECIPES = {
    # w % 4 == 0: four pixels per lane; both flip values, both parities of x0, scales below and above 1
    'RA': dict(B=4, C=9, H=41, W=67, n_inst=10, crop=(21, 36), p=0.5, depth=_U16_DEPTH, scales=(0.6, 1.5)),
    # w % 4 == 2: one pixel per lane
    'RB': dict(B=3, C=9, H=41, W=67, n_inst=10, crop=(19, 38), p=0.5, depth=_U16_DEPTH, scales=(0.6, 1.5)),
    # an exact 2:1 downscale, no scale draw, no offset draws: rgb is the mean of 2 x 2 pixels
    'RC': dict(B=2, C=9, H=40, W=64, n_inst=8, crop=(20, 32), p=0.5, depth=_U16_DEPTH, scales=(0.5, 0.5)),
    # nearest maps that differ from x * src // dst on both sides (36 -> 44, 63 -> 77; 36 -> 28, 63 -> 49)
    'RD': dict(B=2, C=9, H=36, W=63, n_inst=8, crop=(24, 44), p=0.5, depth=_U16_DEPTH, sizes=((44, 77), (28, 49))),
    # smaller than the crop: upscaled to 35 x 40, x0 is not drawn; float32 depth with invalid values kept
    'RE': dict(B=2, C=9, H=20, W=23, n_inst=6, crop=(33, 40), p=0.5, depth=('float32', 1.5, 0.75, True), upscale=True),
    # rows longer than a wave of four-pixel lanes, several blocks per descriptor
    'RF': dict(B=2, C=9, H=12, W=301, n_inst=8, crop=(10, 300), p=0.5, depth=_U16_DEPTH, scales=(1.0, 1.4)),
}


def make_augment_resize_inputs(recipe: str, seed: int) -> Dict:
    """the raw batch of `make_augment_inputs` for a recipe of AUGMENT_RESIZE_RECIPES"""
    r = AUGMENT_RESIZE_RECIPES[recipe]
    return _make_raw_batch(r['B'], r['C'], r['H'], r['W'], r['n_inst'], r['depth'][0], r['depth'][1], seed)


# ----------------------------------------------------------------------------- scene task
# name: (n_classes, class weights, label smoothing, seed) of tests/golden/scene_task.npz
SCENE_CASES = {'plain': (10, False, 0.0, 70), 'weighted': (10, True, 0.0, 71),
               'smoothed': (45, False, 0.1, 72), 'weighted_smoothed': (45, True, 0.1, 73)}
SCENE_EPOCHS = 2
# the batches of every epoch: (rows, kind)
SCENE_BATCHES = ((8, 'plain'), (6, 'some_void'), (4, 'all_void'), (7, 'ties'))


def _scene_batch(rng, B: int, C: int, kind: str):
    logits = (rng.standard_normal((B, C)) * 3.0).astype(np.float32)
    labels = rng.integers(1, C + 1, size=(B,)).astype(np.int64)
    hit = rng.random(B) < 0.6                   # a head that is right more often than chance
    logits[hit, labels[hit] - 1] += np.float32(6.0)
    if kind == 'some_void':
        labels[rng.choice(B, size=B // 2, replace=False)] = 0
    elif kind == 'all_void':
        labels[:] = 0
    elif kind == 'ties':
        for r in range(0, B, 2):                # every other row: two or three equal largest logits
            cols = rng.choice(C, size=2 + r % 2, replace=False)
            logits[r, cols] = logits[r].max() + np.float32(0.5)
    return logits, labels


def make_scene_inputs(name: str) -> Dict[str, object]:
    """The inputs of one case of SCENE_CASES: 'weights' (float32 [C] or None) and 'batches', a
    list over the epochs of lists of (logits float32 [B, C], labels int64 [B], 0 = void) per
    SCENE_BATCHES.  Generator draws and elementwise float32 arithmetic only, so the bytes are the
    same on every host."""
    C, weighted, _, seed = SCENE_CASES[name]
    rng = np.random.default_rng(seed)
    weights = (rng.random(C) + 0.25).astype(np.float32) if weighted else None
    batches = [[_scene_batch(rng, B, C, kind) for B, kind in SCENE_BATCHES] for _ in range(SCENE_EPOCHS)]
    return {'weights': weights, 'batches': batches}


def scene_input_digest(inputs) -> str:
    arrays = [a for epoch in inputs['batches'] for pair in epoch for a in pair]
    if inputs['weights'] is not None:
        arrays.append(inputs['weights'])
    return input_digest(*arrays)


# ----------------------------------------------------------------------------- learned upsampling
# name: (mode, use_bias, trained, (B, C, h, w), seed) of tests/golden/upsampling.npz; `trained`:
# random weights (and bias), else the module's initial values
UPSAMPLING_CASES = {
    'rep_bias_trained': ('learned-3x3', True, True, (2, 3, 5, 6), 90),
    'rep_bias_initial': ('learned-3x3', True, False, (1, 4, 3, 7), 91),
    'rep_nobias_trained': ('learned-3x3', False, True, (2, 2, 9, 4), 92),
    'rep_nobias_initial': ('learned-3x3', False, False, (1, 3, 1, 5), 93),
    'zero_bias_trained': ('learned-3x3-zeropad', True, True, (2, 3, 5, 6), 94),
    'zero_bias_initial': ('learned-3x3-zeropad', True, False, (1, 4, 3, 7), 95),
    'zero_nobias_trained': ('learned-3x3-zeropad', False, True, (2, 2, 9, 4), 96),
    'zero_nobias_initial': ('learned-3x3-zeropad', False, False, (1, 3, 1, 5), 97),
}
# input of the output-shape record of all four mode names
UPSAMPLING_SHAPE_INPUT = (1, 2, 3, 5)


def make_upsampling_inputs(name: str) -> Dict[str, object]:
    """The inputs of one case of UPSAMPLING_CASES: 'x' float32 [B,C,h,w], 'gy' float32 [B,C,2h,2w]
    (the upstream gradient), 'weight' float32 [C,1,3,3] and 'bias' float32 [C] (None where the case
    keeps the module's initial values / has no bias).  Generator draws and float32 casts only."""
    _, use_bias, trained, (B, C, h, w), seed = UPSAMPLING_CASES[name]
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, C, h, w)).astype(np.float32)
    gy = rng.standard_normal((B, C, 2 * h, 2 * w)).astype(np.float32)
    weight = (rng.standard_normal((C, 1, 3, 3)) * 0.25).astype(np.float32) if trained else None
    bias = rng.standard_normal((C,)).astype(np.float32) if trained and use_bias else None
    return {'x': x, 'gy': gy, 'weight': weight, 'bias': bias}


def upsampling_input_digest(inputs) -> str:
    return input_digest(*(inputs[k] for k in ('x', 'gy', 'weight', 'bias') if inputs[k] is not None))
