"""Writes tests/golden/batch_augment_resize.npz: the reference's unmodified
`data/preprocessing/{resize,crop,flip,normalize,torch}.py`, loaded through `oracle.ref_loader`, run
per sample on CPU on the seeded raw batches of `testing.synthetic.AUGMENT_RESIZE_RECIPES`, under
`np.random.seed(seed)`, as the chain

  RandomResize -> RandomCrop -> RandomHorizontalFlip -> NormalizeRGB -> NormalizeDepth -> ToTorchTensors

the samples of a batch one after the other.  A recipe with `sizes` calls the reference's `resize()`
with the listed size in RandomResize's place; a recipe with `upscale` has no RandomResize and lets
RandomCrop resize the image that is smaller than its crop.

`cv2` IS NOT INSTALLED HERE.  The loader's `cv2` is an empty module; this tool sets
`INTER_NEAREST`, `INTER_LINEAR` and a `resize` on it, in its own process.  That `resize` is a
NUMPY STAND-IN, not OpenCV.  It resizes the WHOLE image, as cv2 would, by two rules written down
from OpenCV's source and NOT compared with a real `cv2` build:
  nearest   `ifx = 1 / (dst / src)` in double, source index `min(floor(x * ifx), src - 1)`
  linear    (8-bit images) per side `scale = 1 / (dst / src)` in double, `f = float32((d + 0.5) *
            scale - 0.5)`, `s = floor(f)`, `f -= s` in float32, clamped to the side with f = 0,
            weights `rint((1 - f) * 2048)` and `rint(f * 2048)`; a pixel is `R = S[i0] * a0 +
            S[i1] * a1` along the row, then `(((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16)
            + 2) >> 2` across the two rows
The package states the same rules in `ops.cv2_nearest_map`, `ops.cv2_nearest_map_vec` and
`ops.cv2_linear_taps` and builds flipped tables of the crop window from them; this tool shares no
code with those, so the two meet only in the result.  Everything else is the reference's own: which
keys are resized how, the uint32 and bool workarounds, the sizes, the draws and their order.

The fixture holds arrays and JSON only, in the layout of batch_augment.npz.  The inputs are NOT
stored: per case the seed, the recipe name and a SHA-256 of the regenerated inputs.

Per case <recipe>:
  params             JSON {recipe, seed, digest, crop, p, depth_mean, depth_std, raw_depth,
                     invalid_depth_value, scales | sizes | upscale}
  table              i32 [B,5]: (y0, x0, flip, rh, rw) per sample, from the dynamic parameters the
                     reference recorded
  out__<key>         the collated outputs, as in batch_augment.npz
  orientations       JSON [[id, angle], ...] per image after the chain

What each recipe is there for is asserted below; where it depends on the draws the tool walks the
seeds upwards from the listed one until it holds.

Usage: python tools/gen_golden_augment_resize.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nicr_mt_scene_analysis_amd.testing import synthetic as syn      # noqa: E402
from oracle import ref_loader                                        # noqa: E402

FIRST_SEEDS = {'RA': 80, 'RB': 81, 'RC': 82, 'RD': 83, 'RE': 84, 'RF': 85}
INVALID_DEPTH_VALUE = 0.0
INTER_NEAREST, INTER_LINEAR = 0, 1


def nearest_map(src, dst):
    ifx = 1.0 / (dst / src)
    return np.array([min(int(np.floor(x * ifx)), src - 1) for x in range(dst)], np.int64)


def linear_taps(src, dst):
    """per destination index (i0, i1, a0, a1)"""
    scale = 1.0 / (dst / src)
    taps = []
    for d in range(dst):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(np.floor(f))
        f = np.float32(f - np.float32(s))
        if s < 0:
            f, s = np.float32(0.0), 0
        if s >= src - 1:
            f, s = np.float32(0.0), src - 1
        taps.append((s, min(s + 1, src - 1), int(np.rint((np.float32(1.0) - f) * np.float32(2048.0))),
                     int(np.rint(f * np.float32(2048.0)))))
    return np.array(taps, np.int64).T


def resize_standin(value, dsize, interpolation=INTER_LINEAR):
    """numpy stand-in for cv2.resize(value, (width, height), interpolation=...)"""
    width, height = dsize
    assert width > 0 and height > 0 and value.ndim in (2, 3)
    if interpolation == INTER_NEAREST:
        rows, cols = nearest_map(value.shape[0], height), nearest_map(value.shape[1], width)
        return np.ascontiguousarray(value[rows[:, None], cols[None, :]])
    assert interpolation == INTER_LINEAR and value.dtype == np.uint8 and value.ndim == 3, 'the 8-bit linear path only'
    j0, j1, b0, b1 = linear_taps(value.shape[0], height)
    i0, i1, a0, a1 = linear_taps(value.shape[1], width)
    S = value.astype(np.int64)
    R = S[:, i0] * a0[None, :, None] + S[:, i1] * a1[None, :, None]               # horizontal pass, every source row
    out = (((b0[:, None, None] * (R[j0] >> 4)) >> 16) + ((b1[:, None, None] * (R[j1] >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return np.ascontiguousarray(out.astype(np.uint8))


def jdump(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


def to_sample(inp, b):
    """image b of the raw batch as the reference's per-sample dict"""
    s = {k: inp[k][b].copy() for k in syn.AUGMENT_SPATIAL_KEYS}
    s['instance'] = s['instance'].astype(np.uint16)          # the dtype the datasets store
    s['orientations'] = dict(inp['orientations'][b])
    return s


def run_case(mods, recipe, seed):
    resize, crop, flip, normalize, totorch = mods
    r = syn.AUGMENT_RESIZE_RECIPES[recipe]
    B, (ch, cw) = r['B'], r['crop']
    _, mean, std, raw_depth = r['depth']
    inp = syn.make_augment_resize_inputs(recipe, seed)
    chain = [crop.RandomCrop(crop_height=ch, crop_width=cw), flip.RandomHorizontalFlip(p=r['p']),
             normalize.NormalizeRGB(),
             normalize.NormalizeDepth(depth_mean=mean, depth_std=std, raw_depth=raw_depth,
                                      invalid_depth_value=INVALID_DEPTH_VALUE),
             totorch.ToTorchTensors()]
    if 'scales' in r:
        chain.insert(0, resize.RandomResize(min_scale=r['scales'][0], max_scale=r['scales'][1]))
    np.random.seed(seed)
    samples, table = [], np.zeros((B, 5), np.int32)
    for b in range(B):
        sample = to_sample(inp, b)
        if 'sizes' in r:
            sample = resize.resize(sample, height=r['sizes'][b][0], width=r['sizes'][b][1])
        for step in chain:
            sample = step(sample)
        meta = {m['type']: m for m in sample['_applied_preprocessing']}
        cropped = meta['RandomCrop']
        assert cropped['was_resized'] == ('upscale' in r)
        if 'scales' in r:
            assert (meta['RandomResize']['old_height'], meta['RandomResize']['old_width']) == (r['H'], r['W'])
            size = (meta['RandomResize']['new_height'], meta['RandomResize']['new_width'])
            assert size == (cropped['resize_height'], cropped['resize_width'])
        elif 'sizes' in r:
            size = tuple(r['sizes'][b])
            assert size == (cropped['resize_height'], cropped['resize_width'])
        else:
            size = (cropped['resize_height'], cropped['resize_width'])
        sy, sx = cropped['crop_slice_y'], cropped['crop_slice_x']
        assert (sy.stop - sy.start, sx.stop - sx.start) == (ch, cw)
        table[b] = (sy.start, sx.start, bool(meta['RandomHorizontalFlip']['was_flipped'])) + size
        samples.append(sample)
    return inp, samples, table


def holds(recipe, inp, table):
    """what the recipe is there for, as far as it depends on the draws"""
    r = syn.AUGMENT_RESIZE_RECIPES[recipe]
    H, W, (ch, cw) = r['H'], r['W'], r['crop']
    y0, x0, flip, rh, rw = table.T
    if recipe == 'RA':
        return set(flip) == {0, 1} and set(x0 % 2) == {0, 1} and (rh < H).any() and (rh > H).any()
    if recipe in ('RB', 'RF'):
        return ((rh != H) | (rw != W)).all()
    if recipe == 'RD':
        # inside the crop windows, OpenCV's double rule and x * src // dst part on rows and on columns
        differs = [False, False]
        for b in range(r['B']):
            for axis, (src, dst, start, n) in enumerate(((H, rh[b], y0[b], ch), (W, rw[b], x0[b], cw))):
                wrong = np.arange(dst) * src // dst
                differs[axis] |= bool((nearest_map(src, dst) != wrong)[start:start + n].any())
        return all(differs) and set(flip) == {0, 1}
    if recipe == 'RE':
        seen = np.concatenate([inp['depth'][b][nearest_map(H, rh[b])[y0[b]:y0[b] + ch]][:, nearest_map(W, rw[b])].ravel()
                               for b in range(r['B'])])
        bits = seen.view(np.uint32)
        return (bits == 0).any() and (bits == 0x80000000).any() and (seen == np.float32(r['depth'][1])).any()
    return True


def main():
    ref = ref_loader.load_reference()
    cv2 = sys.modules['cv2']                     # the loader's empty module
    assert not hasattr(cv2, 'resize'), 'a real cv2 is installed: use it instead of the stand-in'
    cv2.INTER_NEAREST, cv2.INTER_LINEAR, cv2.resize = INTER_NEAREST, INTER_LINEAR, resize_standin
    mods = (ref.resize,) + tuple(ref_loader._load(f'data.preprocessing.{m}', f'data/preprocessing/{m}.py')
                                 for m in ('crop', 'flip', 'normalize', 'torch'))
    out, names = {}, []
    for recipe, seed in FIRST_SEEDS.items():
        r = syn.AUGMENT_RESIZE_RECIPES[recipe]
        while True:
            inp, samples, table = run_case(mods, recipe, seed)
            if holds(recipe, inp, table):
                break
            seed += 1
        B, H, W, (ch, cw) = r['B'], r['H'], r['W'], r['crop']
        _, mean, std, raw_depth = r['depth']
        assert holds(recipe, inp, table), table
        assert ((table[:, 0] + ch <= table[:, 3]) & (table[:, 1] + cw <= table[:, 4])).all()
        if recipe == 'RC':                       # no scale draw, no offset draws: the window is the resized image
            assert (table[:, [0, 1, 3, 4]] == (0, 0, ch, cw)).all(), table
        if recipe == 'RD':
            assert table[:, 3:].tolist() == [list(s) for s in r['sizes']]
        if recipe == 'RE':
            assert (table[:, 3:] == (35, 40)).all() and (table[:, 1] == 0).all(), table
        pfx = f'{recipe}__'
        how = {k: r[k] for k in ('scales', 'sizes', 'upscale') if k in r}
        out[pfx + 'params'] = jdump({
            'recipe': recipe, 'seed': seed, 'digest': syn.augment_input_digest(inp), 'crop': [ch, cw], 'p': r['p'],
            'depth_mean': mean, 'depth_std': std, 'raw_depth': raw_depth,
            'invalid_depth_value': INVALID_DEPTH_VALUE, **how})
        out[pfx + 'table'] = table
        want_dtype = {'rgb': np.float32, 'depth': np.float32, 'semantic': np.uint8, 'instance': np.int32,
                      'normal': np.float32, 'valid': np.bool_, 'segment_ids': np.int64}
        for k in syn.AUGMENT_SPATIAL_KEYS:
            stacked = np.stack([s[k].numpy() for s in samples])
            assert stacked.dtype == want_dtype[k], (k, stacked.dtype)
            assert stacked.shape == (B,) + ({'rgb': (3,), 'normal': (3,), 'depth': (1,)}.get(k, ())) + (ch, cw), k
            out[pfx + 'out__' + k] = stacked
        out[pfx + 'orientations'] = jdump([[[int(i), float(a)] for i, a in s['orientations'].items()]
                                           for s in samples])
        names.append(recipe)
        print(recipe, 'seed', seed, 'table', table.tolist())
    # RC: an exact 2:1 downscale of rgb is the rounded mean of 2 x 2 pixels
    inp = syn.make_augment_resize_inputs('RC', json.loads(bytes(out['RC__params'].tobytes()).decode())['seed'])
    S = inp['rgb'].astype(np.int64)
    mean2x2 = (S[:, 0::2, 0::2] + S[:, 0::2, 1::2] + S[:, 1::2, 0::2] + S[:, 1::2, 1::2] + 2) >> 2
    rgb_mean = np.array((0.485, 0.456, 0.406), dtype='float32') * 255
    rgb_std = np.array((0.229, 0.224, 0.225), dtype='float32') * 255
    for b, (_, _, flip, _, _) in enumerate(out['RC__table']):
        want = (mean2x2[b, :, ::-1] if flip else mean2x2[b]).astype(np.float32)
        want = ((want - rgb_mean) / rgb_std).transpose(2, 0, 1)
        assert np.array_equal(want.view(np.uint32), out['RC__out__rgb'][b].view(np.uint32)), b
    out['names'] = jdump(names)
    path = os.path.join(ROOT, 'tests', 'golden', 'batch_augment_resize.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
