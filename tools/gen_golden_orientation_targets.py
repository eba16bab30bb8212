"""Writes tests/golden/orientation_targets.npz: the reference's unmodified
`data/preprocessing/orientation.py` (`OrientationTargetGenerator`), loaded through
`oracle.ref_loader` (`prep_orientation`), run per sample on CPU on the seeded cases of
`testing.synthetic.ORIENTATION_RECIPES`, once with the class list and once with `None`.

The fixture holds arrays and JSON only.  The label maps are NOT stored: per case the seed, the
recipe name and a SHA-256 of the regenerated inputs; the tests regenerate them and fail on a
digest mismatch.

Per case <recipe>__<list|none>:
  params          JSON {recipe, seed, digest, with_class_list}
  orientations    JSON: per image [[instance id, angle], ...] in dict order
  orientation     f32 [B,H,W,2], the reference's HWC images stacked
  foreground      np.packbits of bool [B,H,W]
  present         JSON: per image [[instance id, angle], ...] of `orientations_present`, in the
                  reference's (np.unique) order

Before writing, the tool asserts on the reference's own output that every case holds what the
recipe promises (see `check_case`).

Usage: python tools/gen_golden_orientation_targets.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nicr_mt_scene_analysis_amd.testing import synthetic as syn      # noqa: E402
from oracle import ref_loader                                        # noqa: E402

SEEDS = {'ragged': 50, 'wire': 51}


def jdump(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


def pairs(dicts):
    return [[[int(k), float(v)] for k, v in d.items()] for d in dicts]


def case_digest(inp):
    return syn.input_digest(inp['semantic'], inp['instance'], inp['estimate'],
                            jdump(pairs(inp['orientations'])))


def majority(inp, b, iid):
    votes = np.bincount(inp['semantic'][b][inp['instance'][b] == iid])
    return votes, int(votes.argmax())


def check_case(inp, present, with_list):
    sem, ins, est, ori = inp['semantic'], inp['instance'], inp['estimate'], inp['orientations']
    B, H, W = sem.shape
    in_map = set(np.unique(ins[0]).tolist())
    # an id in the map without an angle; an angle for an id that is not in the map
    assert syn.ORI_NO_ANGLE in in_map and syn.ORI_NO_ANGLE not in ori[0]
    assert syn.ORI_NOT_IN_MAP in ori[0] and syn.ORI_NOT_IN_MAP not in in_map
    assert syn.ORI_NO_ANGLE not in present[0] and syn.ORI_NOT_IN_MAP not in present[0]
    assert any(k not in np.unique(ins[1]) for k in ori[1])
    # an image with an empty dict
    assert ori[2] == {} and present[2] == {} and (ins[2] != 0).any()
    # majority class void / not flagged
    assert majority(inp, 0, syn.ORI_VOID)[1] == 0 and not est[0]
    c = majority(inp, 0, syn.ORI_UNFLAGGED)[1]
    assert c != 0 and not est[c]
    # exact ties between a flagged and an unflagged class, one in each order
    v, c = majority(inp, 0, syn.ORI_TIE_FLAGGED)
    assert v[1] == v[2] == v.max() and c == 1 and est[1] and not est[2]
    v, c = majority(inp, 0, syn.ORI_TIE_UNFLAGGED)
    assert v[2] == v[3] == v.max() and c == 2 and est[3] and not est[2]
    crafted = (syn.ORI_VOID, syn.ORI_UNFLAGGED, syn.ORI_TIE_FLAGGED, syn.ORI_TIE_UNFLAGGED)
    accepted = crafted if not with_list else (syn.ORI_TIE_FLAGGED,)
    for iid in crafted:
        assert (iid in present[0]) == (iid in accepted), (iid, with_list)
    if H >= 96:
        assert (ins[0] == syn.ORI_BIG).sum() > H * W // 2 and syn.ORI_BIG in ori[0]
    angles = [a for d in ori for a in d.values()]
    assert 0.0 in angles and float(np.pi) in angles and min(angles) < 0 and max(angles) > 2 * np.pi
    assert sum(len(p) for p in present) > 2


def main():
    ref = ref_loader.load_reference(task_helpers=True)
    Generator = ref.prep_orientation.OrientationTargetGenerator
    out = {}
    names = []
    for recipe, seed in SEEDS.items():
        inp = syn.make_orientation_inputs(recipe, seed)
        digest = case_digest(inp)
        B = inp['semantic'].shape[0]
        for tag, flags in (('list', tuple(bool(f) for f in inp['estimate'])), ('none', None)):
            gen = Generator(semantic_classes_estimate_orientation=flags)
            images, fgs, present = [], [], []
            for b in range(B):
                sample = gen({'semantic': inp['semantic'][b].copy(), 'instance': inp['instance'][b].copy(),
                              'orientations': dict(inp['orientations'][b])})
                assert sample['orientation'].dtype == np.float32 and sample['orientation_foreground'].dtype == bool
                images.append(sample['orientation'])
                fgs.append(sample['orientation_foreground'])
                present.append({int(k): float(v) for k, v in sample['orientations_present'].items()})
            check_case(inp, present, flags is not None)
            name = f'{recipe}__{tag}'
            names.append(name)
            out[f'{name}__params'] = jdump({'recipe': recipe, 'seed': seed, 'digest': digest,
                                            'with_class_list': flags is not None})
            out[f'{name}__orientations'] = jdump(pairs(inp['orientations']))
            out[f'{name}__orientation'] = np.stack(images)
            out[f'{name}__foreground'] = np.packbits(np.stack(fgs).reshape(-1))
            out[f'{name}__present'] = jdump(pairs(present))
            print(name, 'painted px', int(np.stack(fgs).sum()), 'present', [len(p) for p in present])
    out['names'] = jdump(names)
    path = os.path.join(ROOT, 'tests', 'golden', 'orientation_targets.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
