"""numpy reference of `OrientationTargetGenerator` (reference data/preprocessing/orientation.py:
59-95) and the small helpers around it, shared by tests/test_orientation_targets.py and
tests/test_targets_routes.py."""
import numpy as np


def restate(sem, ins, orientations, estimate):
    """the rule of reference orientation.py:59-95 for a batch: per image and instance id (ascending,
    0 skipped) that has an angle: majority class over the mask (bincount.argmax: a tie goes to the
    smaller class, void counts) must be flagged when a class list is given; then the biternion is
    painted over the mask.  -> orientation f32 [B,2,H,W], foreground bool [B,H,W], list of dicts"""
    B, H, W = sem.shape
    ori = np.zeros((B, 2, H, W), np.float32)
    fg = np.zeros((B, H, W), bool)
    present = []
    for b in range(B):
        ids, inv = np.unique(ins[b], return_inverse=True)
        inv = inv.reshape(-1)
        nc = int(sem[b].max()) + 1 if estimate is None else max(len(estimate), int(sem[b].max()) + 1)
        votes = np.bincount(inv * nc + sem[b].reshape(-1).astype(np.int64), minlength=len(ids) * nc)
        major = votes.reshape(len(ids), nc).argmax(axis=1)
        table = np.zeros((len(ids), 2), np.float32)
        accept = np.zeros((len(ids),), bool)
        pres = {}
        for i, iid in enumerate(ids.tolist()):
            if iid == 0 or iid not in orientations[b]:
                continue
            if estimate is not None and not estimate[major[i]]:
                continue
            rad = orientations[b][iid]
            table[i] = np.array([np.cos(rad), np.sin(rad)], dtype='float32')
            accept[i] = True
            pres[iid] = rad
        ori[b, 0] = table[inv, 0].reshape(H, W)
        ori[b, 1] = table[inv, 1].reshape(H, W)
        fg[b] = accept[inv].reshape(H, W)
        present.append(pres)
    return ori, fg, present


def paint_present(ins, present):
    """the image that follows from the masks and the dicts of accepted ids alone"""
    B, H, W = ins.shape
    ori = np.zeros((B, 2, H, W), np.float32)
    for b in range(B):
        for iid, rad in present[b].items():
            bit = np.array([np.cos(rad), np.sin(rad)], dtype='float32')
            ori[b, 0][ins[b] == iid] = bit[0]
            ori[b, 1][ins[b] == iid] = bit[1]
    return ori


def ulp_distance(a, b):
    def ordered(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(ordered(a) - ordered(b))


def assert_bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def pack_keys(orientations, pad=64):
    ids = [sorted(k for k in d if 1 <= k <= 65535) for d in orientations]
    K = max(pad, -(-max(len(i) for i in ids) // pad) * pad)
    B = len(ids)
    keys = np.zeros((B, K), np.int32)
    bit = np.zeros((B, K, 2), np.float32)
    for b, i in enumerate(ids):
        keys[b, :len(i)] = i
        for k, iid in enumerate(i):
            bit[b, k] = np.array([np.cos(orientations[b][iid]), np.sin(orientations[b][iid])], dtype='float32')
    return keys, np.array([len(i) for i in ids], np.int32), bit


def random_angles(ins, rng, fraction=0.6):
    out = []
    for b in range(ins.shape[0]):
        ids = np.unique(ins[b])
        d = {int(i): float(rng.uniform(-np.pi, 3 * np.pi)) for i in ids if i > 0 and rng.random() < fraction}
        d[int(ids.max()) % 65535 + 1] = 0.25          # (an extra key; it may or may not be in the map)
        out.append(d)
    return out
