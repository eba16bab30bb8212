"""CPU tier: the host checks of nmsa_batch_augment (csrc/augment.hip).  Every field of the
descriptor table and every sample's window is checked on the host copy before anything is
enqueued, so a bad table comes back as NMSA_ERR_ARG (-1) or NMSA_ERR_UNSUPPORTED (-4) without a
device: nothing below reaches a HIP call, and the fake addresses are never dereferenced."""
import ctypes as C

import numpy as np
import pytest

from nicr_mt_scene_analysis_amd import _lib as L

ARG, UNSUPPORTED = -1, -4
WORDS = 24
B, H, W, h, w = 2, 41, 67, 37, 50
# word offsets within a descriptor (include/nmsa.h, nmsa_augment_desc)
SRC, DST, NB, SH, SW, CH, CROP_H, CROP_W, MODE, LOG2, OUT_DTYPE, RAW = 0, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13
MEAN, STD = 16, 19
MOVE, RGB_NORM, DEPTH_NORM = 0, 1, 2


def descriptor(mode, channels, log2_size, src=0x10000, dst=0x20000):
    d = np.zeros((WORDS,), np.int32)
    d[:4].view(np.uint64)[:] = (src, dst)
    d[NB:RAW + 1] = (B, H, W, channels, h, w, mode, log2_size, L.NMSA_F32, 0)
    d[MEAN:MEAN + 3].view(np.float32)[:] = (123.675, 116.28, 103.53)
    d[STD:STD + 3].view(np.float32)[:] = (58.395, 57.12, 57.375)
    return d


GOOD = {'move': descriptor(MOVE, 3, 2), 'rgb': descriptor(RGB_NORM, 3, 0), 'depth': descriptor(DEPTH_NORM, 1, 1)}
PARAMS = np.array([[4, 17, 1], [0, 0, 0]], np.int32)           # the last window: y0 + h == H, x0 + w == W


def rc(descs, params=PARAMS, n_desc=None, n_samples=B, n_words=None, host=None, device=0x3000):
    buf = np.concatenate([np.concatenate(descs), np.asarray(params, np.int32).ravel(), np.zeros((2,), np.int32)])
    assert buf.ctypes.data % 8 == 0
    return L.lib().nmsa_batch_augment(
        C.c_void_p(buf.ctypes.data if host is None else host), C.c_void_p(device),
        len(descs) if n_desc is None else n_desc, n_samples,
        len(descs) * WORDS + 3 * n_samples if n_words is None else n_words, None)


def broken(kind, at, value, as_float=False):
    bad = GOOD[kind].copy()
    if as_float:
        bad[at:at + 1].view(np.float32)[:] = value
    else:
        bad[at] = value
    return [bad]


def test_the_unbroken_table_passes_the_checks():
    """the table every other test breaks in one place gets past the checks: without a device the
    call then fails at its first HIP call (NMSA_ERR_LAUNCH, -2).  Not run where a device exists:
    the addresses are fake."""
    import torch
    if torch.cuda.is_available():
        pytest.skip('only without a device: the table holds fake addresses')
    assert rc(list(GOOD.values())) == -2
    for d in GOOD.values():
        assert rc([d]) == -2


def test_call_level_arguments():
    good = list(GOOD.values())
    assert rc(good, n_desc=0) == ARG and rc(good, n_desc=-1) == ARG
    assert rc(good * 86, n_desc=257, n_words=1 << 20) == ARG          # above NMSA_AUGMENT_MAX_DESC
    assert rc(good, device=0) == ARG and rc(good, host=0) == ARG
    assert rc(good, device=0x3004) == ARG                              # staging is 8-byte aligned
    assert rc(good, n_samples=0) == ARG
    assert rc(good, n_words=3 * WORDS + 3 * B - 1) == ARG              # the parameters do not fit
    assert rc(good, n_samples=3, n_words=3 * WORDS + 3 * B) == ARG


@pytest.mark.parametrize('kind', sorted(GOOD))
def test_fields_every_mode_checks(kind):
    for at, value in ((SRC, 0), (DST, 0),                              # NULL
                      (NB, 0), (NB, B + 1), (NB, -1),                  # samples: positive, equal to n_samples
                      (SH, 0), (SW, -5), (CH, 0), (CH, -1), (CROP_H, 0), (CROP_W, 0), (CROP_W, -1),
                      (CROP_H, H + 1), (CROP_W, W + 1),                # h > H, w > W
                      (MODE, 3), (MODE, -1), (LOG2, -1), (LOG2, 4)):
        assert rc(broken(kind, at, value)) == ARG, (kind, at, value)


def test_pointer_alignment():
    assert rc(broken('move', SRC, 0x10002)) == ARG and rc(broken('move', DST, 0x20002)) == ARG     # 4-byte elements
    assert rc(broken('depth', SRC, 0x10001)) == ARG                   # uint16 source
    assert rc(broken('depth', DST, 0x20002)) == ARG and rc(broken('rgb', DST, 0x20002)) == ARG     # float32 results
    wide = descriptor(MOVE, 1, 3, src=0x10004)
    assert rc([wide]) == ARG                                           # 8-byte elements on 4


def test_sample_windows_and_flips():
    good = [GOOD['move']]
    for bad in ([[5, 17, 1], [0, 0, 0]], [[4, 18, 0], [0, 0, 0]], [[4, 17, 1], [-1, 0, 0]], [[4, 17, 1], [0, -1, 0]],
                [[4, 17, 2], [0, 0, 0]], [[4, 17, 1], [0, 0, -1]], [[1 << 30, 0, 0], [0, 0, 0]]):
        assert rc(good, params=bad) == ARG, bad
    # the windows are checked against every descriptor's own source
    small = GOOD['move'].copy()
    small[SH] = H - 1
    assert rc([GOOD['move'], small]) == ARG


def test_mode_specific_fields():
    assert rc(broken('rgb', CH, 1)) == ARG and rc(broken('rgb', CH, 4)) == ARG           # C != 3
    assert rc(broken('rgb', LOG2, 2)) == ARG                                              # the source is uint8
    assert rc(broken('depth', CH, 3)) == ARG
    assert rc(broken('depth', LOG2, 0)) == ARG and rc(broken('depth', LOG2, 3)) == ARG   # uint16 or float32
    for c in range(3):
        assert rc(broken('rgb', STD + c, 0.0, as_float=True)) == ARG, c
        assert rc(broken('rgb', STD + c, -0.0, as_float=True)) == ARG, c
    assert rc(broken('depth', STD, 0.0, as_float=True)) == ARG
    # float16 results are the reference's `output_dtype`, not built here; bfloat16 is nobody's
    assert rc(broken('rgb', OUT_DTYPE, L.NMSA_F16)) == UNSUPPORTED
    assert rc(broken('depth', OUT_DTYPE, L.NMSA_F16)) == UNSUPPORTED
    assert rc(broken('rgb', OUT_DTYPE, L.NMSA_BF16)) == ARG and rc(broken('depth', OUT_DTYPE, 7)) == ARG


def test_element_count_above_int32():
    big = GOOD['move'].copy()
    big[[SH, SW, CROP_H, CROP_W]] = 32768                              # 2 * 3 * 2^30
    assert rc([big], params=[[0, 0, 0], [0, 0, 0]]) == ARG
    big[CH] = 1
    big[CROP_W] = 32768 // 2                                           # 2 * 2^15 * 2^14 = 2^30 passes; 2^31 does not
    big[NB] = 4
    assert rc([big], params=np.zeros((4, 3), np.int32), n_samples=4) == ARG
    many = GOOD['move'].copy()
    many[CH] = 1 << 30
    assert rc([many]) == ARG
