"""CPU tier: the host checks of nmsa_batch_augment_resized (csrc/augment_resize.hip).  Every field of
the descriptor table and every entry of the window tables is checked on the host copy before
anything is enqueued — a table entry that left the source would be a GPU fault —, so a bad buffer
comes back as NMSA_ERR_ARG (-1) or NMSA_ERR_UNSUPPORTED (-4) without a device: nothing below reaches
a HIP call, and the fake addresses are never dereferenced."""
import ctypes as C

import numpy as np
import pytest

from nicr_mt_scene_analysis_amd import _lib as L
from nicr_mt_scene_analysis_amd import ops

ARG, UNSUPPORTED = -1, -4
WORDS = 24
B, H, W, h, w = 2, 36, 63, 24, 44
# word offsets within a descriptor (include/nmsa.h, nmsa_augment_resize_desc)
SRC, DST, NB, SH, SW, CH, CROP_H, CROP_W, MODE, LOG2, OUT_DTYPE, RAW = 0, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13
MEAN, STD = 16, 19
MOVE, RGB_NORM, DEPTH_NORM = 0, 1, 2
# the tables behind the descriptors: [B, w] x 3, then [B, h] x 3
COL_NEAR, COL_TAPS, COL_WTS = 0, B * w, 2 * B * w
ROW_NEAR, ROW_TAPS, ROW_WTS = 3 * B * w, 3 * B * w + B * h, 3 * B * w + 2 * B * h


def descriptor(mode, channels, log2_size, src=0x10000, dst=0x20000):
    d = np.zeros((WORDS,), np.int32)
    d[:4].view(np.uint64)[:] = (src, dst)
    d[NB:RAW + 1] = (B, H, W, channels, h, w, mode, log2_size, L.NMSA_F32, 0)
    d[MEAN:MEAN + 3].view(np.float32)[:] = (123.675, 116.28, 103.53)
    d[STD:STD + 3].view(np.float32)[:] = (58.395, 57.12, 57.375)
    return d


GOOD = {'move': descriptor(MOVE, 3, 2), 'rgb': descriptor(RGB_NORM, 3, 0), 'depth': descriptor(DEPTH_NORM, 1, 1)}
# the first window ends on the last row and column of an upscaled image, the second is a whole downscaled one
TABLES = np.concatenate([t.ravel() for t in ops.augment_window_tables(
    [[20, 33, 1, 44, 77], [0, 0, 0, 24, 44]], (H, W), (h, w))])
assert TABLES[COL_NEAR:COL_TAPS].max() == W - 1 and TABLES[ROW_NEAR:ROW_TAPS].max() == H - 1


def rc(descs, tables=TABLES, n_desc=None, n_samples=B, n_words=None, host=None, device=0x3000):
    buf = np.zeros((len(descs) * WORDS + len(tables) + 4 + 4,), np.int32)
    at = (-buf.ctypes.data // 4) % 4                                   # the staging is 16-byte aligned
    buf = buf[at:at + len(descs) * WORDS + len(tables) + 4]
    assert buf.ctypes.data % 16 == 0
    buf[:len(descs) * WORDS] = np.concatenate(descs)
    buf[len(descs) * WORDS:len(descs) * WORDS + len(tables)] = tables
    return L.lib().nmsa_batch_augment_resized(
        C.c_void_p(buf.ctypes.data if host is None else host), C.c_void_p(device),
        len(descs) if n_desc is None else n_desc, n_samples,
        len(descs) * WORDS + len(tables) if n_words is None else n_words, None)


def broken(kind, at, value, as_float=False):
    bad = GOOD[kind].copy()
    if as_float:
        bad[at:at + 1].view(np.float32)[:] = value
    else:
        bad[at] = value
    return [bad]


def with_entry(at, value):
    tables = TABLES.copy()
    tables[at] = value
    return tables


def pair(low, high):
    return int(np.array([low | (high << 16)], np.uint32).view(np.int32)[0])


def test_the_unbroken_buffer_passes_the_checks():
    """the buffer every other test breaks in one place gets past the checks: without a device the
    call then fails at its first HIP call (NMSA_ERR_LAUNCH, -2).  Not run where a device exists:
    the addresses are fake."""
    import torch
    if torch.cuda.is_available():
        pytest.skip('only without a device: the table holds fake addresses')
    assert rc(list(GOOD.values())) == -2
    for d in GOOD.values():
        assert rc([d]) == -2
    # the largest weight and the last row and column as taps are inside the ranges
    assert rc([GOOD['rgb']], with_entry(COL_WTS, pair(2048, 0))) == -2
    assert rc([GOOD['rgb']], with_entry(COL_TAPS, pair(W - 1, W - 1))) == -2


def test_call_level_arguments():
    good = list(GOOD.values())
    assert rc(good, n_desc=0) == ARG and rc(good, n_desc=-1) == ARG
    assert rc(good * 86, n_desc=257, n_words=1 << 20) == ARG          # above NMSA_AUGMENT_MAX_DESC
    assert rc(good, device=0) == ARG and rc(good, host=0) == ARG
    assert rc(good, device=0x3008) == ARG                              # staging is 16-byte aligned
    assert rc(good, n_samples=0) == ARG
    assert rc(good, n_words=3 * WORDS + len(TABLES) - 1) == ARG        # the tables do not fit
    assert rc(good, n_words=3 * WORDS - 1) == ARG and rc(good, n_words=0) == ARG
    assert rc(good, n_samples=3) == ARG


@pytest.mark.parametrize('kind', sorted(GOOD))
def test_fields_every_mode_checks(kind):
    for at, value in ((SRC, 0), (DST, 0),                              # NULL
                      (NB, 0), (NB, B + 1), (NB, -1),                  # samples: positive, equal to n_samples
                      (SH, 0), (SW, -5), (CH, 0), (CH, -1), (CROP_H, 0), (CROP_W, 0), (CROP_W, -1),
                      (CROP_H, h + 1), (CROP_W, w + 4),                # the tables of that window do not fit
                      (SH, H - 1), (SW, W - 1),                        # a nearest entry leaves this source
                      (MODE, 3), (MODE, -1), (LOG2, -1), (LOG2, 4)):
        assert rc(broken(kind, at, value)) == ARG, (kind, at, value)


def test_descriptors_share_one_window():
    other = GOOD['move'].copy()
    other[CROP_H] = h - 1
    assert rc([GOOD['move'], other]) == ARG and rc([other, GOOD['move']]) == ARG
    small = GOOD['move'].copy()                                        # the entries are checked against every source
    small[SW] = W - 1
    assert rc([GOOD['move'], small]) == ARG


def test_pointer_alignment():
    assert rc(broken('move', SRC, 0x10002)) == ARG and rc(broken('move', DST, 0x20002)) == ARG     # 4-byte elements
    assert rc(broken('depth', SRC, 0x10001)) == ARG                   # uint16 source
    assert rc(broken('depth', DST, 0x20002)) == ARG and rc(broken('rgb', DST, 0x20002)) == ARG     # float32 results
    assert rc([descriptor(MOVE, 1, 3, src=0x10004)]) == ARG           # 8-byte elements on 4


def test_table_entries():
    every = list(GOOD.values())
    for at, limit in ((COL_NEAR, W), (COL_NEAR + B * w - 1, W), (ROW_NEAR, H), (ROW_NEAR + B * h - 1, H)):
        for value in (-1, limit, 1 << 30, -(1 << 31)):
            for descs in (every, [GOOD['move']], [GOOD['depth']]):
                assert rc(descs, with_entry(at, value)) == ARG, (at, value)
    for at, limit in ((COL_TAPS, W), (COL_TAPS + B * w - 1, W), (ROW_TAPS, H), (ROW_TAPS + B * h - 1, H)):
        for value in (pair(limit, 0), pair(0, limit), pair(65535, 65535), -1):
            assert rc(every, with_entry(at, value)) == ARG and rc([GOOD['rgb']], with_entry(at, value)) == ARG, (at, value)
    for at in (COL_WTS, COL_WTS + B * w - 1, ROW_WTS, ROW_WTS + B * h - 1):
        for value in (pair(2049, 0), pair(0, 2049), pair(0, 32768), -1):
            assert rc(every, with_entry(at, value)) == ARG, (at, value)


def test_mode_specific_fields():
    assert rc(broken('rgb', CH, 1)) == ARG and rc(broken('rgb', CH, 4)) == ARG           # C != 3
    assert rc(broken('rgb', LOG2, 2)) == ARG                                              # the source is uint8
    assert rc(broken('depth', CH, 3)) == ARG
    assert rc(broken('depth', LOG2, 0)) == ARG and rc(broken('depth', LOG2, 3)) == ARG   # uint16 or float32
    for c in range(3):
        assert rc(broken('rgb', STD + c, 0.0, as_float=True)) == ARG, c
        assert rc(broken('rgb', STD + c, -0.0, as_float=True)) == ARG, c
    assert rc(broken('depth', STD, 0.0, as_float=True)) == ARG
    assert rc(broken('rgb', OUT_DTYPE, L.NMSA_F16)) == UNSUPPORTED
    assert rc(broken('depth', OUT_DTYPE, L.NMSA_F16)) == UNSUPPORTED
    assert rc(broken('rgb', OUT_DTYPE, L.NMSA_BF16)) == ARG and rc(broken('depth', OUT_DTYPE, 7)) == ARG
    # the taps are half words: an rgb source side above 65536 cannot be addressed
    assert rc(broken('rgb', SW, 65537)) == ARG and rc(broken('rgb', SH, 65537)) == ARG


def test_element_count_above_int32():
    # 2^15 x 2^15 window, 2 samples: the tables alone pass (all zeros), the element count does not
    big = GOOD['move'].copy()
    big[[CROP_H, CROP_W]] = 32768
    tables = np.zeros((3 * B * 2 * 32768,), np.int32)
    assert rc([big], tables) == ARG
    one = big.copy()
    one[CH] = 1                                                        # 2 * 2^30 = 2^31
    assert rc([one], tables) == ARG
    many = GOOD['move'].copy()
    many[CH] = 1 << 30
    assert rc([many]) == ARG
