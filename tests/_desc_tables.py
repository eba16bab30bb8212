"""Helpers of the descriptor-table tests (test_desc_tables_reference.py, test_desc_table_launches.py,
test_staging_caches.py): the word layout of `nmsa_augment_desc` and `nmsa_multiscale_desc`
(include/nmsa.h), launches of the two C entry points straight from a pinned table, a device arena
with poison around everything it hands out, and plain numpy formulations of the two operations.

Nothing on the reference side is project code: the references are numpy slices, `np.flip`,
`transpose`, fancy indexing and float32 arithmetic (one subtract, one divide).  Importing this
module needs no device."""
import ctypes as C

import numpy as np

# ------------------------------------------------------------------------------- word layouts
# nmsa_augment_desc, 24 words (two uint64, twelve int32, seven float32, one reserved int32)
AUG_WORDS = 24
(A_SRC, A_DST, A_B, A_SH, A_SW, A_C, A_CROP_H, A_CROP_W, A_MODE, A_LOG2, A_OUT_DTYPE, A_RAW,
 A_BLOCK_BEGIN, A_PPL, A_MEAN, A_STD, A_INVALID, A_RESERVED) = 0, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 19, 22, 23
AUG_FIELDS = {'src': A_SRC, 'dst': A_DST, 'B': A_B, 'H': A_SH, 'W': A_SW, 'C': A_C, 'h': A_CROP_H, 'w': A_CROP_W,
              'mode': A_MODE, 'log2_size': A_LOG2, 'out_dtype': A_OUT_DTYPE, 'raw_depth': A_RAW,
              'block_begin': A_BLOCK_BEGIN, 'pixels_per_lane': A_PPL, 'mean': A_MEAN, 'std': A_STD,
              'invalid_depth_value': A_INVALID, 'reserved': A_RESERVED}
MOVE, RGB_NORM, DEPTH_NORM = 0, 1, 2
AUG_MAX_DESC, AUG_THREADS = 256, 256

# nmsa_multiscale_desc, 16 words (two uint64, nine int32, three reserved int32)
MS_WORDS = 16
M_SRC, M_DST, M_PLANES, M_SH, M_SW, M_H, M_W, M_LOG2, M_ROW_MAP, M_COL_MAP, M_BLOCK_BEGIN, M_RESERVED = \
    0, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13
MS_FIELDS = {'src': M_SRC, 'dst': M_DST, 'planes': M_PLANES, 'H': M_SH, 'W': M_SW, 'h': M_H, 'w': M_W,
             'log2_size': M_LOG2, 'row_map': M_ROW_MAP, 'col_map': M_COL_MAP, 'block_begin': M_BLOCK_BEGIN,
             'reserved': M_RESERVED}
MS_MAX_DESC, MS_THREADS = 1024, 256

NMSA_F32 = 0
DEVICE = 'cuda'


def augment_desc(src, dst, B, H, W, channels, h, w, mode=MOVE, log2_size=0, raw_depth=0,
                 mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), invalid=0.0, out_dtype=NMSA_F32):
    """the 24 words of one nmsa_augment_desc; block_begin and pixels_per_lane are the call's"""
    d = np.zeros((AUG_WORDS,), np.int32)
    d[A_SRC:A_SRC + 4].view(np.uint64)[:] = (src, dst)
    d[A_B:A_RAW + 1] = (B, H, W, channels, h, w, mode, log2_size, out_dtype, raw_depth)
    d[A_MEAN:A_MEAN + 3].view(np.float32)[:] = mean
    d[A_STD:A_STD + 3].view(np.float32)[:] = std
    d[A_INVALID:A_INVALID + 1].view(np.float32)[:] = invalid
    return d


def multiscale_desc(src, dst, planes, H, W, h, w, log2_size, row_map, col_map):
    """the 16 words of one nmsa_multiscale_desc; block_begin is the call's"""
    d = np.zeros((MS_WORDS,), np.int32)
    d[M_SRC:M_SRC + 4].view(np.uint64)[:] = (src, dst)
    d[M_PLANES:M_COL_MAP + 1] = (planes, H, W, h, w, log2_size, row_map, col_map)
    return d


# ------------------------------------------------------------------------------- launches
def _launch(fn_name, words, args_after_staging):
    import torch
    from nicr_mt_scene_analysis_amd import _lib as L
    words = np.ascontiguousarray(words, np.int32)
    host = torch.empty((len(words),), dtype=torch.int32).pin_memory()
    host.numpy()[:] = words
    device = torch.empty_like(host, device=DEVICE)
    assert host.data_ptr() % 8 == 0 and device.data_ptr() % 8 == 0
    rc = getattr(L.lib(), fn_name)(C.c_void_p(host.data_ptr()), C.c_void_p(device.data_ptr()),
                                   *args_after_staging, len(words), L.stream_ptr(device.device))
    L.check(rc, fn_name)
    torch.cuda.synchronize()
    return host.numpy().copy()


def launch_augment(descs, params, tail=()):
    """one nmsa_batch_augment call on the current stream of `descs` (24-word arrays) and the
    [B,3] table `params`, `tail` further words behind them; synchronised -> the host words after
    the call, as [n_desc, 24]"""
    params = np.asarray(params, np.int32).reshape(-1, 3)
    words = np.concatenate([np.concatenate(descs), params.ravel(), np.asarray(tail, np.int32)])
    after = _launch('nmsa_batch_augment', words, (len(descs), len(params)))
    assert np.array_equal(after[len(descs) * AUG_WORDS:], words[len(descs) * AUG_WORDS:])
    return after[:len(descs) * AUG_WORDS].reshape(len(descs), AUG_WORDS)


def launch_multiscale(descs, maps, tail=()):
    """one nmsa_multiscale_nearest call on the current stream of `descs` (16-word arrays) and the
    concatenated int32 `maps`, `tail` further words behind them; synchronised -> the host words
    after the call, as [n_desc, 16]"""
    words = np.concatenate([np.concatenate(descs), np.asarray(maps, np.int32), np.asarray(tail, np.int32)])
    after = _launch('nmsa_multiscale_nearest', words, (len(descs),))
    assert np.array_equal(after[len(descs) * MS_WORDS:], words[len(descs) * MS_WORDS:])
    return after[:len(descs) * MS_WORDS].reshape(len(descs), MS_WORDS)


# ------------------------------------------------------------------------------- arena
class Arena:
    """One uint8 device tensor filled with PATTERN.  `put` copies a source into it, `take`
    reserves an output; both at `address % align == misalign` with at least GUARD pattern bytes
    on either side.  `check_guards` asserts that every byte outside the ranges handed out still
    holds the pattern, `check_sources` that every source still holds what was put there."""
    PATTERN = 0xA5
    GUARD = 64

    def __init__(self, nbytes):
        import torch
        self.buf = torch.full((int(nbytes) + 2 * self.GUARD + 256,), self.PATTERN, dtype=torch.uint8, device=DEVICE)
        self.base = self.buf.data_ptr()
        self.cursor = 0
        self.ranges, self.sources = [], []

    @staticmethod
    def room(nbytes, align=256):
        """bytes to reserve in the constructor for one range of `nbytes` at `align`"""
        return int(nbytes) + 2 * Arena.GUARD + int(align)

    def take(self, nbytes, align=256, misalign=0):
        """-> device address of `nbytes` reserved bytes"""
        nbytes, align, misalign = int(nbytes), int(align), int(misalign)
        assert nbytes > 0 and align > 0 and 0 <= misalign < align
        at = self.cursor + self.GUARD
        at += (misalign - (self.base + at)) % align
        assert (self.base + at) % align == misalign and at - self.cursor >= self.GUARD
        assert at + nbytes + self.GUARD <= self.buf.numel(), 'the arena is too small'
        self.ranges.append((at, at + nbytes))
        self.cursor = at + nbytes
        return self.base + at

    def put(self, array, align=256, misalign=0):
        """-> device address of a copy of `array` (C order)"""
        import torch
        raw = np.ascontiguousarray(array).reshape(-1).view(np.uint8).copy()
        address = self.take(raw.size, align, misalign)
        at = address - self.base
        self.buf[at:at + raw.size] = torch.from_numpy(raw).to(DEVICE)
        self.sources.append((at, raw))
        return address

    def read(self, address, nbytes):
        """-> the `nbytes` bytes at `address` as a uint8 array"""
        at = address - self.base
        assert any(lo <= at and at + nbytes <= hi for lo, hi in self.ranges)
        return self.buf[at:at + int(nbytes)].cpu().numpy()

    def check_guards(self):
        host = self.buf.cpu().numpy()
        outside = np.ones(host.shape, bool)
        for lo, hi in self.ranges:
            outside[lo:hi] = False
        assert outside[:self.GUARD].all() and outside[-self.GUARD:].all()
        bad = np.flatnonzero(outside & (host != self.PATTERN))
        assert bad.size == 0, f'{bad.size} bytes outside the ranges handed out were written, first at {bad[:8]} ' \
                              f'(ranges {[r for r in self.ranges if abs(r[0] - bad[0]) < 4096 or abs(r[1] - bad[0]) < 4096]})'

    def check_sources(self):
        host = self.buf.cpu().numpy()
        for at, raw in self.sources:
            assert np.array_equal(host[at:at + raw.size], raw), f'the source at offset {at} was written'


# ------------------------------------------------------------------------------- references
def raw_bytes(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def augment_reference(src, table, hw, mode=MOVE, mean=None, std=None, raw_depth=False, invalid=0.0):
    """`src` [B,H,W,C] -> [B,C,h,w]: per sample the window, flipped along x when asked, channels
    first; RGB_NORM / DEPTH_NORM then one float32 subtract and one float32 divide, DEPTH_NORM
    with `raw_depth` keeping elements whose float32 value equals the invalid value"""
    h, w = hw
    assert src.ndim == 4 and len(table) == src.shape[0]
    out = []
    for b, (y0, x0, flipped) in enumerate(np.asarray(table).tolist()):
        v = src[b, y0:y0 + h, x0:x0 + w]
        assert v.shape[:2] == (h, w)
        if flipped:
            v = np.flip(v, axis=1)
        out.append(v.transpose(2, 0, 1))
    out = np.ascontiguousarray(np.stack(out))
    if mode == MOVE:
        return out
    mean32 = np.asarray(mean, np.float32).reshape(-1)
    std32 = np.asarray(std, np.float32).reshape(-1)
    assert mean32.size == std32.size == out.shape[1]
    v32 = out.astype(np.float32)
    with np.errstate(all='ignore'):
        normed = (v32 - mean32[None, :, None, None]) / std32[None, :, None, None]
        if mode == RGB_NORM:
            return normed
        invalid32 = np.float32(invalid)
        return np.where(bool(raw_depth) & (v32 == invalid32), invalid32, normed).astype(np.float32)


def multiscale_reference(src, rows, cols):
    """`src` [planes,H,W] -> [planes,h,w]: src[:, rows][:, :, cols]"""
    assert src.ndim == 3
    return np.ascontiguousarray(src[:, np.asarray(rows)][:, :, np.asarray(cols)])


# ------------------------------------------------------------------------------- whole launches
SPECIAL_BITS32 = (0x7fc00000, 0xffc00001, 0x7f800123, 0x80000000, 0x00000000, 0x7f800000, 0xff800000,
                  0x00000001, 0x807fffff)
SPECIAL_BITS64 = (0x7ff8000000000000, 0xfff8000000000001, 0x7ff0000000000123, 0x8000000000000000, 0,
                  0x7ff0000000000000, 0xfff0000000000000, 1, 0x800fffffffffffff)


def random_bits(rng, shape, size):
    """unsigned elements of `size` bytes drawn over the whole range; the 4- and 8-byte ones with
    NaN payloads, -0.0, infinities and denormals strewn in"""
    dtype = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[size]
    a = rng.integers(0, np.iinfo(dtype).max, shape, dtype=dtype, endpoint=True)
    if size >= 4:
        strewn = rng.random(shape) < 0.25
        a[strewn] = rng.choice(np.array(SPECIAL_BITS32 if size == 4 else SPECIAL_BITS64, dtype), size=int(strewn.sum()))
    return a


def vec_bytes(dst_size):
    """bytes of the kernel's four-pixel store of `dst_size`-byte elements (include/nmsa.h:
    pixels_per_lane is 4 where w % 4 == 0 and the destination allows it)"""
    return min(16, 4 * dst_size)


def run_augment(cases, table, tail=()):
    """One launch of `cases`, each a dict: src [B,H,W,C] array, hw (h, w), and optionally mode,
    mean, std, raw_depth, invalid, align / misalign of the destination (default 256 / 0) and of
    the source (src_align / src_misalign, default 256 / 0).  Every output is compared with
    `augment_reference` as bytes, the guards and the sources are checked.
    -> (words read back [n,24], outputs as arrays [B,C,h,w])"""
    table = np.asarray(table, np.int32).reshape(-1, 3)
    B = len(table)
    sizes = []
    for c in cases:
        src, (h, w) = c['src'], c['hw']
        assert src.ndim == 4 and src.shape[0] == B
        out_size = src.dtype.itemsize if c.get('mode', MOVE) == MOVE else 4
        sizes.append((src.nbytes, B * src.shape[3] * h * w * out_size))
    arena = Arena(sum(Arena.room(s, c.get('src_align', 256)) + Arena.room(d, c.get('align', 256))
                      for c, (s, d) in zip(cases, sizes)))
    descs, dsts = [], []
    for c, (s, d) in zip(cases, sizes):
        src, (h, w) = c['src'], c['hw']
        src_at = arena.put(src, c.get('src_align', 256), c.get('src_misalign', 0))
        dst_at = arena.take(d, c.get('align', 256), c.get('misalign', 0))
        dsts.append(dst_at)
        _, H, W, channels = src.shape
        consts = {}
        if c.get('mode', MOVE) != MOVE:
            consts = {'mean': tuple(c['mean']) + (0.0,) * (3 - len(c['mean'])),
                      'std': tuple(c['std']) + (1.0,) * (3 - len(c['std'])),
                      'raw_depth': int(c.get('raw_depth', 0)), 'invalid': c.get('invalid', 0.0)}
        descs.append(augment_desc(src_at, dst_at, B, H, W, channels, h, w, c.get('mode', MOVE),
                                  src.dtype.itemsize.bit_length() - 1, **consts))
    words = launch_augment(descs, table, tail)
    outs = []
    for i, (c, (s, d)) in enumerate(zip(cases, sizes)):
        src, (h, w) = c['src'], c['hw']
        mode = c.get('mode', MOVE)
        want = augment_reference(src, table, (h, w), mode, c.get('mean'), c.get('std'), c.get('raw_depth', 0),
                                 c.get('invalid', 0.0))
        got = arena.read(dsts[i], d)
        assert want.nbytes == d
        outs.append(got.view(want.dtype).reshape(want.shape))
        if not np.array_equal(got, raw_bytes(want)):
            wrong = np.flatnonzero(got.view(want.dtype.str.replace('f', 'u')) != raw_bytes(want).view(want.dtype.str.replace('f', 'u')))
            raise AssertionError(f'descriptor {i} of {len(cases)} ({src.dtype} {src.shape} -> {want.shape}, mode {mode}, '
                                 f'pixels_per_lane {words[i, A_PPL]}): {wrong.size} of {want.size} elements differ, '
                                 f'first at {np.unravel_index(wrong[:4], want.shape)}')
        # the fields the call does not own came back as they went in
        kept = [k for k in range(AUG_WORDS) if k not in (A_BLOCK_BEGIN, A_PPL)]
        assert np.array_equal(words[i, kept], descs[i][kept])
    arena.check_guards()
    arena.check_sources()
    return words, outs


def run_multiscale(cases, tail=(), shared_maps=None):
    """One launch of `cases`, each a dict: src [planes,H,W] array, rows, cols, and optionally
    align / misalign of the destination.  Without `shared_maps` every case's maps are appended in
    turn; with it (an int32 array) each case names `row_map` / `col_map` offsets into it, and its
    rows / cols are read from there.  Every output is compared with `multiscale_reference` as
    bytes, the guards and the sources are checked.  -> (words read back [n,16], outputs)"""
    maps, offsets = ([], []) if shared_maps is None else (np.asarray(shared_maps, np.int32), None)
    if shared_maps is None:
        at = 0
        for c in cases:
            rows, cols = np.asarray(c['rows'], np.int32), np.asarray(c['cols'], np.int32)
            offsets.append((at, at + len(rows)))
            maps += [rows, cols]
            at += len(rows) + len(cols)
        maps = np.concatenate(maps)
    else:
        offsets = [(c['row_map'], c['col_map']) for c in cases]
        for c in cases:
            c['rows'] = maps[c['row_map']:c['row_map'] + c['h']]
            c['cols'] = maps[c['col_map']:c['col_map'] + c['w']]
            assert len(c['rows']) == c['h'] and len(c['cols']) == c['w']
    sizes = [(c['src'].nbytes, c['src'].shape[0] * len(c['rows']) * len(c['cols']) * c['src'].dtype.itemsize) for c in cases]
    arena = Arena(sum(Arena.room(s, c.get('src_align', 256)) + Arena.room(d, c.get('align', 256))
                      for c, (s, d) in zip(cases, sizes)))
    descs, dsts = [], []
    for c, (s, d), (row_map, col_map) in zip(cases, sizes, offsets):
        src = c['src']
        assert src.ndim == 3
        src_at = arena.put(src, c.get('src_align', 256), c.get('src_misalign', 0))
        dst_at = arena.take(d, c.get('align', 256), c.get('misalign', 0))
        dsts.append(dst_at)
        descs.append(multiscale_desc(src_at, dst_at, src.shape[0], src.shape[1], src.shape[2], len(c['rows']),
                                     len(c['cols']), src.dtype.itemsize.bit_length() - 1, row_map, col_map))
    words = launch_multiscale(descs, maps, tail)
    outs = []
    for i, (c, (s, d)) in enumerate(zip(cases, sizes)):
        want = multiscale_reference(c['src'], c['rows'], c['cols'])
        got = arena.read(dsts[i], d)
        assert want.nbytes == d
        outs.append(got.view(want.dtype).reshape(want.shape))
        if not np.array_equal(got, raw_bytes(want)):
            wrong = np.flatnonzero(outs[-1].reshape(-1) != want.reshape(-1))
            raise AssertionError(f'descriptor {i} of {len(cases)} ({c["src"].dtype} {c["src"].shape} -> {want.shape}): '
                                 f'{wrong.size} of {want.size} elements differ, first at '
                                 f'{np.unravel_index(wrong[:4], want.shape)}')
        kept = [k for k in range(MS_WORDS) if k != M_BLOCK_BEGIN]
        assert np.array_equal(words[i, kept], descs[i][kept])
    arena.check_guards()
    arena.check_sources()
    return words, outs


def block_prefix(items, threads=256):
    """exclusive prefix of ceil(items / threads)"""
    blocks = [-(-int(n) // threads) for n in items]
    return [int(sum(blocks[:i])) for i in range(len(blocks))]
