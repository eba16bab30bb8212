"""
Functional front-end of the HIP hot path: torch device tensors in, torch device
tensors out, every call stream-ordered on torch's current HIP stream, no host
synchronisation.  These are thin argument marshallers over include/nmsa.h; the
reference-shaped classes (model/postprocessing, utils/panoptic_merge, metric,
loss) are built on top of them.
"""
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

DEFAULT_MAX_CENTERS = 256

# persistent, always-zero vote tables (one per device / shape): nmsa_panoptic_assign clears
# the rows it read, so the next step needs no memset.  Keyed by stream as well, so that
# concurrent pipelines on different streams never share a table.
# At most _VOTE_TABLES_MAX tables are kept (least recently used first out): a ragged last batch
# or short-lived streams must not leave a table behind each.  A dropped table is freed through
# torch's allocator, stream-ordered behind the kernels that used it; a table that a captured
# hipGraph holds stays alive through the graph's private pool.
_VOTE_TABLES: 'collections.OrderedDict[tuple, torch.Tensor]' = __import__('collections').OrderedDict()
_VOTE_TABLES_MAX = 8


def _vote_table(dev: torch.device, B: int, n_cols: int) -> torch.Tensor:
    key = (dev, B, n_cols, torch.cuda.current_stream(dev).cuda_stream)
    t = _VOTE_TABLES.get(key)
    if t is None:
        t = torch.zeros((B, 256, n_cols), dtype=torch.int32, device=dev)
        _VOTE_TABLES[key] = t
        while len(_VOTE_TABLES) > _VOTE_TABLES_MAX:
            _VOTE_TABLES.popitem(last=False)
    else:
        _VOTE_TABLES.move_to_end(key)
    return t


def _u8(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """bool / uint8 tensor viewed as uint8 (torch.bool storage is one byte)."""
    if t is None:
        return None
    if t.dtype == torch.bool:
        return t.contiguous().view(torch.uint8)
    if t.dtype == torch.uint8:
        return t.contiguous()
    return (t != 0).contiguous().view(torch.uint8)


# ----------------------------------------------------------------------------- a2
def center_nms_topk(
    center_heatmap: torch.Tensor,
    foreground_mask: Optional[torch.Tensor] = None,
    threshold: float = 0.1,
    kernel_size: int = 3,
    top_k: int = 64,
    apply_foreground_mask: bool = False,
    max_centers: int = DEFAULT_MAX_CENTERS,
    want_mask: bool = False,
) -> Dict[str, torch.Tensor]:
    """reference: InstancePostprocessing._get_instance_centers (instance.py:79-168)"""
    c = L.require_device_tensor(center_heatmap, 'center_heatmap')
    if c.dtype != torch.float32:
        c = c.float()
    if c.ndim == 4:
        assert c.shape[1] == 1
        c = c[:, 0]
    c = c.contiguous()
    B, H, W = c.shape
    dev = c.device
    fg = _u8(foreground_mask) if apply_foreground_mask else None
    cyx = torch.empty((B, max_centers, 2), dtype=torch.int32, device=dev)
    n = torch.empty((B,), dtype=torch.int32, device=dev)
    scores = torch.empty((B, max_centers), dtype=torch.float32, device=dev)
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if want_mask else None
    ws_bytes = L.lib().nmsa_center_nms_workspace_bytes(B, H, W)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    L.check(L.lib().nmsa_center_nms_topk(
        L.ptr(c), L.ptr(fg), B, H, W, float(threshold), int(kernel_size), int(top_k),
        int(bool(apply_foreground_mask)), int(max_centers),
        L.ptr(cyx), L.ptr(n), L.ptr(scores), L.ptr(mask), L.ptr(ws), ws_bytes,
        L.stream_ptr(dev)), 'nmsa_center_nms_topk')
    out = {'centers_yx': cyx, 'n_centers': n, 'scores': scores}
    if want_mask:
        out['center_mask'] = mask.view(torch.bool)
    return out


# ----------------------------------------------------------------------------- a3
def group_offsets(
    center_offset: torch.Tensor,
    foreground_mask: torch.Tensor,
    centers_yx: torch.Tensor,
    n_centers: torch.Tensor,
    scale_y: float = 1.0,
    scale_x: float = 1.0,
    distance_threshold: Optional[float] = None,
    want_area: bool = True,
) -> Dict[str, torch.Tensor]:
    """reference: InstancePostprocessing._get_instance_segmentation (instance.py:187-253)"""
    off = L.require_device_tensor(center_offset, 'center_offset')
    if off.dtype != torch.float32:
        off = off.float()
    B, two, H, W = off.shape
    assert two == 2
    dev = off.device
    fg = _u8(foreground_mask)
    inst = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    area = torch.empty((B, 256), dtype=torch.int32, device=dev) if want_area else None
    L.check(L.lib().nmsa_group_offsets(
        L.ptr(off), L.ptr(fg), L.ptr(centers_yx), L.ptr(n_centers), B, H, W,
        int(centers_yx.shape[1]), float(scale_y), float(scale_x),
        0 if distance_threshold is None else 1,
        0.0 if distance_threshold is None else float(distance_threshold),
        L.ptr(inst), L.ptr(area), L.stream_ptr(dev)), 'nmsa_group_offsets')
    return {'instance': inst, 'area': area}


# ----------------------------------------------------------------------------- f2
NMSA_ELEM_F32 = 8


def _crop_geometry(t: torch.Tensor, crop) -> Tuple[int, int, int, int, int, int]:
    Hs, Ws = int(t.shape[-2]), int(t.shape[-1])
    if crop is None:
        return Hs, Ws, 0, 0, Hs, Ws
    sl_h, sl_w = crop
    y0, y1, st_y = sl_h.indices(Hs)
    x0, x1, st_x = sl_w.indices(Ws)
    if st_y != 1 or st_x != 1 or y1 <= y0 or x1 <= x0:
        raise ValueError(f'unsupported valid-region slices {crop}')
    return Hs, Ws, y0, x0, y1 - y0, x1 - x0


def resize_nearest(maps: torch.Tensor, size: Tuple[int, int], crop=None) -> torch.Tensor:
    """crop `maps[..., crop]` and F.interpolate(mode='nearest') to `size`, bit-identical to the
    reference's `_crop_to_valid_region_and_resize_prediction` (dense_base.py:15-58),
    including its float32 round trip for int32 / int64 maps."""
    x = L.require_device_tensor(maps, 'maps')
    code = NMSA_ELEM_F32 if x.dtype == torch.float32 else L.int_dtype_code(x)
    Hs, Ws, y0, x0, h, w = _crop_geometry(x, crop)
    Ho, Wo = int(size[0]), int(size[1])
    planes = x.numel() // (Hs * Ws)
    out = torch.empty(tuple(x.shape[:-2]) + (Ho, Wo), dtype=x.dtype, device=x.device)
    L.check(L.lib().nmsa_resize_nearest(
        L.ptr(x), code, planes, Hs, Ws, y0, x0, h, w, Ho, Wo, L.ptr(out),
        L.stream_ptr(x.device)), 'nmsa_resize_nearest')
    return out


def resize_bilinear(maps: torch.Tensor, size: Tuple[int, int], crop=None) -> torch.Tensor:
    """crop + F.interpolate(mode='bilinear', align_corners=False) (dense_base.py:15-58)."""
    x = L.require_device_tensor(maps, 'maps')
    Hs, Ws, y0, x0, h, w = _crop_geometry(x, crop)
    Ho, Wo = int(size[0]), int(size[1])
    planes = x.numel() // (Hs * Ws)
    out = torch.empty(tuple(x.shape[:-2]) + (Ho, Wo), dtype=x.dtype, device=x.device)
    L.check(L.lib().nmsa_resize_bilinear(
        L.ptr(x), L.float_dtype_code(x), planes, Hs, Ws, y0, x0, h, w, Ho, Wo, L.ptr(out),
        L.stream_ptr(x.device)), 'nmsa_resize_bilinear')
    return out


def semantic_argmax_resized(
    logits: torch.Tensor,
    size: Tuple[int, int],
    crop=None,
    want_u8: bool = False,
    want_i64: bool = True,
    want_score: bool = True,
) -> Dict[str, torch.Tensor]:
    """reference: semantic.py:61-80 — crop + bilinear resize + softmax + max at the dataset
    resolution, in one pass over the network-resolution logits."""
    x = L.require_device_tensor(logits, 'logits')
    B, Cn = int(x.shape[0]), int(x.shape[1])
    Hs, Ws, y0, x0, h, w = _crop_geometry(x, crop)
    Ho, Wo = int(size[0]), int(size[1])
    dev = x.device
    u8 = torch.empty((B, Ho, Wo), dtype=torch.uint8, device=dev) if want_u8 else None
    i64 = torch.empty((B, Ho, Wo), dtype=torch.int64, device=dev) if want_i64 else None
    sc = torch.empty((B, Ho, Wo), dtype=torch.float32, device=dev) if want_score else None
    L.check(L.lib().nmsa_semantic_argmax_resized(
        L.ptr(x), L.float_dtype_code(x), B, Cn, Hs, Ws, y0, x0, h, w, Ho, Wo,
        L.ptr(u8), L.ptr(i64), L.ptr(sc), L.stream_ptr(dev)), 'nmsa_semantic_argmax_resized')
    return {'idx_u8': u8, 'idx': i64, 'score': sc}


# ----------------------------------------------------------------------------- a1
def semantic_argmax(
    logits: torch.Tensor,
    want_u8: bool = False,
    want_i64: bool = True,
    want_score: bool = True,
) -> Dict[str, torch.Tensor]:
    """reference: SemanticPostprocessing._postprocess_inference (semantic.py:52-53)"""
    x = L.require_device_tensor(logits, 'logits')
    B, Cn, H, W = x.shape
    dev = x.device
    u8 = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if want_u8 else None
    i64 = torch.empty((B, H, W), dtype=torch.int64, device=dev) if want_i64 else None
    sc = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_score else None
    L.check(L.lib().nmsa_semantic_argmax(
        L.ptr(x), L.float_dtype_code(x), B, Cn, H, W, L.ptr(u8), L.ptr(i64), L.ptr(sc),
        L.stream_ptr(dev)), 'nmsa_semantic_argmax')
    return {'idx_u8': u8, 'idx': i64, 'score': sc}


def semantic_softmax(logits: torch.Tensor) -> torch.Tensor:
    """reference: F.softmax(output, dim=1) (semantic.py:52)"""
    x = L.require_device_tensor(logits, 'logits')
    B, Cn, H, W = x.shape
    probs = torch.empty((B, Cn, H, W), dtype=torch.float32, device=x.device)
    L.check(L.lib().nmsa_semantic_softmax(
        L.ptr(x), L.float_dtype_code(x), B, Cn, H, W, L.ptr(probs),
        L.stream_ptr(x.device)), 'nmsa_semantic_softmax')
    return probs


# ------------------------------------------------------------------ a1+a3+a4+a5
def panoptic_pipeline(
    semantic_logits: torch.Tensor,
    center_heatmap: torch.Tensor,
    center_offset: torch.Tensor,
    is_thing: torch.Tensor,                 # u8/bool [C], on device
    threshold: float = 0.1,
    kernel_size: int = 3,
    top_k: int = 64,
    apply_foreground_mask: bool = False,
    normalized_offset: bool = True,
    distance_threshold: Optional[float] = None,
    max_instances_per_category: int = 1 << 16,
    void_label: int = 0,
    max_centers: int = DEFAULT_MAX_CENTERS,
    want_score: bool = False,
    want_foreground: bool = True,
    want_panoptic_semantic: bool = False,
    fused_kernel_events: Optional[list] = None,
    on_centers=None,
) -> Dict[str, torch.Tensor]:
    """center-NMS -> fused argmax/grouping/votes -> assign -> paint.

    `on_centers`: called with the center tables right after the top-k selection is queued (the
    postprocessing API starts the asynchronous copy of the center counts there, so that its
    overflow check never waits for the streaming kernels behind it).

    `fused_kernel_events`: if a list is given, a (start, end) pair of HIP events
    recorded on the launch stream around the dominant kernel is appended
    (bench.py's live roofline measurement).

    reference: PanopticPostprocessing._postprocess_inference (panoptic.py:77-168).
    When the foreground-masked heatmap option is on, the foreground depends on
    the semantic argmax, so the argmax runs first as its own kernel.
    """
    lib = L.lib()
    x = L.require_device_tensor(semantic_logits, 'semantic_logits')
    off = L.require_device_tensor(center_offset, 'center_offset')
    if off.dtype != torch.float32:
        off = off.float()
    B, Cn, H, W = x.shape
    dev = x.device
    st = L.stream_ptr(dev)
    thing = _u8(is_thing)

    fg_for_nms = None
    if apply_foreground_mask:
        pre = semantic_argmax(x, want_u8=True, want_i64=False, want_score=False)
        fg_for_nms = thing[pre['idx_u8'].long()]
    cen = center_nms_topk(center_heatmap, fg_for_nms, threshold, kernel_size, top_k,
                          apply_foreground_mask, max_centers)
    if on_centers is not None:
        on_centers(cen)

    sem_u8 = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    inst = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    fg = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if want_foreground else None
    score = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_score else None
    votes = _vote_table(dev, B, Cn + 1)
    vote_key = (dev, B, Cn + 1, torch.cuda.current_stream(dev).cuda_stream)
    sy, sx = (float(H), float(W)) if normalized_offset else (1.0, 1.0)
    if fused_kernel_events is not None:
        ev0 = torch.cuda.Event(enable_timing=True)
        ev1 = torch.cuda.Event(enable_timing=True)
        ev0.record(torch.cuda.current_stream(dev))
    L.check(lib.nmsa_panoptic_fused(
        L.ptr(x), L.float_dtype_code(x), L.ptr(off), L.ptr(cen['centers_yx']),
        L.ptr(cen['n_centers']), L.ptr(thing), B, Cn, H, W, int(max_centers), sy, sx,
        0 if distance_threshold is None else 1,
        0.0 if distance_threshold is None else float(distance_threshold),
        L.ptr(sem_u8), L.ptr(inst), L.ptr(fg), L.ptr(score), L.ptr(votes), 1,
        int(top_k) + 1, st), 'nmsa_panoptic_fused')
    if fused_kernel_events is not None:
        ev1.record(torch.cuda.current_stream(dev))
        fused_kernel_events.append((ev0, ev1))

    pan_of_inst = torch.empty((B, 256), dtype=torch.int64, device=dev)
    area = torch.empty((B, 256), dtype=torch.int32, device=dev)
    ids_pan = torch.empty((B, 256), dtype=torch.int64, device=dev)
    ids_ins = torch.empty((B, 256), dtype=torch.int64, device=dev)
    n_ids = torch.empty((B,), dtype=torch.int32, device=dev)
    try:
        L.check(lib.nmsa_panoptic_assign(
            L.ptr(votes), B, Cn + 1, 1, int(max_instances_per_category), int(void_label),
            L.ptr(pan_of_inst), L.ptr(area), L.ptr(ids_pan), L.ptr(ids_ins), L.ptr(n_ids), st),
            'nmsa_panoptic_assign')
    except Exception:
        _VOTE_TABLES.pop(vote_key, None)          # the table was written but not cleared
        raise

    pan = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    pan_sem = torch.empty((B, H, W), dtype=torch.int64, device=dev) \
        if want_panoptic_semantic else None
    L.check(lib.nmsa_panoptic_paint(
        L.ptr(sem_u8), L.ptr(inst), L.ptr(pan_of_inst), L.ptr(thing), B, Cn, H, W,
        int(max_instances_per_category), int(void_label), L.ptr(pan), L.ptr(pan_sem), st),
        'nmsa_panoptic_paint')

    return {
        'semantic_idx_u8': sem_u8, 'semantic_score': score,
        'foreground': None if fg is None else fg.view(torch.bool),
        'instance': inst, 'panoptic': pan, 'panoptic_semantic': pan_sem,
        'centers_yx': cen['centers_yx'], 'n_centers': cen['n_centers'],
        'center_scores': cen['scores'], 'area': area,
        'ids_pan': ids_pan, 'ids_ins': ids_ins, 'n_ids': n_ids,
        'pan_of_inst': pan_of_inst,
    }


# ----------------------------------------------------------------------------- f3
def panoptic_scores(
    logits: torch.Tensor,
    semantic_idx_u8: torch.Tensor,
    semantic_prob: torch.Tensor,
    instance: torch.Tensor,
    panoptic: torch.Tensor,
    pan_of_inst: torch.Tensor,
    instance_score_table: torch.Tensor,
    max_instances_per_category: int,
) -> Dict[str, torch.Tensor]:
    """reference: the `compute_scores` branch of PanopticPostprocessing (panoptic.py:171-239)"""
    x = L.require_device_tensor(logits, 'logits')
    B, Cn, H, W = x.shape
    dev = x.device
    sem = L.require_device_tensor(semantic_idx_u8, 'semantic_idx_u8')
    prob = L.require_device_tensor(semantic_prob, 'semantic_prob')
    ins = L.require_device_tensor(instance, 'instance')
    pan = L.require_device_tensor(panoptic, 'panoptic')
    poi = L.require_device_tensor(pan_of_inst, 'pan_of_inst')
    tab = L.require_device_tensor(instance_score_table, 'instance_score_table')
    assert sem.dtype == torch.uint8 and ins.dtype == torch.uint8 and pan.dtype == torch.int64
    assert prob.dtype == torch.float32 and tab.dtype == torch.float32 and poi.dtype == torch.int64
    assert tuple(tab.shape) == (B, 256) and tuple(poi.shape) == (B, 256)
    out = [torch.empty((B, H, W), dtype=torch.float32, device=dev) for _ in range(3)]
    mean = torch.empty((B, 256), dtype=torch.float32, device=dev)
    ws_bytes = L.lib().nmsa_panoptic_scores_workspace_bytes(B)
    ws = torch.empty((ws_bytes // 8,), dtype=torch.float64, device=dev)
    L.check(L.lib().nmsa_panoptic_scores(
        L.ptr(x), L.float_dtype_code(x), L.ptr(sem), L.ptr(prob), L.ptr(ins), L.ptr(pan),
        L.ptr(poi), L.ptr(tab), B, Cn, H, W, int(max_instances_per_category),
        L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), L.ptr(mean), L.ptr(ws), ws_bytes,
        L.stream_ptr(dev)), 'nmsa_panoptic_scores')
    return {'semantic_score': out[0], 'instance_score': out[1], 'panoptic_score': out[2],
            'mean_semantic_score': mean}


# ----------------------------------------------------------------------------- f4
_GAUSS_LUTS: Dict[tuple, torch.Tensor] = {}


def _gauss_lut(sigma: int, dev: torch.device) -> torch.Tensor:
    """heat-map value by integer squared distance: the entries of the reference's precomputed
    (6s+3)^2 patch (data/preprocessing/instance.py:147-154), same numpy float64 exp, rounded to
    float32 exactly like `np.maximum(center_img, gauss)` stored into the float32 image does."""
    key = (int(sigma), dev)
    if key not in _GAUSS_LUTS:
        import numpy as np
        r = 3 * int(sigma) + 1
        d2 = np.arange(2 * r * r + 1, dtype=np.float64)
        lut = np.exp(-d2 / (2 * int(sigma) ** 2)).astype(np.float32)
        _GAUSS_LUTS[key] = torch.from_numpy(lut).to(dev)
    return _GAUSS_LUTS[key]


# Persistent workspaces of the target generators, one per (device, stream, B, classes,
# max_instances): on the on-wire layout a call leaves its hash tables zeroed, so the next call on
# the same workspace skips the memset (`workspace_is_clean`).  LRU of 4.  A hipGraph captured on a
# stream that has no workspace yet makes one inside the capture and zeroes it on every replay (a
# kernel in csrc/targets.hip, tg_zero: a captured hipMemsetAsync was not redone on later replays).
_TARGET_WORKSPACES: 'collections.OrderedDict[tuple, list]' = __import__('collections').OrderedDict()


def _targets_workspace(B: int, n_classes: int, max_instances: int, dev, reusable: bool = False):
    """(workspace, bytes, entry): entry = [tensor, clean]; `clean` = this workspace was last used
    by a target-generator call on the on-wire layout that was enqueued successfully, and may skip
    its memset (the caller sets entry[1] = 1 after its own call went through)"""
    nbytes = L.lib().nmsa_targets_workspace_bytes(B, n_classes, max_instances)
    if nbytes == 0:
        raise ValueError('max_instances must be in [1, 4096]')
    if not reusable:
        t = torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=dev)
        return t, nbytes, [t, 0]
    key = (dev, torch.cuda.current_stream(dev).cuda_stream, B, n_classes, max_instances)
    entry = _TARGET_WORKSPACES.get(key)
    if entry is None:
        entry = _TARGET_WORKSPACES[key] = [torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=dev), 0]
        while len(_TARGET_WORKSPACES) > 4:
            _TARGET_WORKSPACES.popitem(last=False)
    else:
        _TARGET_WORKSPACES.move_to_end(key)
    return entry[0], nbytes, entry


def _targets_on_wire(sem: torch.Tensor, ins: torch.Tensor, H: int, W: int, n_classes: int) -> bool:
    """the layouts the one-launch front end of csrc/targets.hip takes (it SETS the status word and
    leaves its workspace clean): the on-wire dtypes, rows of 4 pixels"""
    import os
    return (os.environ.get('NMSA_TG_FUSED', '1') != '0' and sem.dtype == torch.uint8 and
            ins.dtype == torch.int32 and W % 4 == 0 and n_classes <= 16384 and
            sem.data_ptr() % 4 == 0 and ins.data_ptr() % 16 == 0)


def targets_route(semantic: torch.Tensor, instance: torch.Tensor, n_classes: int, sigma: int = 8,
                  max_instances: int = 1024) -> int:
    """The kernels `instance_targets` / `panoptic_targets` / `orientation_targets` run for these
    label maps (`nmsa_targets_route`): a mask of `_lib.NMSA_TG_ROUTE_*` bits.  The outputs and the
    workspace of those calls are fresh torch allocations (256-byte aligned) and go in as NULL,
    which the query counts as aligned; nothing is launched or allocated."""
    sem = L.require_device_tensor(semantic, 'semantic')
    ins = L.require_device_tensor(instance, 'instance')
    B, H, W = sem.shape
    rc = L.lib().nmsa_targets_route(
        L.ptr(sem), L.int_dtype_code(sem), L.ptr(ins), L.int_dtype_code(ins), int(n_classes), H, W,
        int(sigma), int(max_instances), None, None, None, None, None)
    if rc < 0:
        L.check(rc, 'nmsa_targets_route')
    return rc


def instance_clear_stuff(semantic: torch.Tensor, instance: torch.Tensor,
                         is_stuff_class: torch.Tensor) -> torch.Tensor:
    """reference: InstanceClearStuffIDs (data/preprocessing/instance.py:46-93); in place."""
    sem = L.require_device_tensor(semantic, 'semantic')
    if not instance.is_cuda or not instance.is_contiguous():
        raise L.NmsaError('instance must be a contiguous device tensor (modified in place)')
    lut = _u8(is_stuff_class)
    L.check(L.lib().nmsa_instance_clear_stuff(
        L.ptr(sem), L.int_dtype_code(sem), L.ptr(instance), L.int_dtype_code(instance),
        L.ptr(lut), int(lut.numel()), int(sem.numel()), L.stream_ptr(sem.device)),
        'nmsa_instance_clear_stuff')
    return instance


def instance_targets(
    semantic: torch.Tensor,
    instance: torch.Tensor,
    n_classes: int,
    is_thing_class: Optional[torch.Tensor],
    is_stuff_class: Optional[torch.Tensor],
    sigma: int,
    normalized_offset: bool = True,
    max_instances: int = 1024,
) -> Dict[str, torch.Tensor]:
    """reference: InstanceTargetGenerator._preprocess (data/preprocessing/instance.py:157-286)
    for a whole batch [B,H,W]."""
    sem = L.require_device_tensor(semantic, 'semantic')
    ins = L.require_device_tensor(instance, 'instance')
    B, H, W = sem.shape
    dev = sem.device
    th = None if is_thing_class is None else _u8(is_thing_class)
    st = None if is_stuff_class is None else _u8(is_stuff_class)
    cap = ((int(max_instances) + 1023) // 1024) * 1024
    center = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    offset = torch.empty((B, 2, H, W), dtype=torch.float32 if normalized_offset else torch.int16,
                         device=dev)
    fg = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    cm = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    enc = torch.empty((B, cap), dtype=torch.int32, device=dev)
    skp = torch.empty((B, cap), dtype=torch.int32, device=dev)
    n_enc = torch.empty((B,), dtype=torch.int32, device=dev)
    n_skp = torch.empty((B,), dtype=torch.int32, device=dev)
    on_wire = _targets_on_wire(sem, ins, H, W, int(n_classes))
    ws, ws_bytes, ws_entry = _targets_workspace(B, int(n_classes), int(max_instances), dev, reusable=on_wire)
    clean, ws_entry[1] = ws_entry[1], 0
    status = torch.empty((1,), dtype=torch.int32, device=dev) if on_wire else \
        torch.zeros((1,), dtype=torch.int32, device=dev)
    L.check(L.lib().nmsa_instance_targets(
        L.ptr(sem), L.int_dtype_code(sem), L.ptr(ins), L.int_dtype_code(ins), L.ptr(th), L.ptr(st),
        B, int(n_classes), H, W, int(sigma), L.ptr(_gauss_lut(sigma, dev)),
        int(bool(normalized_offset)), int(max_instances),
        L.ptr(center), L.ptr(offset), L.ptr(fg), L.ptr(cm), L.ptr(enc), L.ptr(n_enc),
        L.ptr(skp), L.ptr(n_skp), L.ptr(status), L.ptr(ws), ws_bytes, int(clean), L.stream_ptr(dev)),
        'nmsa_instance_targets')
    ws_entry[1] = int(on_wire)
    return {'center': center, 'offset': offset, 'foreground': fg.view(torch.bool),
            'center_mask': cm.view(torch.bool), 'encoded_ids': enc, 'n_encoded': n_enc,
            'skipped_ids': skp, 'n_skipped': n_skp, 'status': status}


def panoptic_targets(
    semantic: torch.Tensor,
    instance: torch.Tensor,
    n_classes: int,
    is_thing_class: Optional[torch.Tensor],
    max_instances_per_category: int,
    void_label: int = 0,
    max_instances: int = 1024,
    max_segments: int = 2048,
) -> Dict[str, torch.Tensor]:
    """reference: naive_merge_semantic_and_instance_np (utils/panoptic_merge.py:43-107) as
    called by PanopticTargetGenerator (data/preprocessing/panoptic.py:48-85), per batch."""
    sem = L.require_device_tensor(semantic, 'semantic')
    ins = L.require_device_tensor(instance, 'instance')
    B, H, W = sem.shape
    dev = sem.device
    th = None if is_thing_class is None else _u8(is_thing_class)
    pan = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    ids_pan = torch.empty((B, int(max_segments)), dtype=torch.int64, device=dev)
    ids_ins = torch.empty((B, int(max_segments)), dtype=torch.int64, device=dev)
    n_ids = torch.empty((B,), dtype=torch.int32, device=dev)
    on_wire = _targets_on_wire(sem, ins, H, W, int(n_classes))
    ws, ws_bytes, ws_entry = _targets_workspace(B, int(n_classes), int(max_instances), dev, reusable=on_wire)
    clean, ws_entry[1] = ws_entry[1], 0
    status = torch.empty((1,), dtype=torch.int32, device=dev) if on_wire else \
        torch.zeros((1,), dtype=torch.int32, device=dev)
    L.check(L.lib().nmsa_panoptic_targets(
        L.ptr(sem), L.int_dtype_code(sem), L.ptr(ins), L.int_dtype_code(ins), L.ptr(th),
        B, int(n_classes), H, W, int(max_instances_per_category), int(void_label),
        int(max_instances), int(max_segments), L.ptr(pan), L.ptr(ids_pan), L.ptr(ids_ins),
        L.ptr(n_ids), L.ptr(status), L.ptr(ws), ws_bytes, int(clean), L.stream_ptr(dev)),
        'nmsa_panoptic_targets')
    ws_entry[1] = int(on_wire)
    return {'panoptic': pan, 'ids_pan': ids_pan, 'ids_ins': ids_ins, 'n_ids': n_ids,
            'status': status}


def orientation_targets(
    semantic: torch.Tensor,
    instance: torch.Tensor,
    n_classes: int,
    estimate_class: Optional[torch.Tensor],
    keys: torch.Tensor,
    n_keys: torch.Tensor,
    biternion: torch.Tensor,
    max_instances: int = 1024,
) -> Dict[str, torch.Tensor]:
    """reference: OrientationTargetGenerator._preprocess (data/preprocessing/orientation.py:37-97)
    for a whole batch [B,H,W].  `keys` i32 [B,K]: per image the instance ids that have an
    orientation, strictly ascending, the first `n_keys[b]` valid; `biternion` f32 [B,K,2] their
    (cos, sin).  `present` u8 [B,K] flags the keys that were painted."""
    sem = L.require_device_tensor(semantic, 'semantic')
    ins = L.require_device_tensor(instance, 'instance')
    k = L.require_device_tensor(keys, 'keys')
    nk = L.require_device_tensor(n_keys, 'n_keys')
    bit = L.require_device_tensor(biternion, 'biternion')
    B, H, W = sem.shape
    K = int(k.shape[1])
    if k.dtype != torch.int32 or nk.dtype != torch.int32 or bit.dtype != torch.float32:
        raise TypeError('keys / n_keys must be int32 and biternion float32')
    if tuple(k.shape) != (B, K) or tuple(nk.shape) != (B,) or tuple(bit.shape) != (B, K, 2):
        raise ValueError(f'keys [B,K], n_keys [B], biternion [B,K,2] expected for B = {B}, got '
                         f'{tuple(k.shape)}, {tuple(nk.shape)}, {tuple(bit.shape)}')
    dev = sem.device
    est = None if estimate_class is None else _u8(estimate_class)
    ori = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev)
    fg = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    present = torch.empty((B, K), dtype=torch.uint8, device=dev)
    on_wire = _targets_on_wire(sem, ins, H, W, int(n_classes))
    ws, ws_bytes, ws_entry = _targets_workspace(B, int(n_classes), int(max_instances), dev, reusable=on_wire)
    clean, ws_entry[1] = ws_entry[1], 0
    status = torch.empty((1,), dtype=torch.int32, device=dev) if on_wire else \
        torch.zeros((1,), dtype=torch.int32, device=dev)
    L.check(L.lib().nmsa_orientation_targets(
        L.ptr(sem), L.int_dtype_code(sem), L.ptr(ins), L.int_dtype_code(ins), L.ptr(est),
        L.ptr(k), L.ptr(nk), L.ptr(bit), B, int(n_classes), H, W, K, int(max_instances),
        L.ptr(ori), L.ptr(fg), L.ptr(present), L.ptr(status), L.ptr(ws), ws_bytes, int(clean),
        L.stream_ptr(dev)), 'nmsa_orientation_targets')
    ws_entry[1] = int(on_wire)
    return {'orientation': ori, 'foreground': fg.view(torch.bool), 'present': present,
            'status': status}


def dve_targets(
    panoptic: torch.Tensor,
    keys: torch.Tensor,
    n_keys: torch.Tensor,
    embeddings: Optional[torch.Tensor] = None,
    image_embedding: Optional[torch.Tensor] = None,
    diff_factor: float = 0.65,
) -> Dict[str, torch.Tensor]:
    """reference: DenseVisualEmbeddingTargetGenerator (dense_visual_embedding.py:22-93)."""
    pan = L.require_device_tensor(panoptic, 'panoptic')
    k = L.require_device_tensor(keys, 'keys')
    nk = L.require_device_tensor(n_keys, 'n_keys')
    assert pan.dtype == torch.int64 and k.dtype == torch.int64 and nk.dtype == torch.int32
    B, H, W = pan.shape
    K = int(k.shape[1])
    dev = pan.device
    idx = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    lut = None
    D = 0
    emb = img = None
    if embeddings is not None:
        emb = L.require_device_tensor(embeddings, 'embeddings').float()
        img = L.require_device_tensor(image_embedding, 'image_embedding').float()
        D = int(emb.shape[2])
        lut = torch.empty((B, K, D), dtype=torch.float32, device=dev)
    L.check(L.lib().nmsa_dve_targets(
        L.ptr(pan), L.ptr(k), L.ptr(nk), L.ptr(emb), L.ptr(img), float(diff_factor),
        B, K, D, H, W, L.ptr(lut), L.ptr(idx), L.stream_ptr(dev)), 'nmsa_dve_targets')
    return {'indices': idx, 'lut': lut}


def _dve_project_args(emb, weight_a, weight_b):
    """checked arguments of `nmsa_dve_project`: (B, D, H, W), the contiguous map and per head
    (weight, C, freshly allocated logits) or (None, 0, None)"""
    if emb.dtype != torch.float32:
        raise TypeError(f'emb must be float32, got {emb.dtype}')
    if not emb.is_cuda:
        raise L.NmsaError(f'emb is on {emb.device}: the HIP path needs tensors on the MI355X '
                          '(there is no CPU fallback).')
    if emb.ndim != 4:
        raise ValueError(f'emb must be [B, D, H, W], got shape {tuple(emb.shape)}')
    B, D, H, W = (int(n) for n in emb.shape)
    dev = emb.device
    heads = []
    for name, w in (('weight_a', weight_a), ('weight_b', weight_b)):
        if w is None:
            heads.append((None, 0, None))
            continue
        if w.dtype != torch.float32:
            raise TypeError(f'{name} must be float32, got {w.dtype}')
        w = L.require_device_tensor(w, name)
        if w.device != dev:
            raise ValueError(f'{name} is on {w.device}, emb on {dev}')
        if w.ndim == 4 and w.shape[2:] == (1, 1):       # the reference's conv2d weight
            w = w[:, :, 0, 0].contiguous()
        if w.ndim != 2 or int(w.shape[1]) != D or int(w.shape[0]) < 1:
            raise ValueError(f'{name} must be [C, {D}], got shape {tuple(w.shape)}')
        Cn = int(w.shape[0])
        heads.append((w, Cn, torch.empty((B, Cn, H, W), dtype=torch.float32, device=dev)))
    # cold path: a strided map is normalised through a contiguous copy and copied back
    x = emb if emb.is_contiguous() else emb.contiguous()
    return (B, D, H, W), x, heads


def dve_project(
    emb: torch.Tensor,
    weight_a: Optional[torch.Tensor] = None,
    weight_b: Optional[torch.Tensor] = None,
    *,
    generic: bool = False,
) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """reference: DenseVisualEmbeddingPostprocessing (dense_visual_embedding.py:126 + :81) —
    `emb /= emb.norm(dim=1, keepdim=True)` IN PLACE, then `F.conv2d(emb, weight[:, :, None, None])`
    for up to two [C, D] class-embedding matrices, all from one pass over `emb`.  Returns
    (logits_a, logits_b); None for a head that is off.  `generic` selects the plain per-pixel
    kernel on shapes the MFMA kernel would take (tests)."""
    (B, D, H, W), x, heads = _dve_project_args(emb, weight_a, weight_b)
    if x.numel():
        (wa, Ca, la), (wb, Cb, lb) = heads
        L.check(L.lib().nmsa_dve_project(
            L.ptr(x), B, D, H, W, L.ptr(wa), Ca, L.ptr(la), L.ptr(wb), Cb, L.ptr(lb),
            1 if generic else 0, L.stream_ptr(emb.device)), 'nmsa_dve_project')
        if x is not emb:
            emb.copy_(x)
    return heads[0][2], heads[1][2]


def dve_project_route(
    emb: torch.Tensor,
    weight_a: Optional[torch.Tensor] = None,
    weight_b: Optional[torch.Tensor] = None,
    *,
    generic: bool = False,
) -> int:
    """The kernel `dve_project` runs for these arguments (`nmsa_dve_project_route`): 0 for the
    per-pixel kernel, PT * 16 + NT for the MFMA instantiation `<PT, NT>` (131, 67, 70).  The logits
    are allocated as `dve_project` allocates them, so the alignment seen here is the launch's;
    nothing is launched and `emb` is left alone."""
    (B, D, H, W), x, heads = _dve_project_args(emb, weight_a, weight_b)
    (wa, Ca, la), (wb, Cb, lb) = heads
    rc = L.lib().nmsa_dve_project_route(
        L.ptr(x), B, D, H, W, L.ptr(wa), Ca, L.ptr(la), L.ptr(wb), Cb, L.ptr(lb), 1 if generic else 0)
    if rc < 0:
        L.check(rc, 'nmsa_dve_project_route')
    return rc


# ----------------------------------------------------------------------------- multiscale
def cv2_nearest_map(src: int, dst: int) -> np.ndarray:
    """Source index of every destination index of a nearest-neighbour resize of one side from
    `src` to `dst` elements, as OpenCV's `resizeNN` (cv2.INTER_NEAREST) computes it: in double
    arithmetic `ifx = 1 / (dst / src)`, `map[x] = min(floor(x * ifx), src - 1)`.  This is NOT
    `x * src // dst`: src = 116, dst = 14 maps 7 to 57 (x * ifx = 57.99999999999999).  The ONE
    place the rule lives; the device only reads the resulting int32 maps."""
    src, dst = int(src), int(dst)
    if src < 1 or dst < 1:
        raise ValueError(f'side lengths must be positive, got {src} -> {dst}')
    ifx = 1.0 / (dst / src)
    return np.array([min(int(math.floor(x * ifx)), src - 1) for x in range(dst)], dtype=np.int32)


_MS_DESC_WORDS = 16         # sizeof(nmsa_multiscale_desc) / 4
_MS_ALIGN = 256             # every output starts on its own 256 bytes of the one allocation
# Staging of nmsa_multiscale_nearest, one per (device, stream, shape set): pinned host words
# (descriptor table | index maps), their device twin, the event of the last copy out of the pinned
# words, and the layout of the outputs.  The maps and the shape fields are written once; a call
# only fills in the addresses.  LRU of 8.  A call under hipGraph capture takes the staging of an
# earlier eager call out of the cache for good: a replay copies the pinned words again, so they
# are never rewritten and live as long as the process.
_MS_STAGING: 'collections.OrderedDict[tuple, dict]' = __import__('collections').OrderedDict()
_MS_CAPTURED = []


def _ms_build_staging(sig, downscales, hw, dev) -> dict:
    h, w = hw
    shapes = {d: (int(h / d), int(w / d)) for d in downscales}
    maps, map_at, words = [], {}, 0
    for d, (hd, wd) in shapes.items():
        map_at[d] = (words, words + hd)
        maps += [cv2_nearest_map(h, hd), cv2_nearest_map(w, wd)]
        words += hd + wd
    n_desc = len(sig) * len(shapes)
    host = torch.empty((n_desc * _MS_DESC_WORDS + words,), dtype=torch.int32).pin_memory()
    packed = host.numpy()
    packed[:] = 0
    if maps:
        packed[n_desc * _MS_DESC_WORDS:] = np.concatenate(maps)
    table = packed[:n_desc * _MS_DESC_WORDS].reshape(n_desc, _MS_DESC_WORDS)
    outputs, nbytes, i = [], 0, 0
    for d, (hd, wd) in shapes.items():
        for name, shape, dtype in sig:
            size = torch.empty((), dtype=dtype).element_size()
            planes = int(np.prod(shape[:-2], dtype=np.int64))
            table[i, 4:12] = (planes, h, w, hd, wd, size.bit_length() - 1, *map_at[d])
            outputs.append((d, name, shape[:-2] + (hd, wd), dtype, nbytes, planes * hd * wd * size))
            nbytes += -(-planes * hd * wd * size // _MS_ALIGN) * _MS_ALIGN
            i += 1
    # (the address is taken here, once: the buffer was pinned above, and a pinned-memory query
    # has no place in a call that may run under hipGraph capture)
    return {'host': host, 'host_ptr': L.ptr(host), 'addresses': table.view(np.uint64)[:, :2], 'n_desc': n_desc,
            'device': torch.empty_like(host, device=dev), 'event': None, 'outputs': outputs,
            'nbytes': nbytes, 'shapes': shapes}


def multiscale_nearest(tensors: Dict[str, torch.Tensor], downscales: Sequence[int],
                       hw: Tuple[int, int]) -> Dict[int, Dict[str, torch.Tensor]]:
    """reference: MultiscaleSupervisionGenerator._preprocess (multiscale_supervision.py:41-67) ->
    resize() with cv2.INTER_NEAREST (resize.py:95-161), for a whole batch: every tensor [..., H, W]
    of `tensors` at every size (int(H / d), int(W / d)), by ONE launch of nmsa_multiscale_nearest
    behind one asynchronous copy of the descriptor table.  Elements of 1, 2, 4 or 8 bytes move as
    raw bits.  -> {d: {name: tensor [..., int(H / d), int(W / d)]}}; the outputs of one call are
    views of one allocation."""
    h, w = int(hw[0]), int(hw[1])
    downscales = tuple(downscales)
    sig, dev = [], None
    for name, t in tensors.items():
        _require_on_device(t, name)
        if dev is not None and t.device != dev:
            raise ValueError(f'{name} is on {t.device}, the other tensors on {dev}')
        dev = t.device
        if not t.is_contiguous():
            raise ValueError(f'{name} must be contiguous')
        if t.ndim < 3 or tuple(t.shape[-2:]) != (h, w):
            raise ValueError(f'{name} must be [..., {h}, {w}], got shape {tuple(t.shape)}')
        if t.element_size() not in (1, 2, 4, 8) or t.is_complex():
            raise ValueError(f'{name}: elements of 1, 2, 4 or 8 bytes are supported, got {t.dtype}')
        if t.numel() == 0:
            raise ValueError(f'{name} is empty: shape {tuple(t.shape)}')
        sig.append((name, tuple(int(n) for n in t.shape), t.dtype))
    for d in downscales:
        if d <= 0 or int(h / d) == 0 or int(w / d) == 0:
            raise ValueError(f'downscale {d} of {h} x {w} is empty')
    if not sig or not downscales:
        return {d: {} for d in downscales}
    if len(sig) * len(set(downscales)) > 1024:                    # NMSA_MULTISCALE_MAX_DESC
        raise ValueError('more than 1024 (key, scale) pairs in one call')
    capturing = torch.cuda.is_current_stream_capturing()
    shape_set = (dev, h, w, downscales, tuple(sig))
    if capturing:
        # pinned memory cannot be allocated while a stream captures: the capture takes over the
        # staging of an earlier eager call with these shapes (the warm-up run every capture needs
        # anyway; its copy has run: torch.cuda.graph synchronises the device on entry), and
        # later eager calls build their own
        key = next((k for k in _MS_STAGING if k[:-1] == shape_set), None)
        if key is None:
            raise RuntimeError('multiscale_nearest under hipGraph capture: call it once with these '
                               'shapes before the capture (its pinned staging cannot be allocated '
                               'while a stream captures)')
        st = _MS_STAGING.pop(key)
        _MS_CAPTURED.append(st)
    else:
        key = shape_set + (torch.cuda.current_stream(dev).cuda_stream,)
        st = _MS_STAGING.get(key)
        if st is None:
            st = _MS_STAGING[key] = _ms_build_staging(sig, downscales, (h, w), dev)
            while len(_MS_STAGING) > 8:
                _, dropped = _MS_STAGING.popitem(last=False)
                if dropped['event'] is not None:
                    dropped['event'].synchronize()      # its last copy still reads the pinned words
        else:
            _MS_STAGING.move_to_end(key)
            # the copy of the call before reads the pinned words: it must have run (a wait on that
            # one copy, not on the stream: it returns at once unless the device is a whole call behind)
            if st['event'] is not None:
                st['event'].synchronize()
    out = torch.empty((st['nbytes'],), dtype=torch.uint8, device=dev)
    base = out.data_ptr()
    for i, (d, name, shape, dtype, at, nbytes) in enumerate(st['outputs']):
        st['addresses'][i] = (tensors[name].data_ptr(), base + at)
    L.check(L.lib().nmsa_multiscale_nearest(
        st['host_ptr'], L.ptr(st['device']), st['n_desc'], int(st['host'].numel()),
        L.stream_ptr(dev)), 'nmsa_multiscale_nearest')
    if not capturing:
        if st['event'] is None:
            st['event'] = torch.cuda.Event()
        st['event'].record(torch.cuda.current_stream(dev))
    result: Dict[int, Dict[str, torch.Tensor]] = {d: {} for d in st['shapes']}
    for d, name, shape, dtype, at, nbytes in st['outputs']:
        result[d][name] = out[at:at + nbytes].view(dtype).view(shape)
    return result


# ----------------------------------------------------------------------------- batch augmentation
_AUG_DESC_WORDS = 24        # sizeof(nmsa_augment_desc) / 4
_AUG_MODES = {'move': 0, 'rgb_norm': 1, 'depth_norm': 2}
# Staging of nmsa_batch_augment, one per (device, stream, shape set), kept and handed to captures
# exactly as _MS_STAGING above: LRU of 8, a call under hipGraph capture takes the staging of an
# earlier eager call out of the cache for good.
_AUG_STAGING: 'collections.OrderedDict[tuple, AugmentStaging]' = __import__('collections').OrderedDict()
_AUG_CAPTURED = []


def check_augment_params(params, B: int, source_hw: Tuple[int, int], crop_hw: Tuple[int, int]) -> np.ndarray:
    """`params` as the int32 [B,3] table of (y0, x0, flip) per sample, every window inside the
    source and every flip 0 or 1 (the checks of nmsa_batch_augment, with a message)"""
    table = np.asarray(params)
    if table.shape != (B, 3) or table.dtype.kind not in 'iub':
        raise ValueError(f'params must be {B} integer triples (y0, x0, flip), got {table.dtype} {table.shape}')
    table = table.astype(np.int64)
    (H, W), (h, w) = source_hw, crop_hw
    if (table[:, :2] < 0).any() or (table[:, 0] + h > H).any() or (table[:, 1] + w > W).any():
        raise ValueError(f'a crop window of {h} x {w} leaves the {H} x {W} source: {table[:, :2].tolist()}')
    if not np.isin(table[:, 2], (0, 1)).all():
        raise ValueError(f'flip must be 0 or 1, got {table[:, 2].tolist()}')
    return table.astype(np.int32)


class AugmentStaging:
    """Staging of one shape set of `batch_augment`: pinned host words (descriptor table | (y0, x0,
    flip) per sample), their device twin, the event of the last copy out of the pinned words and
    the layout of the outputs.  Shapes, modes and constants are written once; a call fills in the
    addresses and the parameters.  A hipGraph that captured a call re-reads the pinned words at
    every replay: `write_params` puts a new table there for the next replay."""

    def __init__(self, sig, B, source_hw, crop_hw, dev) -> None:
        (H, W), (h, w) = source_hw, crop_hw
        self.B, self.source_hw, self.crop_hw, self.n_desc = B, source_hw, crop_hw, len(sig)
        self.host = torch.empty((self.n_desc * _AUG_DESC_WORDS + self._tail_words(),), dtype=torch.int32).pin_memory()
        packed = self.host.numpy()
        packed[:] = 0
        table = packed[:self.n_desc * _AUG_DESC_WORDS].reshape(self.n_desc, _AUG_DESC_WORDS)
        self._bind_tail(packed[self.n_desc * _AUG_DESC_WORDS:])
        self.outputs, self.nbytes = [], 0
        for i, (name, shape, dtype, mode, consts) in enumerate(sig):
            C = shape[3] if len(shape) == 4 else 1
            size = torch.empty((), dtype=dtype).element_size()
            table[i, 4:12] = (B, H, W, C, h, w, _AUG_MODES[mode], size.bit_length() - 1)
            out_dtype = dtype
            if mode != 'move':
                mean, std, raw_depth, invalid = consts
                out_dtype = torch.float32
                table[i, 12:14] = (L.NMSA_F32, int(raw_depth))
                table[i, 16:16 + C].view(np.float32)[:] = mean
                table[i, 19:19 + C].view(np.float32)[:] = std
                table[i, 22:23].view(np.float32)[:] = invalid
            out_shape = (B, h, w) if len(shape) == 3 and mode == 'move' else (B, C, h, w)
            nbytes = B * C * h * w * torch.empty((), dtype=out_dtype).element_size()
            self.outputs.append((name, out_shape, out_dtype, self.nbytes, nbytes))
            self.nbytes += -(-nbytes // _MS_ALIGN) * _MS_ALIGN
        # (the address is taken here, once: see _ms_build_staging)
        self.host_ptr = L.ptr(self.host)
        self.addresses = table.view(np.uint64)[:, :2]
        self.device = torch.empty_like(self.host, device=dev)
        self.event = None

    def _tail_words(self) -> int:
        return 3 * self.B

    def _bind_tail(self, tail: np.ndarray) -> None:
        self.params = tail.reshape(self.B, 3)

    def write_params(self, params) -> None:
        """(y0, x0, flip) per sample for the next replay of the graph that captured this staging;
        checked here, because a replay does not pass through the entry point's checks again"""
        self.params[:] = check_augment_params(params, self.B, self.source_hw, self.crop_hw)


def _augment_signature(tensors: Dict[str, torch.Tensor], norm: Dict[str, tuple]):
    """the tensors of one augmentation call checked against each other and against `norm`
    -> ([(name, shape, dtype, mode, constants)], device, (B, H, W))"""
    sig, dev, BHW = [], None, None
    for name, t in tensors.items():
        _require_on_device(t, name)
        if dev is not None and t.device != dev:
            raise ValueError(f'{name} is on {t.device}, the other tensors on {dev}')
        dev = t.device
        if not t.is_contiguous():
            raise ValueError(f'{name} must be contiguous')
        if t.ndim not in (3, 4) or t.numel() == 0:
            raise ValueError(f'{name} must be a non-empty [B,H,W] or [B,H,W,C], got shape {tuple(t.shape)}')
        if BHW is not None and tuple(t.shape[:3]) != BHW:
            raise ValueError(f'{name} is {tuple(t.shape[:3])}, the other tensors {BHW}')
        BHW = tuple(int(n) for n in t.shape[:3])
        spec = norm.get(name, ('move',))
        if spec[0] == 'move':
            if t.element_size() not in (1, 2, 4, 8) or t.is_complex():
                raise ValueError(f'{name}: elements of 1, 2, 4 or 8 bytes are supported, got {t.dtype}')
            consts = None
        elif spec[0] == 'rgb_norm':
            if t.dtype != torch.uint8 or t.ndim != 4 or t.shape[3] != 3:
                raise ValueError(f'{name}: rgb_norm takes uint8 [B,H,W,3], got {t.dtype} {tuple(t.shape)}')
            mean, std = (tuple(float(np.float32(v)) for v in vs) for vs in spec[1:3])
            if len(mean) != 3 or len(std) != 3:
                raise ValueError(f'{name}: rgb_norm takes three means and three stds')
            consts = (mean, std, False, 0.0)
        elif spec[0] == 'depth_norm':
            if t.dtype not in (torch.uint16, torch.float32) or t.ndim != 3:
                raise ValueError(f'{name}: depth_norm takes uint16 or float32 [B,H,W], got {t.dtype} {tuple(t.shape)}')
            consts = ((float(np.float32(spec[1])),), (float(np.float32(spec[2])),), bool(spec[3]),
                      float(np.float32(spec[4])))
        else:
            raise ValueError(f'{name}: unknown mode {spec[0]!r}')
        if consts is not None and 0.0 in consts[1]:
            raise ValueError(f'{name}: a std of 0')
        sig.append((name, tuple(int(n) for n in t.shape), t.dtype, spec[0], consts))
    if set(norm) - set(tensors):
        raise KeyError(f'norm names entries that are not in tensors: {sorted(set(norm) - set(tensors))}')
    if len(sig) > 256:                                            # NMSA_AUGMENT_MAX_DESC
        raise ValueError('more than 256 keys in one call')
    return sig, dev, BHW


def _augment_launch(what: str, cache, captured: list, staging_type, tensors, sig, dev, BHW, crop_hw, write, entry):
    """one launch of `entry` for `sig` from the staging of its shape set (LRU of 8 in `cache`, a
    capture's in `captured`); `write(staging)` fills in the call's parameters -> (outputs, staging)"""
    B, H, W = BHW
    h, w = crop_hw
    capturing = torch.cuda.is_current_stream_capturing()
    shape_set = (dev, h, w, tuple(sig))
    if capturing:
        # (why: see multiscale_nearest)
        key = next((k for k in cache if k[:-1] == shape_set), None)
        if key is None:
            raise RuntimeError(f'{what} under hipGraph capture: call it once with these shapes '
                               'before the capture (its pinned staging cannot be allocated while a '
                               'stream captures)')
        st = cache.pop(key)
        captured.append(st)
    else:
        key = shape_set + (torch.cuda.current_stream(dev).cuda_stream,)
        st = cache.get(key)
        if st is None:
            st = cache[key] = staging_type(sig, B, (H, W), (h, w), dev)
            while len(cache) > 8:
                _, dropped = cache.popitem(last=False)
                if dropped.event is not None:
                    dropped.event.synchronize()         # its last copy still reads the pinned words
        else:
            cache.move_to_end(key)
            if st.event is not None:
                st.event.synchronize()                  # the copy of the call before has run
    out = torch.empty((st.nbytes,), dtype=torch.uint8, device=dev)
    base = out.data_ptr()
    for i, (name, shape, dtype, at, nbytes) in enumerate(st.outputs):
        st.addresses[i] = (tensors[name].data_ptr(), base + at)
    write(st)
    L.check(entry(st.host_ptr, L.ptr(st.device), st.n_desc, B, int(st.host.numel()), L.stream_ptr(dev)), 'nmsa_' + what)
    if not capturing:
        if st.event is None:
            st.event = torch.cuda.Event()
        st.event.record(torch.cuda.current_stream(dev))
    return {name: out[at:at + nbytes].view(dtype).view(shape) for name, shape, dtype, at, nbytes in st.outputs}, st


def batch_augment(tensors: Dict[str, torch.Tensor], params, crop_hw: Tuple[int, int],
                  norm: Optional[Dict[str, tuple]] = None, return_staging: bool = False):
    """reference: RandomCrop (crop.py:57-73) -> RandomHorizontalFlip (flip.py:40-47) ->
    NormalizeRGB / NormalizeDepth (normalize.py) -> ToTorchTensors (torch.py:31-38), for a whole
    collated batch by ONE launch of nmsa_batch_augment behind one asynchronous copy of the
    descriptor table.  `tensors`: contiguous [B,H,W] or channels-last [B,H,W,C] device tensors of
    one B, H, W.  `params`: integer [B,3], (y0, x0, flip) per sample.  `norm[name]` is
    ('rgb_norm', mean[3], std[3]) for a uint8 [B,H,W,3] entry or ('depth_norm', mean, std,
    raw_depth, invalid_depth_value) for a uint16 / float32 [B,H,W] entry; the constants are used as
    float32.  Every other entry moves as raw bits of 1, 2, 4 or 8 bytes.  -> {name: [B,h,w] for
    [B,H,W], [B,C,h,w] for [B,H,W,C], float32 [B,3,h,w] / [B,1,h,w] for the normalised entries};
    the outputs of one call are views of one allocation.  With `return_staging` the
    `AugmentStaging` used comes back as well (under capture: the one the graph keeps reading)."""
    h, w = int(crop_hw[0]), int(crop_hw[1])
    sig, dev, BHW = _augment_signature(tensors, norm or {})
    if not sig:
        return ({}, None) if return_staging else {}
    B, H, W = BHW
    if h <= 0 or w <= 0 or h > H or w > W:
        raise ValueError(f'a crop of {h} x {w} does not fit the {H} x {W} source')
    table = check_augment_params(params, B, (H, W), (h, w))

    def write(st):
        st.params[:] = table
    result, st = _augment_launch('batch_augment', _AUG_STAGING, _AUG_CAPTURED, AugmentStaging, tensors, sig, dev,
                                 BHW, (h, w), write, L.lib().nmsa_batch_augment)
    return (result, st) if return_staging else result


# ----------------------------------------------------------------------------- batch augmentation behind a resize
# OpenCV's resize rules for ONE side of an image, evaluated for a window of destination indices of
# several samples at once.  cv2_nearest_map above, cv2_nearest_map_vec and cv2_linear_taps below are
# the ONLY places these rules live in the package; the device reads tables.  Both rules are written
# down from OpenCV's source and have NOT been compared with a real cv2 build (none is installed
# where this project is developed); a later comparison touches these functions and the stand-in of
# tools/gen_golden_augment_resize.py, and nothing else.
_CV2_COEF_ONE = 2048        # INTER_RESIZE_COEF_SCALE: the 8-bit linear path's weights are 11-bit fixed point


def _window_positions(start, n: int) -> np.ndarray:
    """f64 [B, n]: the destination indices start[b] .. start[b] + n"""
    return np.asarray(start, np.float64)[:, None] + np.arange(n, dtype=np.float64)


def _cv2_nearest_window(src: int, dst, at: np.ndarray) -> np.ndarray:
    """i32 [B, n]: entries at[b] (`_window_positions`, left as they are) of cv2_nearest_map(src, dst[b])"""
    ifx = 1.0 / (np.asarray(dst, np.float64)[:, None] / float(src))
    x = at * ifx
    return np.minimum(np.floor(x, out=x), src - 1, out=x).astype(np.int32)


def _cv2_linear_window(src: int, dst, at: np.ndarray):
    """(i0, i1 i32 [B, n], a0, a1 i16 [B, n]): entries at[b] of cv2_linear_taps(src, dst[b])"""
    scale = 1.0 / (np.asarray(dst, np.float64)[:, None] / float(src))
    d = at + 0.5
    d *= scale
    d -= 0.5
    f = d.astype(np.float32)
    floor = np.floor(f)
    f -= floor                                                    # float32, as OpenCV's `fx -= sx`
    s = floor.astype(np.int32)
    f[(s < 0) | (s >= src - 1)] = 0
    np.clip(s, 0, src - 1, out=s)
    a1 = np.rint(f * np.float32(_CV2_COEF_ONE)).astype(np.int16)
    np.subtract(np.float32(1.0), f, out=f)
    f *= np.float32(_CV2_COEF_ONE)
    return s, np.minimum(s + 1, src - 1), np.rint(f, out=f).astype(np.int16), a1


def _check_sides(src: int, dst: int) -> Tuple[int, int]:
    src, dst = int(src), int(dst)
    if src < 1 or dst < 1:
        raise ValueError(f'side lengths must be positive, got {src} -> {dst}')
    return src, dst


def cv2_nearest_map_vec(src: int, dst: int) -> np.ndarray:
    """`cv2_nearest_map(src, dst)` without the Python loop (the same double arithmetic in numpy)"""
    src, dst = _check_sides(src, dst)
    return _cv2_nearest_window(src, [dst], _window_positions([0], dst))[0]


def cv2_linear_taps(src: int, dst: int):
    """Taps of a bilinear resize (cv2.INTER_LINEAR) of one side of a uint8 image from `src` to
    `dst` elements, as OpenCV's generic 8-bit path computes them -> (i0, i1, a0, a1): per
    destination index d the two source indices (int32) and their weights of 2048 (int16).
      scale = 1 / (dst / src) in double; f = float32((d + 0.5) * scale - 0.5); s = floor(f);
      f -= s in float32; s < 0: f = 0, s = 0; s >= src - 1: f = 0, s = src - 1;
      i0 = s, i1 = min(s + 1, src - 1), a0 = rint((1 - f) * 2048), a1 = rint(f * 2048)
    A pixel is R = S[i0] * a0 + S[i1] * a1 along a row, then with the row taps (b0, b1)
    (((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16) + 2) >> 2.  At dst == src this is the
    image itself and at an exact 2:1 downscale (a + b + c + d + 2) >> 2, which is what OpenCV's
    area path computes where it takes over INTER_LINEAR.  Written down from OpenCV's source, NOT
    compared with a real cv2 build."""
    src, dst = _check_sides(src, dst)
    return tuple(a[0] for a in _cv2_linear_window(src, [dst], _window_positions([0], dst)))


def check_augment_resize_params(params, B: int, crop_hw: Tuple[int, int]) -> np.ndarray:
    """`params` as the int32 [B,5] table of (y0, x0, flip, rh, rw) per sample: resized sizes of at
    least 1, every crop window inside its sample's resized image, every flip 0 or 1"""
    table = np.asarray(params)
    if table.shape != (B, 5) or table.dtype.kind not in 'iub':
        raise ValueError(f'params must be {B} integer rows (y0, x0, flip, rh, rw), got {table.dtype} {table.shape}')
    table = table.astype(np.int64)
    h, w = crop_hw
    if (table[:, 3:] < 1).any() or (table[:, 3:] > 0x7fffffff).any():
        raise ValueError(f'resized sizes must be at least 1 (and below 2^31): {table[:, 3:].tolist()}')
    if (table[:, :2] < 0).any() or (table[:, 0] + h > table[:, 3]).any() or (table[:, 1] + w > table[:, 4]).any():
        raise ValueError(f'a crop window of {h} x {w} leaves its resized image: {table.tolist()}')
    if not np.isin(table[:, 2], (0, 1)).all():
        raise ValueError(f'flip must be 0 or 1, got {table[:, 2].tolist()}')
    return table.astype(np.int32)


def augment_window_tables(params, source_hw: Tuple[int, int], crop_hw: Tuple[int, int], check: bool = True):
    """The tables nmsa_batch_augment_resized reads, for the [B,5] table (y0, x0, flip, rh, rw):
    per sample the crop window [y0, y0 + h) x [x0, x0 + w) of the image resized from `source_hw`
    to (rh, rw), in OUTPUT coordinates — the column tables of a flipped sample are reversed, so
    the kernel sees no offset and no flip.  -> (cols i32 [3, B, w], rows i32 [3, B, h]), each
    (nearest index, i0 | i1 << 16, a0 | a1 << 16).  On a source side above 65536 the taps do not
    fit their half words and are left 0 (`batch_augment_resized` then refuses rgb).  With `check`
    the entry point's table checks are run here, with a message: for whoever writes the tables
    where no entry point follows (`AugmentResizeStaging.write_params`)."""
    H, W = int(source_hw[0]), int(source_hw[1])
    h, w = int(crop_hw[0]), int(crop_hw[1])
    if H < 1 or W < 1 or h < 1 or w < 1:
        raise ValueError(f'side lengths must be positive, got {H} x {W} and {h} x {w}')
    table = check_augment_resize_params(params, len(np.asarray(params)), (h, w))
    y0, x0, flip, rh, rw = table.T
    out = []
    for src, dst, start, n in ((W, rw, x0, w), (H, rh, y0, h)):
        tables = np.zeros((3, len(table), n), np.int32)
        at = _window_positions(start, n)
        tables[0] = _cv2_nearest_window(src, dst, at)
        if src <= 65536:
            i0, i1, a0, a1 = _cv2_linear_window(src, dst, at)
            # (half words of a little-endian word: low, high)
            packed = tables[1:].view(np.uint16).reshape(2, len(table), n, 2)
            packed[0, ..., 0], packed[0, ..., 1], packed[1, ..., 0], packed[1, ..., 1] = i0, i1, a0, a1
            if check and (min(i0.min(), i1.min()) < 0 or max(i0.max(), i1.max()) >= src or
                          min(a0.min(), a1.min()) < 0 or max(a0.max(), a1.max()) > _CV2_COEF_ONE):
                raise ValueError(f'a linear tap leaves the source side of {src}')
        if check and (tables[0].min() < 0 or tables[0].max() >= src):
            raise ValueError(f'a nearest index leaves the source side of {src}')
        out.append(tables)
    cols, rows = out
    flipped = flip != 0
    cols[:, flipped] = cols[:, flipped, ::-1]
    return cols, rows


_AUGR_STAGING: 'collections.OrderedDict[tuple, AugmentResizeStaging]' = __import__('collections').OrderedDict()
_AUGR_CAPTURED = []


class AugmentResizeStaging(AugmentStaging):
    """Staging of one shape set of `batch_augment_resized`: as `AugmentStaging`, with the window
    tables of `augment_window_tables` behind the descriptors in place of the parameter triples
    (nmsa_augment_resize_desc has the layout of nmsa_augment_desc)."""

    def _tail_words(self) -> int:
        return 3 * self.B * (self.crop_hw[0] + self.crop_hw[1])

    def _bind_tail(self, tail: np.ndarray) -> None:
        h, w = self.crop_hw
        self.cols = tail[:3 * self.B * w].reshape(3, self.B, w)
        self.rows = tail[3 * self.B * w:].reshape(3, self.B, h)

    def write_params(self, params) -> None:
        """(y0, x0, flip, rh, rw) per sample for the next replay of the graph that captured this
        staging: the tables are built and checked first (a replay does not pass through the entry
        point's checks), and written only when they pass"""
        if len(np.asarray(params)) != self.B:
            raise ValueError(f'params must have {self.B} rows')
        self.cols[:], self.rows[:] = augment_window_tables(params, self.source_hw, self.crop_hw)


def batch_augment_resized(tensors: Dict[str, torch.Tensor], params, crop_hw: Tuple[int, int],
                          norm: Optional[Dict[str, tuple]] = None, return_staging: bool = False):
    """reference: RandomResize (resize.py:311-340) or RandomCrop's upscale (crop.py:43-55), then
    the chain of `batch_augment`, for a whole collated batch by ONE launch of
    nmsa_batch_augment_resized behind one asynchronous copy of the descriptors and the window
    tables; the resized images are never formed.  `params`: integer [B,5], (y0, x0, flip, rh, rw)
    per sample — the source resized to rh x rw (cv2.INTER_LINEAR for the 'rgb_norm' entry,
    cv2.INTER_NEAREST for every other, resize.py:113-120), cropped to `crop_hw` at (y0, x0), then
    flipped.  `tensors`, `norm`, the result and `return_staging` (an `AugmentResizeStaging`) as
    `batch_augment`.  This wrapper always takes the resize kernel, also where rh x rw is the
    source's size (the result is then `batch_augment`'s, bit for bit)."""
    h, w = int(crop_hw[0]), int(crop_hw[1])
    sig, dev, BHW = _augment_signature(tensors, norm or {})
    if not sig:
        return ({}, None) if return_staging else {}
    B, H, W = BHW
    if max(H, W) > 65536 and any(mode == 'rgb_norm' for _, _, _, mode, _ in sig):
        raise ValueError(f'rgb_norm behind a resize takes sources of at most 65536 a side, got {H} x {W}')
    if len(np.asarray(params)) != B:
        raise ValueError(f'params must have {B} rows')
    # (the entry point checks every table entry)
    cols, rows = augment_window_tables(params, (H, W), (h, w), check=False)

    def write(st):
        st.cols[:], st.rows[:] = cols, rows
    result, st = _augment_launch('batch_augment_resized', _AUGR_STAGING, _AUGR_CAPTURED, AugmentResizeStaging, tensors,
                                 sig, dev, BHW, (h, w), write, L.lib().nmsa_batch_augment_resized)
    return (result, st) if return_staging else result


# ----------------------------------------------------------------------------- normals
RMSE_MASK_NONE, RMSE_MASK_GIVEN, RMSE_MASK_FROM_TARGET = 0, 1, 2


def _require_on_device(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise L.NmsaError(f'{name} is on {t.device}: the HIP path needs tensors on the MI355X '
                          '(there is no CPU fallback).')


def normal_valid_mask(target: torch.Tensor) -> torch.Tensor:
    """reference: `_get_valid_gt_normals` (task_helper/normal.py:165-167) — bool [B,H,W], False
    where all three channels of `target` [B,3,H,W] equal zero (by value: -0.0 counts, NaN does
    not), from one pass over the target."""
    if target.dtype != torch.float32:
        raise TypeError(f'target must be float32, got {target.dtype}')
    _require_on_device(target, 'target')
    if target.ndim != 4 or target.shape[1] != 3:
        raise ValueError(f'target must be [B, 3, H, W], got shape {tuple(target.shape)}')
    t = target.contiguous()
    B, _, H, W = (int(n) for n in t.shape)
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=t.device)
    if mask.numel():
        L.check(L.lib().nmsa_normal_valid_mask(L.ptr(t), B, H, W, L.ptr(mask), L.stream_ptr(t.device)),
                'nmsa_normal_valid_mask')
    return mask.view(torch.bool)


def rmse_update(sum_state: torch.Tensor, count_state: torch.Tensor, preds: torch.Tensor,
                target: torch.Tensor, mask=None, crop=None) -> None:
    """reference: `RootMeanSquaredError.update` (metric/rmse.py:30-57) into the metric's device
    states: sum_state (float64 scalar) += sum_px sqrt(mean_c (preds - target)^2), count_state
    (int64 scalar) += pixels, no host sync.  `mask`: None, a bool / uint8 [B,H,W] tensor, or
    'target' (valid-normal rule of `normal_valid_mask`, evaluated on the fly).  `preds` has the
    target's shape, or — with `crop` = the valid-region slices, or any other spatial size — is
    the network-resolution map that `resize_nearest(preds, target.shape[-2:], crop)` would bring
    to the target's resolution; that map is then never written."""
    if target.dtype != torch.float32:
        raise TypeError(f'target must be float32, got {target.dtype}')
    code = L.float_dtype_code(preds)                # TypeError for anything but f32 / bf16 / f16
    for name, t in (('preds', preds), ('target', target), ('sum_state', sum_state),
                    ('count_state', count_state)):
        _require_on_device(t, name)
    if sum_state.dtype != torch.float64 or count_state.dtype != torch.int64 or \
            sum_state.numel() != 1 or count_state.numel() != 1:
        raise TypeError('the states are one float64 and one int64 element')
    if preds.ndim != 4 or target.ndim != 4 or preds.shape[:2] != target.shape[:2]:
        raise ValueError(f'preds / target must be [B, C, H, W] with the same B and C, got '
                         f'{tuple(preds.shape)} / {tuple(target.shape)}')
    p, t = preds.contiguous(), target.contiguous()
    B, C, H, W = (int(n) for n in t.shape)
    if not 1 <= C <= 8:
        raise ValueError(f'1 to 8 channels are supported, got {C}')
    source = (0, 0, 0, 0, 0, 0)
    if crop is not None or tuple(p.shape[-2:]) != (H, W):
        source = _crop_geometry(p, crop)
        if source == (H, W, 0, 0, H, W):
            # the crop is the whole map and nothing is resized: the prediction IS at the target's
            # resolution, read it with whole-group loads instead of per-pixel gathers
            source = (0, 0, 0, 0, 0, 0)
    if isinstance(mask, str):
        if mask != 'target':
            raise ValueError(f"mask must be None, a tensor or 'target', got '{mask}'")
        if C != 3:
            raise ValueError("mask='target' is the rule for 3-channel normals")
        mode, m = RMSE_MASK_FROM_TARGET, None
    elif mask is None:
        mode, m = RMSE_MASK_NONE, None
    else:
        _require_on_device(mask, 'mask')
        if tuple(mask.shape) != (B, H, W):
            raise ValueError(f'mask must be [B, H, W] = {(B, H, W)}, got {tuple(mask.shape)}')
        mode, m = RMSE_MASK_GIVEN, _u8(mask)
    if t.numel() == 0:
        return
    L.check(L.lib().nmsa_rmse_update(
        L.ptr(p), code, L.ptr(t), L.ptr(m), mode, B, C, H, W, *source,
        L.ptr(sum_state), L.ptr(count_state), L.stream_ptr(t.device)), 'nmsa_rmse_update')


# ----------------------------------------------------------------------------- scene
_SCENE_OUTPUTS = ('score', 'idx', 'loss', 'grad')


def scene_step(logits: torch.Tensor, labels: Optional[torch.Tensor] = None,
               class_weights: Optional[torch.Tensor] = None, label_smoothing: float = 0.0,
               want: Sequence[str] = ('score', 'idx'), confmat: Optional[torch.Tensor] = None,
               status: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The scene task's step in one launch (include/nmsa.h nmsa_scene_step), no host sync.
    `logits` [B, C] float32 / bfloat16 / float16; `labels` [B] uint8 / int32 / int64 in the form of
    batch['scene'] (0 = void, class c is c + 1) or None.  `want` names the outputs to allocate and
    return: 'score' float32 [B] and 'idx' int64 [B] (reference model/postprocessing/scene.py:42-44),
    'loss' float32 [3] = (numerator, divisor, loss) of torch.nn.CrossEntropyLoss(class_weights,
    label_smoothing, ignore_index=-1, reduction='mean') on labels - 1, 'grad' [B, C] in the
    logits' dtype = d loss / d logits.  `confmat` int64 [C, C] is ADDED into (row = label - 1,
    column = idx) and returned as given.  `status` int32 [1] (allocated when labels are given and
    none is passed) collects L.NMSA_ST_VALUE_RANGE for labels outside 0..C, whose rows count as void."""
    want = tuple(want)
    unknown = [w for w in want if w not in _SCENE_OUTPUTS]
    if unknown:
        raise ValueError(f'unknown outputs {unknown}; known: {_SCENE_OUTPUTS}')
    code = L.float_dtype_code(logits)               # TypeError for anything but f32 / bf16 / f16
    _require_on_device(logits, 'logits')
    if logits.ndim != 2:
        raise ValueError(f'logits must be [B, C], got shape {tuple(logits.shape)}')
    B, C = (int(n) for n in logits.shape)
    if B < 1 or not 1 <= C <= L.NMSA_SCENE_MAX_CLASSES:
        raise ValueError(f'B >= 1 and 1 <= C <= {L.NMSA_SCENE_MAX_CLASSES} are supported, got B={B}, C={C}')
    if not 0.0 <= float(label_smoothing) <= 1.0:
        raise ValueError(f'label_smoothing must be in [0, 1], got {label_smoothing}')
    x, dev = logits.detach().contiguous(), logits.device
    lab, lab_code = None, 0
    if labels is not None:
        _require_on_device(labels, 'labels')
        if labels.dtype not in (torch.uint8, torch.int32, torch.int64):
            raise TypeError(f'labels must be uint8, int32 or int64, got {labels.dtype}')
        if tuple(labels.shape) != (B,):
            raise ValueError(f'labels must be [B] = [{B}], got shape {tuple(labels.shape)}')
        lab, lab_code = labels.contiguous(), L.int_dtype_code(labels)
    elif 'loss' in want or 'grad' in want or confmat is not None:
        raise ValueError('loss, grad and confmat need labels')
    w = None
    if class_weights is not None:
        _require_on_device(class_weights, 'class_weights')
        if class_weights.dtype != torch.float32 or tuple(class_weights.shape) != (C,):
            raise TypeError(f'class_weights must be float32 [{C}], got {class_weights.dtype} '
                            f'{tuple(class_weights.shape)}')
        w = class_weights.contiguous()
    if confmat is not None:
        _require_on_device(confmat, 'confmat')
        if confmat.dtype != torch.int64 or tuple(confmat.shape) != (C, C) or not confmat.is_contiguous():
            raise TypeError(f'confmat must be a contiguous int64 [{C}, {C}] tensor')
    if status is not None:
        _require_on_device(status, 'status')
        if status.dtype != torch.int32 or status.numel() != 1:
            raise TypeError('status is one int32 word')
    elif lab is not None:
        status = torch.zeros((1,), dtype=torch.int32, device=dev)
    out = {}
    if 'score' in want:
        out['score'] = torch.empty((B,), dtype=torch.float32, device=dev)
    if 'idx' in want:
        out['idx'] = torch.empty((B,), dtype=torch.int64, device=dev)
    if 'loss' in want:
        out['loss'] = torch.empty((3,), dtype=torch.float32, device=dev)
    if 'grad' in want:
        out['grad'] = torch.empty((B, C), dtype=x.dtype, device=dev)
    L.check(L.lib().nmsa_scene_step(
        L.ptr(x), code, L.ptr(lab), lab_code, B, C, L.ptr(w), float(label_smoothing),
        L.ptr(out.get('score')), L.ptr(out.get('idx')), L.ptr(out.get('loss')), L.ptr(out.get('grad')),
        L.ptr(confmat), L.ptr(status), L.stream_ptr(dev)), 'nmsa_scene_step')
    if confmat is not None:
        out['confmat'] = confmat
    if status is not None:
        out['status'] = status
    return out


# ----------------------------------------------------------------------------- model ops: argument checks
# What the wrappers from the learned upsampling to the scene head ask of their arguments, said once.  A tensor
# off the device is a NmsaError, anything else a TypeError (a ValueError where a wrapper says so itself).
# `dense`: the tensor must be contiguous as it is given (batch-norm tail, max pool, scene head); otherwise the
# helper hands back a detached, contiguous tensor (a copy only when the caller's is not).  Only addresses, shapes
# and dtypes of what they hand back are used, so a dense tensor is handed back as it is.  They sit on the eager path
# of every fused node: nothing is formatted, and `_require_on_device` is not even called, unless a call is refused.
def _float_map(t: torch.Tensor, name: str = 'x', dense: bool = False) -> int:
    """the dtype code of a non-empty [B, C, H, W] float32 / bfloat16 / float16 map on the device"""
    if not t.is_cuda:
        _require_on_device(t, name)
    code = L.float_dtype_code(t)                    # TypeError for anything but f32 / bf16 / f16
    if t.ndim != 4 or t.numel() == 0:
        raise TypeError(f'{name} must be a non-empty [B, C, H, W] tensor, got shape {tuple(t.shape)}')
    if dense and not t.is_contiguous():
        raise TypeError(f'{name} must be dense NCHW, got strides {tuple(t.stride())}')
    return code


def _like(t: Optional[torch.Tensor], shape: tuple, dtype: torch.dtype, device: torch.device, name: str,
          dense: bool = False) -> Optional[torch.Tensor]:
    """a further tensor of a call, of exactly this shape, dtype and device; None passes through"""
    if t is None:
        return None
    if not t.is_cuda:
        _require_on_device(t, name)
    if t.dtype != dtype or t.shape != shape or t.device != device or (dense and not t.is_contiguous()):
        raise TypeError(f'{name} must be a {"contiguous " if dense else ""}{dtype} {shape} tensor on {device}, '
                        f'got {t.dtype} {tuple(t.shape)} on {t.device}')
    return t if dense else t.detach().contiguous()


def _f32(t: Optional[torch.Tensor], shape: tuple, name: str, dense: bool = False) -> Optional[torch.Tensor]:
    """a float32 parameter or statistics tensor of exactly this shape; None passes through"""
    if t is None:
        return None
    if not t.is_cuda:
        _require_on_device(t, name)
    if t.dtype != torch.float32 or t.shape != shape or (dense and not t.is_contiguous()):
        raise TypeError(f'{name} must be a {"contiguous " if dense else ""}float32 {shape} tensor, '
                        f'got {t.dtype} {tuple(t.shape)}')
    return t if dense else t.detach().contiguous()


def _out(out: Optional[torch.Tensor], shape: tuple, dtype: torch.dtype, device: torch.device,
         name: str = 'out') -> torch.Tensor:
    """the caller's `out=` tensor, or a fresh one"""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if not out.is_cuda:
        _require_on_device(out, name)
    if out.dtype != dtype or out.shape != shape or not out.is_contiguous():
        raise TypeError(f'{name} must be a contiguous {dtype} {shape} tensor')
    return out


def _choice(value, table: dict, what: str) -> int:
    if value not in table:
        raise ValueError(f'{what} must be one of {sorted(table)}, got {value!r}')
    return table[value]


def _ptr_array(tensors):
    return (L.C.c_void_p * len(tensors))(*(None if t is None else t.data_ptr() for t in tensors))


def _int_array(values):
    return (L.C.c_int * len(values))(*values)


def _route(fn_name: str, *args) -> int:
    """the answer of a route query of the library; NmsaError for a negative one"""
    rc = getattr(L.lib(), fn_name)(*args)
    if rc < 0:
        L.check(rc, fn_name)
    return rc


# ----------------------------------------------------------------------------- learned upsampling
# partial-sum workspaces of the backward calls (learned upsampling, LayerNorm-transpose), least recently
# used first out.  One model's set must fit, or every step reallocates: up to five decoders x three
# skip scales of fusions plus two upsampling stages per head stay well below 64; an entry is at most
# a few MB (workgroups x 2 x C floats).
_BWD_WORKSPACES_MAX = 64
_BWD_WORKSPACES: 'collections.OrderedDict[tuple, torch.Tensor]' = __import__('collections').OrderedDict()


def _up_check(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]):
    """-> (dtype code of x, weight, bias); a wrong rank or an empty x is a ValueError here"""
    _require_on_device(x, 'x')
    code = L.float_dtype_code(x)                    # TypeError for anything but f32 / bf16 / f16
    if x.ndim != 4 or x.numel() == 0:
        raise ValueError(f'x must be a non-empty [B, C, h, w] tensor, got shape {tuple(x.shape)}')
    C = int(x.shape[1])
    return code, _f32(weight, (C, 1, 3, 3), 'weight'), _f32(bias, (C,), 'bias')


def _workspace(dev: torch.device, key: tuple, nbytes: int):
    """a backward call's partial sums, cached per (device, stream, key): two streams never share one.
    During a graph capture the buffer comes from the graph's memory pool instead.  `key`: the op and
    its shape; `nbytes`: what the library's size query answers for it NOW: a query that follows the
    launch grid (LayerNorm-transpose: workgroups x 2 x C floats) answers more for the same shape once
    the library sees more compute units, so a cached buffer that is too small is replaced."""
    if torch.cuda.is_current_stream_capturing():
        # a buffer of the graph's own pool: the capture stream's cache entry would outlive the graph
        ws = torch.empty(((nbytes + 15) // 16 * 4,), dtype=torch.float32, device=dev)
        return ws, ws.numel() * 4
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream) + key
    ws = _BWD_WORKSPACES.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = _BWD_WORKSPACES[key] = torch.empty(((nbytes + 15) // 16 * 4,), dtype=torch.float32, device=dev)
        while len(_BWD_WORKSPACES) > _BWD_WORKSPACES_MAX:
            _BWD_WORKSPACES.popitem(last=False)
    _BWD_WORKSPACES.move_to_end(key)
    return ws, ws.numel() * 4


def _up_workspace(dev: torch.device, shape: Tuple[int, int, int, int]):
    return _workspace(dev, ('up',) + tuple(shape), int(L.lib().nmsa_upsample2x_dw3x3_bwd_workspace_bytes(*shape)))


def upsample2x_dw3x3(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                     zeropad: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The reference's learned x2 upsampling (model/upsampling.py:85-96, modes 'learned-3x3' and, with
    `zeropad`, 'learned-3x3-zeropad') in one launch (include/nmsa.h nmsa_upsample2x_dw3x3_fwd): nearest
    x2, replication / zero pad and the depthwise 3x3 convolution.  `x` [B, C, h, w] float32 / bfloat16
    / float16 on the device (made contiguous when it is not, channels-last included), `weight` float32
    [C, 1, 3, 3], `bias` float32 [C] or None.  Returns y [B, C, 2h, 2w] in x's dtype, written into `out`
    when a contiguous tensor of that shape and dtype is given.  No autograd: that is
    `model.upsampling.LearnedUpsamplingFunction`."""
    code, w_, b_ = _up_check(x, weight, bias)
    xc = x.detach().contiguous()
    B, C, h, w = (int(n) for n in xc.shape)
    y = _out(out, (B, C, 2 * h, 2 * w), xc.dtype, xc.device)
    L.check(L.lib().nmsa_upsample2x_dw3x3_fwd(
        L.ptr(xc), code, L.ptr(w_), L.ptr(b_), B, C, h, w, int(bool(zeropad)), L.ptr(y),
        L.stream_ptr(xc.device)), 'nmsa_upsample2x_dw3x3_fwd')
    return y


def upsample2x_dw3x3_backward(gy: torch.Tensor, x: torch.Tensor, weight: torch.Tensor, zeropad: bool = False,
                              need_gx: bool = True, need_gweight: bool = True, need_gbias: bool = True):
    """(gx, gweight, gbias) of `upsample2x_dw3x3` for the upstream gradient `gy` [B, C, 2h, 2w] (x's
    dtype; made contiguous when it is not), None where not needed (nmsa_upsample2x_dw3x3_bwd).  gx has
    x's dtype, gweight [C, 1, 3, 3] and gbias [C] are float32.  Deterministic: a fixed order of
    summation, the same bits on every call."""
    code, w_, _ = _up_check(x, weight, None)
    B, C, h, w = (int(n) for n in x.shape)
    g = _like(gy, (B, C, 2 * h, 2 * w), x.dtype, x.device, 'gy')
    xc = x.detach().contiguous()
    dev = xc.device
    gx = torch.empty_like(xc) if need_gx else None
    gw = torch.empty((C, 1, 3, 3), dtype=torch.float32, device=dev) if need_gweight else None
    gb = torch.empty((C,), dtype=torch.float32, device=dev) if need_gbias else None
    ws, ws_bytes = _up_workspace(dev, (B, C, h, w)) if (need_gweight or need_gbias) else (None, 0)
    L.check(L.lib().nmsa_upsample2x_dw3x3_bwd(
        L.ptr(g), L.ptr(xc), code, L.ptr(w_), B, C, h, w, int(bool(zeropad)),
        L.ptr(gx), L.ptr(gw), L.ptr(gb), L.ptr(ws), ws_bytes, L.stream_ptr(dev)), 'nmsa_upsample2x_dw3x3_bwd')
    return gx, gw, gb


def upsample2x_dw3x3_route(x: torch.Tensor, other: torch.Tensor) -> int:
    """The route a call with these tensors takes (`nmsa_upsample2x_dw3x3_route`):
    L.NMSA_UP_ROUTE_VECTOR or L.NMSA_UP_ROUTE_PIXEL.  `x` [B, C, h, w] is an input-sized tensor of the
    call, `other` another tensor of it (y, gy or gx); only shapes, the dtype and the addresses are
    looked at, nothing is launched."""
    if x.ndim != 4:
        raise ValueError(f'x must be [B, C, h, w], got shape {tuple(x.shape)}')
    B, C, h, w = (int(n) for n in x.shape)
    return _route('nmsa_upsample2x_dw3x3_route', x.data_ptr(), other.data_ptr(), L.float_dtype_code(x), B, C, h, w)


# ------------------------------------------------------- Swin fusion: LayerNorm + NHWC -> NCHW (+ add)
def _lnt_check(x: torch.Tensor, gamma: torch.Tensor, beta: Optional[torch.Tensor]):
    """-> (dtype code, B, P, C, spatial shape, gamma, beta) of an encoder skip tensor [B, H, W, C] or [B, P, C];
    a wrong rank or an empty x is a ValueError here"""
    _require_on_device(x, 'x')
    code = L.float_dtype_code(x)                    # TypeError for anything but f32 / bf16 / f16
    if x.ndim not in (3, 4) or x.numel() == 0:
        raise ValueError(f'x must be a non-empty [B, H, W, C] or [B, P, C] tensor, got shape {tuple(x.shape)}')
    B, C, spatial = int(x.shape[0]), int(x.shape[-1]), tuple(int(n) for n in x.shape[1:-1])
    return code, B, int(np.prod(spatial)), C, spatial, _f32(gamma, (C,), 'gamma'), _f32(beta, (C,), 'beta')


def ln_nhwc_to_nchw(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                    add: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                    out_dtype: Optional[torch.dtype] = None, save_stats: bool = False):
    """The reference's Swin encoder-decoder fusion (model/encoder_decoder_fusion.py:123-148) in one
    launch (include/nmsa.h nmsa_ln_nhwc_nchw_fwd): LayerNorm over the last axis of `x` [B, H, W, C]
    (or [B, P, C]; float32 / bfloat16 / float16 on the device, made contiguous when it is not) with
    float32 `gamma`, `beta` [C], the result as NCHW [B, C, H, W] ([B, C, P]) in `out_dtype` (x's dtype
    or float32; default x's), plus `add` (a tensor of the output's shape and dtype) when given.
    Written into `out` when a contiguous tensor of that shape and dtype is given.  Returns y, or
    (y, mean, rstd) with `save_stats` (float32 [B*P], what `ln_nhwc_to_nchw_backward` takes).  No
    autograd: that is `model.encoder_decoder_fusion.SwinFusionFunction`."""
    code, B, P, C, spatial, g_, b_ = _lnt_check(x, gamma, beta)
    out_dtype = x.dtype if out_dtype is None else out_dtype
    if out_dtype not in (x.dtype, torch.float32):
        raise TypeError(f'out_dtype must be {x.dtype} or torch.float32, got {out_dtype}')
    xc = x.detach().contiguous()
    shape = (B, C) + spatial
    a_ = _like(add, shape, out_dtype, xc.device, 'add')
    y = _out(out, shape, out_dtype, xc.device)
    mean = rstd = None
    if save_stats:
        mean = torch.empty((B * P,), dtype=torch.float32, device=xc.device)
        rstd = torch.empty((B * P,), dtype=torch.float32, device=xc.device)
    L.check(L.lib().nmsa_ln_nhwc_nchw_fwd(
        L.ptr(xc), code, L.ptr(g_), L.ptr(b_), float(eps), L.ptr(a_), B, P, C, L.ptr(y), L.float_dtype_code(y),
        L.ptr(mean), L.ptr(rstd), L.stream_ptr(xc.device)), 'nmsa_ln_nhwc_nchw_fwd')
    return (y, mean, rstd) if save_stats else y


def ln_nhwc_to_nchw_backward(gy: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, mean: torch.Tensor,
                             rstd: torch.Tensor, need_gx: bool = True, need_ggamma: bool = True,
                             need_gbeta: bool = True):
    """(gx, ggamma, gbeta) of `ln_nhwc_to_nchw` for the upstream gradient `gy` [B, C, H, W] (x's dtype
    or float32; made contiguous when it is not) and the statistics the forward call saved, None where
    not needed (nmsa_ln_nhwc_nchw_bwd).  gx has x's shape and dtype, ggamma and gbeta are float32 [C].
    Deterministic: a fixed order of summation, the same bits on every call."""
    code, B, P, C, spatial, g_, _ = _lnt_check(x, gamma, None)
    # gy: x's dtype, or float32 (what the forward call wrote under autocast)
    g = _like(gy, (B, C) + spatial, torch.float32 if gy.dtype == torch.float32 else x.dtype, x.device, 'gy')
    # the saved statistics: [B * P], and as ever any other shape of that many elements
    m_ = _f32(mean, mean.shape if mean.numel() == B * P else (B * P,), 'mean')
    r_ = _f32(rstd, rstd.shape if rstd.numel() == B * P else (B * P,), 'rstd')
    xc = x.detach().contiguous()
    dev = xc.device
    gx = torch.empty_like(xc) if need_gx else None
    gg = torch.empty((C,), dtype=torch.float32, device=dev) if need_ggamma else None
    gb = torch.empty((C,), dtype=torch.float32, device=dev) if need_gbeta else None
    ws, ws_bytes = (_workspace(dev, ('lnt', B, P, C), int(L.lib().nmsa_ln_nhwc_nchw_bwd_workspace_bytes(B, P, C)))
                    if (need_ggamma or need_gbeta) else (None, 0))
    L.check(L.lib().nmsa_ln_nhwc_nchw_bwd(
        L.ptr(g), L.float_dtype_code(g), L.ptr(xc), code, L.ptr(g_), L.ptr(m_), L.ptr(r_), B, P, C,
        L.ptr(gx), L.ptr(gg), L.ptr(gb), L.ptr(ws), ws_bytes, L.stream_ptr(dev)), 'nmsa_ln_nhwc_nchw_bwd')
    return gx, gg, gb


def ln_nhwc_to_nchw_route(x: torch.Tensor, y: torch.Tensor) -> int:
    """The route a call with these tensors takes (`nmsa_ln_nhwc_nchw_route`): L.NMSA_LNT_ROUTE_VECTOR
    or L.NMSA_LNT_ROUTE_ELEMENT.  `x` [B, H, W, C] / [B, P, C] is an NHWC tensor of the call (x, gx),
    `y` an NCHW one (y, add, gy); only shapes, dtypes and addresses are looked at, nothing is launched."""
    if x.ndim not in (3, 4):
        raise ValueError(f'x must be [B, H, W, C] or [B, P, C], got shape {tuple(x.shape)}')
    B, C = int(x.shape[0]), int(x.shape[-1])
    P = int(np.prod([int(n) for n in x.shape[1:-1]]))
    return _route('nmsa_ln_nhwc_nchw_route', x.data_ptr(), y.data_ptr(), L.float_dtype_code(x),
                  L.float_dtype_code(y), B, P, C)


# --------------------------------------------- context module: pyramid pooling, upsample + concat
_PPM_MODES = {'nearest': L.NMSA_PPM_NEAREST, 'bilinear': L.NMSA_PPM_BILINEAR}


def _ppm_sizes(sizes) -> Tuple[Tuple[int, int], ...]:
    """((ph, pw), ...) from a sequence of ints (square) or (ph, pw) pairs"""
    out = []
    for s in sizes:
        ph, pw = (s, s) if isinstance(s, int) else s
        if int(ph) < 1 or int(pw) < 1:
            raise ValueError(f'pool sizes must be at least 1, got {s}')
        out.append((int(ph), int(pw)))
    if not 1 <= len(out) <= L.NMSA_PPM_MAX_BINS:
        raise ValueError(f'1..{L.NMSA_PPM_MAX_BINS} pool sizes per call, got {len(out)}')
    return tuple(out)


# sizes as given -> (normalised sizes, ph array, pw array): a model asks for the same few tuples in
# every step, and building them again is a good part of a call's host time at these map sizes
_PPM_SIZE_ARGS: dict = {}


def _ppm_size_args(sizes):
    key = sizes if isinstance(sizes, tuple) else tuple(tuple(s) if not isinstance(s, int) else s for s in sizes)
    hit = _PPM_SIZE_ARGS.get(key)
    if hit is None:
        sz = _ppm_sizes(key)
        if len(_PPM_SIZE_ARGS) >= 64:
            _PPM_SIZE_ARGS.clear()
        hit = _PPM_SIZE_ARGS[key] = (sz, _int_array([s[0] for s in sz]), _int_array([s[1] for s in sz]))
    return hit


def ppm_pool(x: torch.Tensor, sizes) -> Tuple[torch.Tensor, ...]:
    """All adaptive average pools of the context module in one launch (include/nmsa.h
    nmsa_ppm_pool_fwd): `x` [B, C, H, W] float32 / bfloat16 / float16 on the device (made contiguous
    when it is not, channels-last included), `sizes` 1..4 ints or (ph, pw) pairs.  Returns one
    contiguous [B, C, ph, pw] tensor per size in x's dtype: `F.adaptive_avg_pool2d(x, size)` with
    float32 sums.  No autograd: that is `model.context_module.PyramidPoolFunction`."""
    code = _float_map(x)
    sz, phs, pws = _ppm_size_args(sizes)
    xc = x.detach().contiguous()
    B, C, H, W = xc.shape
    outs = tuple(torch.empty((B, C, ph, pw), dtype=xc.dtype, device=xc.device) for ph, pw in sz)
    L.check(L.lib().nmsa_ppm_pool_fwd(
        L.ptr(xc), code, B, C, H, W, len(sz), phs, pws, _ptr_array(outs), L.stream_ptr(xc.device)),
        'nmsa_ppm_pool_fwd')
    return outs


def ppm_pool_backward(gps, x_shape, sizes) -> torch.Tensor:
    """gx [B, C, H, W] of `ppm_pool` for the gradients `gps` of its outputs (one per size, all of one
    dtype, [B, C, ph, pw], made contiguous when they are not; None: that output was not used) in one
    launch (nmsa_ppm_pool_bwd).  Deterministic: a gather in a fixed order, the same bits on every call."""
    sz, phs, pws = _ppm_size_args(sizes)
    B, C, H, W = (int(n) for n in x_shape)
    gps = tuple(gps)
    given = [g for g in gps if g is not None]
    if len(gps) != len(sz) or not given:
        raise TypeError(f'one gradient (or None) per size and at least one tensor, got {len(gps)} for {len(sz)} sizes')
    code = _float_map(given[0], 'gps')
    dev = given[0].device
    gc = [_like(g, (B, C, ph, pw), given[0].dtype, dev, 'gps') for g, (ph, pw) in zip(gps, sz)]
    gx = torch.empty((B, C, H, W), dtype=given[0].dtype, device=dev)
    L.check(L.lib().nmsa_ppm_pool_bwd(
        _ptr_array(gc), code, B, C, H, W, len(sz), phs, pws, L.ptr(gx), L.stream_ptr(dev)), 'nmsa_ppm_pool_bwd')
    return gx


def ppm_upsample_concat(x: torch.Tensor, ys, mode: str = 'bilinear',
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`torch.cat([x] + [F.interpolate(y, (H, W), mode) for y in ys], 1)` in one launch
    (nmsa_ppm_upcat_fwd): `x` [B, C, H, W] float32 / bfloat16 / float16 on the device, `ys` 1..4
    branch outputs [B, Cr_i, ph_i, pw_i] of x's dtype (all made contiguous when they are not), `mode`
    'nearest' or 'bilinear' (align_corners=False).  Returns [B, C + sum Cr_i, H, W], written into `out`
    when a contiguous tensor of that shape and dtype is given.  No autograd: that is
    `model.context_module.UpsampleConcatFunction`."""
    code = _float_map(x)
    m = _choice(mode, _PPM_MODES, 'mode')
    xc = x.detach().contiguous()
    B, C, H, W = (int(n) for n in xc.shape)
    ys = tuple(ys)
    if not 1 <= len(ys) <= L.NMSA_PPM_MAX_BINS:
        raise ValueError(f'1..{L.NMSA_PPM_MAX_BINS} branches per call, got {len(ys)}')
    yc = []
    for y in ys:
        _require_on_device(y, 'ys')
        if y.dtype != xc.dtype or y.ndim != 4 or int(y.shape[0]) != B or y.numel() == 0:
            raise TypeError(f'ys must be non-empty {xc.dtype} [{B}, Cr, ph, pw] tensors, got {y.dtype} {tuple(y.shape)}')
        yc.append(y.detach().contiguous())
    shape = (B, C + sum(int(y.shape[1]) for y in yc), H, W)
    o = _out(out, shape, xc.dtype, xc.device)
    L.check(L.lib().nmsa_ppm_upcat_fwd(
        L.ptr(xc), _ptr_array(yc), code, B, C, H, W, len(yc), _int_array([int(y.shape[1]) for y in yc]),
        _int_array([int(y.shape[2]) for y in yc]), _int_array([int(y.shape[3]) for y in yc]), m, L.ptr(o),
        L.stream_ptr(xc.device)), 'nmsa_ppm_upcat_fwd')
    return o


def ppm_upsample_concat_backward(g_out: torch.Tensor, n_channels_x: int, branch_shapes, mode: str = 'bilinear',
                                 need=None) -> Tuple[Optional[torch.Tensor], ...]:
    """The gradients of the branch outputs of `ppm_upsample_concat` for the upstream gradient `g_out`
    [B, C + sum Cr_i, H, W] (made contiguous when it is not) in one launch (nmsa_ppm_upcat_bwd).
    `branch_shapes`: the shapes [B, Cr_i, ph_i, pw_i] of the branches; `need`: one bool per branch
    (default all), None is returned for the others.  The gradient of x is the view
    `g_out[:, :n_channels_x]`: no kernel.  Deterministic: a gather in a fixed order."""
    code = _float_map(g_out, 'g_out')
    m = _choice(mode, _PPM_MODES, 'mode')
    shapes = [tuple(int(n) for n in s) for s in branch_shapes]
    if not 1 <= len(shapes) <= L.NMSA_PPM_MAX_BINS:
        raise ValueError(f'1..{L.NMSA_PPM_MAX_BINS} branches per call, got {len(shapes)}')
    need = [True] * len(shapes) if need is None else [bool(n) for n in need]
    B, Ct, H, W = (int(n) for n in g_out.shape)
    C = int(n_channels_x)
    if (len(need) != len(shapes) or any(len(s) != 4 or s[0] != B or min(s) < 1 for s in shapes)
            or C < 1 or C + sum(s[1] for s in shapes) != Ct):
        raise TypeError(f'g_out {tuple(g_out.shape)} does not match {C} channels of x and the branches {shapes}')
    g = g_out.detach().contiguous()
    gys = tuple(torch.empty(s, dtype=g.dtype, device=g.device) if n else None for s, n in zip(shapes, need))
    L.check(L.lib().nmsa_ppm_upcat_bwd(
        L.ptr(g), code, B, C, H, W, len(shapes), _int_array([s[1] for s in shapes]),
        _int_array([s[2] for s in shapes]), _int_array([s[3] for s in shapes]), m, _ptr_array(gys),
        L.stream_ptr(g.device)), 'nmsa_ppm_upcat_bwd')
    return gys


def ppm_route(hw: Tuple[int, int], sizes) -> int:
    """The route `ppm_pool` and `ppm_upsample_concat_backward` take for a map of `hw` = (H, W) and
    these pool sizes (`nmsa_ppm_route`): L.NMSA_PPM_ROUTE_LDS or L.NMSA_PPM_ROUTE_GLOBAL.  Host only,
    nothing is launched."""
    sz, phs, pws = _ppm_size_args(sizes)
    return _route('nmsa_ppm_route', int(hw[0]), int(hw[1]), len(sz), phs, pws)


# ------------------------------------------------ MLP decoders: all branches into the concatenation
_MLPDEC_MODES = {'nearest': L.NMSA_MLPDEC_NEAREST, 'bilinear': L.NMSA_MLPDEC_BILINEAR}
_MLPDEC_MAX_SHIFT = 4


def _mlpdec_shifts(shapes, size=None) -> Tuple[int, int, Tuple[int, ...]]:
    """(H, W, (s_0, ...)) from the branch shapes [B, c_i, h_i, w_i]: H x W is `size`, by default the
    largest map, and every branch must reach it by one power-of-two factor 1 << s_i up to 16, the same
    along H and W.  ValueError for anything else: another factor, factors that differ between H and W, maps that do
    not meet at one output size, no branch or more than four."""
    shapes = [tuple(int(n) for n in s) for s in shapes]
    if not 1 <= len(shapes) <= L.NMSA_MLPDEC_MAX_BRANCHES:
        raise ValueError(f'1..{L.NMSA_MLPDEC_MAX_BRANCHES} branches per call, got {len(shapes)}')
    if any(len(s) != 4 or min(s) < 1 for s in shapes):
        raise ValueError(f'branches must be non-empty [B, c, h, w] maps, got {shapes}')
    H, W = (max(s[2] for s in shapes), max(s[3] for s in shapes)) if size is None else (int(size[0]), int(size[1]))
    shifts = []
    for s in shapes:
        if H % s[2] or W % s[3]:
            raise ValueError(f'a {s[2]}x{s[3]} map does not reach {H}x{W} by a whole factor')
        fh, fw = H // s[2], W // s[3]
        if fh != fw:
            raise ValueError(f'a {s[2]}x{s[3]} map reaches {H}x{W} by {fh} along H and {fw} along W')
        if fh & (fh - 1) or fh > 1 << _MLPDEC_MAX_SHIFT:
            raise ValueError(f'factor {fh} is not a power of two up to {1 << _MLPDEC_MAX_SHIFT}')
        shifts.append(fh.bit_length() - 1)
    return H, W, tuple(shifts)


def mlpdec_upsample_concat(ys, mode: str = 'bilinear', size=None) -> torch.Tensor:
    """`torch.cat([F.interpolate(y, (H, W), mode) for y in ys], 1)` in one launch
    (nmsa_mlpdec_upcat_fwd): `ys` 1..4 maps [B, c_i, H >> s_i, W >> s_i] of one dtype (float32 /
    bfloat16 / float16) on the device, made contiguous when they are not; H x W is `size`, by default
    the largest of them, and every factor a power of two up to 16 (`_mlpdec_shifts`).  `mode`
    'nearest' or 'bilinear' (align_corners=False); a branch that is already H x W is copied.  Returns
    [B, sum c_i, H, W].  No autograd: that is `model.decoder.MlpUpsampleConcatFunction`."""
    ys = tuple(ys)
    m = _choice(mode, _MLPDEC_MODES, 'mode')
    for y in ys:
        _require_on_device(y, 'ys')
    H, W, shifts = _mlpdec_shifts([tuple(y.shape) for y in ys], size)
    code = _float_map(ys[0], 'ys')
    B = int(ys[0].shape[0])
    yc = []
    for y in ys:
        if y.dtype != ys[0].dtype or int(y.shape[0]) != B or y.device != ys[0].device:
            raise TypeError(f'ys must be {ys[0].dtype} [{B}, c, h, w] tensors on one device, '
                            f'got {y.dtype} {tuple(y.shape)}')
        yc.append(y.detach().contiguous())
    cs = [int(y.shape[1]) for y in yc]
    out = torch.empty((B, sum(cs), H, W), dtype=yc[0].dtype, device=yc[0].device)
    L.check(L.lib().nmsa_mlpdec_upcat_fwd(
        _ptr_array(yc), code, B, H, W, len(yc), _int_array(cs), _int_array(shifts), m, L.ptr(out),
        L.stream_ptr(out.device)), 'nmsa_mlpdec_upcat_fwd')
    return out


def mlpdec_upsample_concat_backward(g_out: torch.Tensor, branch_shapes, mode: str = 'bilinear',
                                    need=None) -> Tuple[Optional[torch.Tensor], ...]:
    """The gradients of the branches of `mlpdec_upsample_concat` for the upstream gradient `g_out`
    [B, sum c_i, H, W] (made contiguous when it is not) in one launch (nmsa_mlpdec_upcat_bwd).
    `branch_shapes`: the shapes [B, c_i, h_i, w_i]; `need`: one bool per branch (default all), None is
    returned for the others.  The gradient of a branch that is already H x W is the view
    `g_out[:, off_i:off_i + c_i]`: no kernel.  Deterministic: a gather in a fixed order."""
    code = _float_map(g_out, 'g_out')
    m = _choice(mode, _MLPDEC_MODES, 'mode')
    shapes = [tuple(int(n) for n in s) for s in branch_shapes]
    H, W, shifts = _mlpdec_shifts(shapes, (g_out.shape[2], g_out.shape[3]) if g_out.ndim == 4 else None)
    need = [True] * len(shapes) if need is None else [bool(n) for n in need]
    B, Ct = int(g_out.shape[0]), int(g_out.shape[1])
    if (len(need) != len(shapes) or any(s[0] != B for s in shapes) or sum(s[1] for s in shapes) != Ct
            or (int(g_out.shape[2]), int(g_out.shape[3])) != (H, W)):
        raise TypeError(f'g_out {tuple(g_out.shape)} does not match the branches {shapes}')
    g = g_out.detach().contiguous()
    gys, off = [], 0
    for s, sh, n in zip(shapes, shifts, need):
        if not n:
            gys.append(None)
        elif sh == 0:
            gys.append(g[:, off:off + s[1]])
        else:
            gys.append(torch.empty(s, dtype=g.dtype, device=g.device))
        off += s[1]
    asked = [t if t is not None and sh else None for t, sh in zip(gys, shifts)]
    if any(t is not None for t in asked):
        L.check(L.lib().nmsa_mlpdec_upcat_bwd(
            L.ptr(g), code, B, H, W, len(shapes), _int_array([s[1] for s in shapes]), _int_array(shifts), m,
            _ptr_array(asked), L.stream_ptr(g.device)), 'nmsa_mlpdec_upcat_bwd')
    return tuple(gys)


def mlpdec_route(ys, out: torch.Tensor) -> int:
    """The route `mlpdec_upsample_concat` takes with the branch maps `ys` and the output tensor `out`
    (`nmsa_mlpdec_route`): L.NMSA_MLPDEC_ROUTE_VECTOR (16 bytes per lane: W a multiple of 4 float32 /
    8 half pixels and every tensor on 16 bytes) or L.NMSA_MLPDEC_ROUTE_ELEMENT.  Host only, nothing is
    launched; the backward has one route."""
    ys = tuple(ys)
    H, W, shifts = _mlpdec_shifts([tuple(y.shape) for y in ys], (out.shape[2], out.shape[3]))
    return _route('nmsa_mlpdec_route', _ptr_array(ys), L.ptr(out), L.float_dtype_code(out), H, W, len(ys),
                  _int_array(shifts))


# ------------------------------------------------ dense decoders: x2 upsampling + skip add in one launch
_UPADD_MODES = {'nearest': L.NMSA_UPADD_NEAREST, 'bilinear': L.NMSA_UPADD_BILINEAR,
                'learned-3x3': L.NMSA_UPADD_LEARNED, 'learned-3x3-zeropad': L.NMSA_UPADD_LEARNED_ZEROPAD}


def _upadd_shapes(x: torch.Tensor, skip: torch.Tensor) -> Tuple[int, int, int, int]:
    """(B, C, h, w) of x; a skip that is not a [B, C, 2h, 2w] map is a ValueError"""
    B, C, h, w = (int(n) for n in x.shape)
    if tuple(skip.shape) != (B, C, 2 * h, 2 * w):
        raise ValueError(f'skip must be [{B}, {C}, {2 * h}, {2 * w}] for x {tuple(x.shape)}, got {tuple(skip.shape)}')
    return B, C, h, w


def up2x_add(x: torch.Tensor, skip: torch.Tensor, mode: str, weight: Optional[torch.Tensor] = None,
             bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`Upsampling(mode)(x) + skip` of the dense decoder modules in one launch (include/nmsa.h
    nmsa_up2x_add_fwd): `x` [B, C, h, w] and `skip` [B, C, 2h, 2w] of one dtype (float32 / bfloat16 / float16) on
    the device, made contiguous when they are not.  `mode` 'nearest', 'bilinear' (align_corners=False),
    'learned-3x3' or 'learned-3x3-zeropad'; the learned modes take `weight` float32 [C, 1, 3, 3] and `bias`
    float32 [C] or None, the other two ignore both.  Float32 inside, a half result is rounded once, after the
    addition.  Returns y [B, C, 2h, 2w] in x's dtype, written into `out` when a contiguous tensor of that shape
    and dtype is given (it must not overlap x or skip).  No autograd: that is
    `model.decoder.UpsampleAddFunction`."""
    m = _choice(mode, _UPADD_MODES, 'mode')
    if x.is_cuda and (x.ndim != 4 or x.numel() == 0):
        raise ValueError(f'x must be a non-empty [B, C, h, w] tensor, got shape {tuple(x.shape)}')
    code = _float_map(x, 'x')
    _require_on_device(skip, 'skip')
    B, C, h, w = _upadd_shapes(x, skip)
    learned = m in (L.NMSA_UPADD_LEARNED, L.NMSA_UPADD_LEARNED_ZEROPAD)
    if learned and weight is None:
        raise TypeError(f"mode '{mode}' needs a weight")
    w_ = _f32(weight, (C, 1, 3, 3), 'weight') if learned else None
    b_ = _f32(bias, (C,), 'bias') if learned else None
    xc = x.detach().contiguous()
    sc = _like(skip, (B, C, 2 * h, 2 * w), xc.dtype, xc.device, 'skip')
    y = _out(out, (B, C, 2 * h, 2 * w), xc.dtype, xc.device)
    L.check(L.lib().nmsa_up2x_add_fwd(
        L.ptr(xc), code, m, L.ptr(w_), L.ptr(b_), L.ptr(sc), B, C, h, w, L.ptr(y), L.stream_ptr(xc.device)),
        'nmsa_up2x_add_fwd')
    return y


def up2x_add_route(x: torch.Tensor, skip: torch.Tensor, y: torch.Tensor) -> int:
    """The route `up2x_add` takes with these tensors (`nmsa_up2x_add_route`): L.NMSA_UPADD_ROUTE_VECTOR (w a
    multiple of 2 float32 / 4 half pixels and x, skip and y on 16 bytes) or L.NMSA_UPADD_ROUTE_PIXEL.  Only
    shapes, the dtype and the addresses are looked at, nothing is launched."""
    if x.ndim != 4:
        raise ValueError(f'x must be [B, C, h, w], got shape {tuple(x.shape)}')
    B, C, h, w = _upadd_shapes(x, skip)
    return _route('nmsa_up2x_add_route', x.data_ptr(), skip.data_ptr(), y.data_ptr(), L.float_dtype_code(x),
                  B, C, h, w)


# ------------------------------------------------------- encoder RGB-D fusion: SE-weighted add
_SEFUSE_ACTS = {'relu': L.NMSA_SEFUSE_ACT_RELU, 'silu': L.NMSA_SEFUSE_ACT_SILU}


def _sefuse_maps(first: torch.Tensor, others, names) -> Tuple[int, Tuple[int, int, int, int], list]:
    """dtype code, (B, C, H, W) and the detached, contiguous maps of a call: `first` sets device, dtype
    and shape, every tensor of `others` (None allowed) must match it"""
    code = _float_map(first, names[0])
    shape = tuple(int(n) for n in first.shape)
    if shape[1] < 16:
        raise ValueError(f'the SE weighting needs at least 16 channels, got {shape[1]}')
    maps = [first.detach().contiguous()]
    for t, name in zip(others, names[1:]):
        maps.append(_like(t, shape, first.dtype, first.device, name))
    return code, shape, maps


def _sefuse_params(params, C: int, device, n_each: int):
    """the float32 parameter tensors of one call as a pointer array: per modality W1 [R, C], b1 [R],
    W2 [C, R], b2 [C] (`n_each` = 4) or W1, W2 (`n_each` = 2); 1x1 convolution weights [.., .., 1, 1]
    are taken as they are.  A modality given as None is passed as NULL pointers."""
    R = C // 16
    shapes = ((R, C), (R,), (C, R), (C,)) if n_each == 4 else ((R, C), (C, R))
    keep, flat = [], []
    for m, group in enumerate(params):
        if group is None:
            flat.extend([None] * n_each)
            continue
        if len(group) != n_each:
            raise TypeError(f'{n_each} parameter tensors per modality, got {len(group)}')
        for t, shape in zip(group, shapes):
            _require_on_device(t, 'params')
            if t.dtype != torch.float32 or t.numel() != int(np.prod(shape)) or tuple(t.shape[:len(shape)]) != shape:
                raise TypeError(f'parameter of modality {m} must be float32 {shape}, got {t.dtype} {tuple(t.shape)}')
            t = t.detach().contiguous()
            keep.append(t)
            flat.append(t)
    return keep, _ptr_array(flat)


def sefuse_squeeze(x_rgb: torch.Tensor, x_depth: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """s float32 [2, B, C]: the plane means of `x_rgb` (s[0]) and `x_depth` (s[1]), both [B, C, H, W] of
    one dtype (float32 / bfloat16 / float16) on the device, in one launch (include/nmsa.h
    nmsa_sefuse_squeeze): float32 sums in a fixed order, no atomics."""
    code, (B, C, H, W), (xr, xd) = _sefuse_maps(x_rgb, (x_depth,), ('x_rgb', 'x_depth'))
    s = _out(out, (2, B, C), torch.float32, xr.device)
    L.check(L.lib().nmsa_sefuse_squeeze(L.ptr(xr), L.ptr(xd), code, B, C, H, W, L.ptr(s), L.stream_ptr(xr.device)),
            'nmsa_sefuse_squeeze')
    return s


def sefuse_excite(s: torch.Tensor, params_rgb, params_depth, act: str = 'relu', save_z1: bool = False):
    """w float32 [2, B, C] = sigmoid(W2 act(W1 s + b1) + b2) per modality from the squeeze `s` [2, B, C]
    in one launch (nmsa_sefuse_excite).  `params_*`: (W1 [C//16, C], b1, W2 [C, C//16], b2) float32 on the
    device (the 1x1 convolution weights as they are); `act` 'relu' or 'silu'.  With `save_z1` returns
    (w, z1), z1 float32 [2, B, C//16] the hidden pre-activation `sefuse_excite_backward` takes."""
    a = _choice(act, _SEFUSE_ACTS, 'act')
    _require_on_device(s, 's')
    if s.ndim != 3 or s.shape[0] != 2 or s.dtype != torch.float32 or s.numel() == 0:
        raise TypeError(f's must be a non-empty float32 [2, B, C] tensor, got {s.dtype} {tuple(s.shape)}')
    B, C = int(s.shape[1]), int(s.shape[2])
    if C < 16:
        raise ValueError(f'the SE weighting needs at least 16 channels, got {C}')
    sc = s.detach().contiguous()
    keep, ptrs = _sefuse_params((params_rgb, params_depth), C, sc.device, 4)
    if len(keep) != 8:
        raise TypeError('the parameters of both modalities are needed')
    w = torch.empty((2, B, C), dtype=torch.float32, device=sc.device)
    z1 = torch.empty((2, B, C // 16), dtype=torch.float32, device=sc.device) if save_z1 else None
    L.check(L.lib().nmsa_sefuse_excite(L.ptr(sc), ptrs, a, B, C, L.ptr(w), L.ptr(z1), L.stream_ptr(sc.device)),
            'nmsa_sefuse_excite')
    return (w, z1) if save_z1 else w


def sefuse_scale_add(x_rgb: torch.Tensor, x_depth: torch.Tensor, w: torch.Tensor,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x_rgb * w[0][:, :, None, None] + x_depth * w[1][:, :, None, None] in one launch
    (nmsa_sefuse_scale_add): float32 arithmetic, one rounding to the maps' dtype.  `w` float32
    [2, B, C]; written into `out` when a contiguous tensor of the maps' shape and dtype is given."""
    code, (B, C, H, W), (xr, xd) = _sefuse_maps(x_rgb, (x_depth,), ('x_rgb', 'x_depth'))
    wc = _f32(w, (2, B, C), 'w')
    y = _out(out, (B, C, H, W), xr.dtype, xr.device)
    L.check(L.lib().nmsa_sefuse_scale_add(L.ptr(xr), L.ptr(xd), code, L.ptr(wc), B, C, H, W, L.ptr(y),
                                          L.stream_ptr(xr.device)), 'nmsa_sefuse_scale_add')
    return y


def sefuse_weight_grad(gy: torch.Tensor, x_rgb: Optional[torch.Tensor], x_depth: Optional[torch.Tensor],
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gw float32 [2, B, C]: the plane sums of gy * x_rgb (gw[0]) and gy * x_depth (gw[1]) from one read of
    `gy` in one launch (nmsa_sefuse_weight_grad); fixed order, no atomics.  A map given as None is not
    read and its half of gw is zero (left as it is in a given `out`)."""
    code, (B, C, H, W), (g, xr, xd) = _sefuse_maps(gy, (x_rgb, x_depth), ('gy', 'x_rgb', 'x_depth'))
    if out is not None:
        gw = _out(out, (2, B, C), torch.float32, g.device)
    elif xr is None or xd is None:
        gw = torch.zeros((2, B, C), dtype=torch.float32, device=g.device)
    else:
        gw = torch.empty((2, B, C), dtype=torch.float32, device=g.device)
    L.check(L.lib().nmsa_sefuse_weight_grad(L.ptr(g), L.ptr(xr), L.ptr(xd), code, B, C, H, W, L.ptr(gw),
                                            L.stream_ptr(g.device)), 'nmsa_sefuse_weight_grad')
    return gw


def sefuse_excite_backward(gw: torch.Tensor, w: torch.Tensor, z1: torch.Tensor, weights_rgb, weights_depth,
                           act: str = 'relu'):
    """(gz2 [2, B, C], gz1 [2, B, C//16], gs [2, B, C], h [2, B, C//16]) float32 of `sefuse_excite` for the
    weight gradient `gw` in one launch (nmsa_sefuse_excite_bwd): gz2 = gw w (1 - w), gz1 = (W2^T gz2)
    act'(z1), gs = W1^T gz1, h = act(z1).  `weights_*`: (W1, W2) of the modality, or None: that
    modality is not wanted and its halves are zero."""
    a = _choice(act, _SEFUSE_ACTS, 'act')
    _require_on_device(gw, 'gw')
    if gw.ndim != 3 or gw.shape[0] != 2 or gw.numel() == 0:
        raise TypeError(f'gw must be a non-empty float32 [2, B, C] tensor, got {tuple(gw.shape)}')
    B, C = int(gw.shape[1]), int(gw.shape[2])
    if C < 16:
        raise ValueError(f'the SE weighting needs at least 16 channels, got {C}')
    R = C // 16
    g = _f32(gw, (2, B, C), 'gw')
    wc = _f32(w, (2, B, C), 'w')
    z = _f32(z1, (2, B, R), 'z1')
    keep, ptrs = _sefuse_params((weights_rgb, weights_depth), C, g.device, 2)
    make = torch.empty if len(keep) == 4 else torch.zeros
    gz2, gs = (make((2, B, C), dtype=torch.float32, device=g.device) for _ in range(2))
    gz1, h = (make((2, B, R), dtype=torch.float32, device=g.device) for _ in range(2))
    L.check(L.lib().nmsa_sefuse_excite_bwd(L.ptr(g), L.ptr(wc), L.ptr(z), ptrs, a, B, C, L.ptr(gz2), L.ptr(gz1),
                                           L.ptr(gs), L.ptr(h), L.stream_ptr(g.device)), 'nmsa_sefuse_excite_bwd')
    return gz2, gz1, gs, h


def sefuse_apply_backward(gy: torch.Tensor, w: torch.Tensor, gs: torch.Tensor, need_rgb: bool = True,
                          need_depth: bool = True, out_rgb: Optional[torch.Tensor] = None,
                          out_depth: Optional[torch.Tensor] = None):
    """(gx_rgb, gx_depth), gx_m = gy * w[m] + gs[m] / (H * W), in gy's dtype in one launch
    (nmsa_sefuse_apply_bwd); None for a modality that is not needed."""
    code, (B, C, H, W), (g,) = _sefuse_maps(gy, (), ('gy',))
    wc = _f32(w, (2, B, C), 'w')
    gsc = _f32(gs, (2, B, C), 'gs')
    gxr = _out(out_rgb, (B, C, H, W), g.dtype, g.device, 'out_rgb') if need_rgb else None
    gxd = _out(out_depth, (B, C, H, W), g.dtype, g.device, 'out_depth') if need_depth else None
    if need_rgb or need_depth:
        L.check(L.lib().nmsa_sefuse_apply_bwd(L.ptr(g), code, L.ptr(wc), L.ptr(gsc), B, C, H, W, L.ptr(gxr),
                                              L.ptr(gxd), L.stream_ptr(g.device)), 'nmsa_sefuse_apply_bwd')
    return gxr, gxd


def sefuse_route(*tensors: torch.Tensor) -> int:
    """The routes a map call of the SE-weighted add takes with these 1..3 [B, C, H, W] tensors
    (`nmsa_sefuse_route`): L.NMSA_SEFUSE_ROUTE_VECTOR or _ELEMENT (16-byte accesses: H*W a multiple of
    4 float32 / 8 half elements and every tensor on 16 bytes), or-ed with L.NMSA_SEFUSE_ROUTE_WAVE or
    _BLOCK (how the squeeze and the weight gradient cut a plane: one wave up to
    L.NMSA_SEFUSE_WAVE_PLANE_MAX elements, one workgroup above).  Host only, nothing is launched."""
    if not 1 <= len(tensors) <= 3 or any(t.ndim != 4 for t in tensors):
        raise ValueError('1..3 [B, C, H, W] tensors')
    ptrs = [t.data_ptr() for t in tensors] + [None] * (3 - len(tensors))
    return _route('nmsa_sefuse_route', *ptrs, L.float_dtype_code(tensors[0]), int(tensors[0].shape[2]),
                  int(tensors[0].shape[3]))


# ------------------------------------------------------- residual blocks: the fused batch-norm tail
_BNTAIL_ACTS = {'relu': L.NMSA_BNTAIL_ACT_RELU, 'silu': L.NMSA_BNTAIL_ACT_SILU}


def _bntail_maps(first: torch.Tensor, others, names):
    """dtype code, (B, C, H, W) and the detached maps of a call: `first` sets device, dtype and shape, every
    tensor of `others` (None allowed) must match it; all must be dense NCHW"""
    code = _float_map(first, names[0], dense=True)
    shape = tuple(int(n) for n in first.shape)
    maps = [first]
    for t, name in zip(others, names[1:]):
        maps.append(_like(t, shape, first.dtype, first.device, name, dense=True))
    return code, shape, maps


def _bntail_scale(scale: Optional[torch.Tensor], like: torch.Tensor) -> Optional[torch.Tensor]:
    if scale is None:
        return None
    B, C = int(like.shape[0]), int(like.shape[1])
    _require_on_device(scale, 'scale')
    if scale.dtype != like.dtype or scale.numel() != B * C or tuple(scale.shape[:2]) != (B, C):
        raise TypeError(f'scale must be {like.dtype} [{B}, {C}] (or [{B}, {C}, 1, 1]), got {scale.dtype} '
                        f'{tuple(scale.shape)}')
    return scale.detach().contiguous()


def bntail_workspace_bytes(shape) -> int:
    return int(L.lib().nmsa_bntail_workspace_bytes(*(int(n) for n in shape)))


def _bntail_part(part: Optional[torch.Tensor], shape, dev) -> Tuple[torch.Tensor, int]:
    """the unit partials of a shape: the caller's float32 tensor, or the cached workspace of the stream"""
    nbytes = bntail_workspace_bytes(shape)
    if part is None:
        return _workspace(dev, ('bntail',) + tuple(shape), nbytes)
    _require_on_device(part, 'part')
    if part.dtype != torch.float32 or not part.is_contiguous() or part.numel() * 4 < nbytes:
        raise TypeError(f'part must be a contiguous float32 tensor of at least {nbytes} bytes')
    return part, part.numel() * 4


def bntail_stats(x: torch.Tensor, part: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The batch statistics of `x` [B, C, H, W] (float32 / bfloat16 / float16, dense NCHW) as per-unit
    partials (mean_u, M2_u) in one launch (include/nmsa.h nmsa_bntail_stats): a flat float32 workspace whose
    first C * U * 2 values are [C, U, 2], U = B * ceil(H*W / L.NMSA_BNTAIL_SEGMENT).  `bntail_apply` merges them.
    Two passes over registers per unit, Chan's merge between units: no E[x^2] - E[x]^2, no atomics."""
    code, shape, (xc,) = _bntail_maps(x, (), ('x',))
    ws, nbytes = _bntail_part(part, shape, xc.device)
    L.check(L.lib().nmsa_bntail_stats(L.ptr(xc), code, *shape, L.ptr(ws), nbytes, L.stream_ptr(xc.device)),
            'nmsa_bntail_stats')
    return ws


def bntail_apply(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, running_mean: torch.Tensor,
                 running_var: torch.Tensor, eps: float, momentum: float = 0.0, act: str = 'relu',
                 part: Optional[torch.Tensor] = None, identity: Optional[torch.Tensor] = None,
                 scale: Optional[torch.Tensor] = None, save: bool = False, out: Optional[torch.Tensor] = None):
    """y = act(((x - mean) * invstd * gamma + beta) * scale[b, c] + identity) in one launch (nmsa_bntail_apply).
    `part` given (the result of `bntail_stats(x)`): training, the batch statistics; `running_mean` and
    `running_var` (float32 [C]) are UPDATED in place with `momentum`.  `part` None: eval, they are read.
    `identity` (x's shape and dtype) and `scale` ([B, C] of x's dtype, the Dropout2d scale) are optional.
    With `save` returns (y, mean, invstd), the float32 [C] statistics `bntail_backward_*` take."""
    a = _choice(act, _BNTAIL_ACTS, 'act')
    code, shape, (xc, idc) = _bntail_maps(x, (identity,), ('x', 'identity'))
    B, C, H, W = shape
    if part is not None and B * H * W < 2:
        raise ValueError(f'Expected more than 1 value per channel when training, got input size {list(shape)}')
    sc = _bntail_scale(scale, xc)
    g, b = _f32(gamma, (C,), 'gamma', dense=True), _f32(beta, (C,), 'beta', dense=True)
    rm = _f32(running_mean, (C,), 'running_mean', dense=True)
    rv = _f32(running_var, (C,), 'running_var', dense=True)
    y = _out(out, shape, xc.dtype, xc.device)
    mean = torch.empty((C,), dtype=torch.float32, device=xc.device) if save else None
    invstd = torch.empty((C,), dtype=torch.float32, device=xc.device) if save else None
    nbytes = 0
    if part is not None:
        part, nbytes = _bntail_part(part, shape, xc.device)
    L.check(L.lib().nmsa_bntail_apply(L.ptr(xc), L.ptr(idc), L.ptr(sc), code, B, C, H, W, L.ptr(g), L.ptr(b),
                                      L.ptr(part), nbytes, L.ptr(rm), L.ptr(rv), float(eps), float(momentum), a,
                                      L.ptr(mean), L.ptr(invstd), L.ptr(y), L.stream_ptr(xc.device)),
            'nmsa_bntail_apply')
    return (y, mean, invstd) if save else y


def _bntail_bwd_args(gy, x, aux, scale, gamma, beta, mean, invstd, act):
    a = _choice(act, _BNTAIL_ACTS, 'act')
    code, shape, (g, xc, ac) = _bntail_maps(gy, (x, aux), ('gy', 'x', 'aux'))
    if xc is None or (a == L.NMSA_BNTAIL_ACT_RELU and ac is None):
        raise TypeError("x is needed, and under 'relu' aux (the saved output y)")
    C = shape[1]
    vecs = [_f32(t, (C,), n, dense=True)
            for t, n in ((gamma, 'gamma'), (beta, 'beta'), (mean, 'mean'), (invstd, 'invstd'))]
    head = (L.ptr(g), L.ptr(xc), L.ptr(ac), L.ptr(_bntail_scale(scale, g)), code, *shape,
            *(L.ptr(v) for v in vecs), a)
    return head, shape, g, (xc, ac, vecs)


def bntail_backward_reduce(gy: torch.Tensor, x: torch.Tensor, aux: Optional[torch.Tensor], gamma: torch.Tensor,
                           beta: Optional[torch.Tensor], mean: torch.Tensor, invstd: torch.Tensor, act: str = 'relu',
                           scale: Optional[torch.Tensor] = None, finish: bool = False,
                           part: Optional[torch.Tensor] = None):
    """The per-unit partials (sum gu, sum gu * xh) of the tail's backward pass in one launch
    (nmsa_bntail_bwd_reduce); `aux` is the saved output y under 'relu' and the identity (or None) under
    'silu'.  Returns the workspace `bntail_backward_apply` merges, or with `finish` (dgamma, dbeta) float32 [C],
    merged by the launch itself in the same order (a backward pass without a map gradient, eval mode)."""
    head, shape, g, keep = _bntail_bwd_args(gy, x, aux, scale, gamma, beta, mean, invstd, act)
    ws, nbytes = _bntail_part(part, shape, g.device)
    dgamma = torch.empty((shape[1],), dtype=torch.float32, device=g.device) if finish else None
    dbeta = torch.empty((shape[1],), dtype=torch.float32, device=g.device) if finish else None
    L.check(L.lib().nmsa_bntail_bwd_reduce(*head, L.ptr(ws), nbytes, L.ptr(dgamma), L.ptr(dbeta),
                                           L.stream_ptr(g.device)), 'nmsa_bntail_bwd_reduce')
    return (dgamma, dbeta) if finish else ws


def bntail_backward_apply(gy: torch.Tensor, x: torch.Tensor, aux: Optional[torch.Tensor], gamma: torch.Tensor,
                          beta: Optional[torch.Tensor], mean: torch.Tensor, invstd: torch.Tensor, act: str = 'relu',
                          scale: Optional[torch.Tensor] = None, part: Optional[torch.Tensor] = None,
                          need_x: bool = True, need_identity: bool = False, need_params: bool = False,
                          out_x: Optional[torch.Tensor] = None, out_identity: Optional[torch.Tensor] = None):
    """(gx, gid, dgamma, dbeta) of the tail in one launch (nmsa_bntail_bwd_apply); None for what is not
    needed.  `part` (the result of `bntail_backward_reduce`): the training formula, and with `need_params`
    the merged dgamma, dbeta; `part` None: the eval formula gx = gamma * invstd * gu (`need_params` must be
    False: take them from `bntail_backward_reduce(..., finish=True)`)."""
    head, shape, g, keep = _bntail_bwd_args(gy, x, aux, scale, gamma, beta, mean, invstd, act)
    if need_params and part is None:
        raise ValueError('dgamma and dbeta need the partials of bntail_backward_reduce')
    nbytes = 0
    if part is not None:
        part, nbytes = _bntail_part(part, shape, g.device)
    gx = _out(out_x, shape, g.dtype, g.device, 'out_x') if need_x else None
    gid = _out(out_identity, shape, g.dtype, g.device, 'out_identity') if need_identity else None
    dgamma = torch.empty((shape[1],), dtype=torch.float32, device=g.device) if need_params else None
    dbeta = torch.empty((shape[1],), dtype=torch.float32, device=g.device) if need_params else None
    if need_x or need_identity or need_params:
        L.check(L.lib().nmsa_bntail_bwd_apply(*head, L.ptr(part), nbytes, L.ptr(gx), L.ptr(gid), L.ptr(dgamma),
                                              L.ptr(dbeta), L.stream_ptr(g.device)), 'nmsa_bntail_bwd_apply')
    return gx, gid, dgamma, dbeta


def bntail_route(*tensors: torch.Tensor) -> Tuple[int, int]:
    """(route, segments) of a call of the fused batch-norm tail with these 1..5 [B, C, H, W] maps
    (`nmsa_bntail_route`): L.NMSA_BNTAIL_ROUTE_VECTOR (16-byte accesses: H*W a multiple of 4 float32 / 8 half
    elements and every map on 16 bytes) or _ELEMENT, and the units a plane is cut into
    (ceil(H*W / L.NMSA_BNTAIL_SEGMENT)).  Host only, nothing is launched."""
    if not 1 <= len(tensors) <= 5 or any(t.ndim != 4 for t in tensors):
        raise ValueError('1..5 [B, C, H, W] tensors')
    ptrs = [t.data_ptr() for t in tensors] + [None] * (5 - len(tensors))
    seg = L.C.c_int(0)
    rc = _route('nmsa_bntail_route', *ptrs, L.float_dtype_code(tensors[0]), int(tensors[0].shape[2]),
                int(tensors[0].shape[3]), L.C.byref(seg))
    return rc, seg.value


# ------------------------------------------------------------- the stem max pool of the ResNet backbones
def maxpool3x3s2_out_shape(shape) -> Tuple[int, int, int, int]:
    B, C, H, W = (int(n) for n in shape)
    return B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1


def maxpool3x3s2(x: torch.Tensor, need_code: bool = True, out: Optional[torch.Tensor] = None):
    """`F.max_pool2d(x, 3, 2, 1)` in one launch (include/nmsa.h nmsa_maxpool3x3s2_fwd).  `x` [B, C, H, W] float32
    / bfloat16 / float16, dense NCHW on the device.  Returns (y, code): y [B, C, Ho, Wo] in x's dtype carries the
    selected elements' bits (ATen's selection rule: first maximum, last NaN); code uint8 of y's shape is the
    window position 0..8 of the selected pixel, what `maxpool3x3s2_backward` reads in place of ATen's int64 index.
    Without `need_code` (inference) none is allocated or written and None is returned for it.  No autograd:
    that is `model.pooling.MaxPool3x3S2Function`."""
    code = _float_map(x, 'x', dense=True)
    xc = x.detach()
    B, C, H, W = (int(n) for n in xc.shape)
    oshape = maxpool3x3s2_out_shape(xc.shape)
    y = _out(out, oshape, xc.dtype, xc.device)
    k = torch.empty(oshape, dtype=torch.uint8, device=xc.device) if need_code else None
    L.check(L.lib().nmsa_maxpool3x3s2_fwd(L.ptr(xc), code, B, C, H, W, L.ptr(y), L.ptr(k), L.stream_ptr(xc.device)),
            'nmsa_maxpool3x3s2_fwd')
    return y, k


def maxpool3x3s2_backward(gy: torch.Tensor, code: torch.Tensor, input_hw: Tuple[int, int],
                          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gx [B, C, H, W] of `maxpool3x3s2` for the upstream gradient `gy` [B, C, Ho, Wo] and the forward's `code`
    in one launch (nmsa_maxpool3x3s2_bwd): a gather, every element written, float32 sums in a fixed order
    (oy, then ox, ascending) rounded once: the same bits on every call."""
    dcode = _float_map(gy, 'gy', dense=True)
    H, W = (int(n) for n in input_hw)
    B, C = int(gy.shape[0]), int(gy.shape[1])
    oshape = maxpool3x3s2_out_shape((B, C, H, W))
    k = _like(code, oshape, torch.uint8, gy.device, 'code', dense=True)
    if tuple(gy.shape) != oshape:
        raise TypeError(f'gy must be {oshape} for an input of {H}x{W}, got {tuple(gy.shape)}')
    g = gy.detach()
    gx = _out(out, (B, C, H, W), g.dtype, g.device)
    L.check(L.lib().nmsa_maxpool3x3s2_bwd(L.ptr(g), L.ptr(k), dcode, B, C, H, W, L.ptr(gx), L.stream_ptr(g.device)),
            'nmsa_maxpool3x3s2_bwd')
    return gx


def maxpool3x3s2_route(x: torch.Tensor, *others: torch.Tensor) -> int:
    """The route a call with these tensors takes (`nmsa_maxpool3x3s2_route`, asked once per other tensor):
    L.NMSA_MP_ROUTE_VECTOR when every answer is, else L.NMSA_MP_ROUTE_PIXEL.  `x` [B, C, H, W] is an
    input-sized tensor of the call (x or gx), `others` its remaining tensors (y and code; gy and code).  Only
    shapes, the dtype and the addresses are looked at, nothing is launched."""
    if x.ndim != 4 or not others:
        raise ValueError('an input-sized [B, C, H, W] tensor and at least one more tensor of the call')
    B, C, H, W = (int(n) for n in x.shape)
    route = L.NMSA_MP_ROUTE_VECTOR
    for t in others:
        if _route('nmsa_maxpool3x3s2_route', x.data_ptr(), t.data_ptr(), L.float_dtype_code(x), B, C, H,
                  W) != L.NMSA_MP_ROUTE_VECTOR:
            route = L.NMSA_MP_ROUTE_PIXEL
    return route


# ------------------------------------------------------------- the scene classification decoder
def _sh_params(weight: torch.Tensor, bias: Optional[torch.Tensor], C: int):
    """-> (K, weight, bias) of a linear layer over C channels: float32 [K, C] and [K] (or None), dense"""
    K = int(weight.shape[0]) if weight.ndim == 2 else -1            # -1: no [K, C] at all, refused below
    return K, _f32(weight, (K, C), 'weight', dense=True), _f32(bias, (K,), 'bias', dense=True)


def scene_head(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], need_pooled: bool = True,
               out_dtype: Optional[torch.dtype] = None):
    """`F.linear(F.adaptive_avg_pool2d(x, 1).flatten(1), weight, bias)` in one launch (include/nmsa.h
    nmsa_scene_head_fwd).  `x` [B, C, H, W] float32 / bfloat16 / float16, dense NCHW on the device; `weight`
    float32 [K, C], `bias` float32 [K] or None.  Returns (logits, pooled): logits [B, K] in `out_dtype` (x's
    dtype when None), pooled float32 [B, C], what `scene_head_backward` reads in place of the map.  Without
    `need_pooled` (inference) none is allocated or written and None is returned for it.  No autograd: that is
    `model.decoder.SceneHeadFunction`."""
    code = _float_map(x, 'x', dense=True)
    xc = x.detach()
    B, C, H, W = (int(n) for n in xc.shape)
    K, w_, b_ = _sh_params(weight, bias, C)
    out_dtype = xc.dtype if out_dtype is None else out_dtype
    ocode = L.float_code_of_dtype(out_dtype, 'out_dtype')
    logits = torch.empty((B, K), dtype=out_dtype, device=xc.device)
    pooled = torch.empty((B, C), dtype=torch.float32, device=xc.device) if need_pooled else None
    L.check(L.lib().nmsa_scene_head_fwd(L.ptr(xc), code, B, C, H, W, L.ptr(w_), L.ptr(b_), L.ptr(pooled),
                                        L.ptr(logits), ocode, K, L.stream_ptr(xc.device)),
            'nmsa_scene_head_fwd')
    return logits, pooled


def scene_head_backward(g: torch.Tensor, pooled: torch.Tensor, weight: torch.Tensor, x_shape, x_dtype: torch.dtype,
                        need=(True, True, True)):
    """(gx, gweight, gbias) of `scene_head` for the upstream gradient `g` [B, K] (float32 / bfloat16 / float16),
    the forward's `pooled` and `weight`, in one launch (nmsa_scene_head_bwd): gx [B, C, H, W] in `x_dtype`,
    gweight float32 [K, C], gbias float32 [K]; None where `need` says the gradient is not wanted (nothing is
    allocated or computed for it).  Every sum runs in a fixed order: the same bits on every call."""
    _require_on_device(g, 'g')
    B, C, H, W = (int(n) for n in x_shape)
    gcode = L.float_code_of_dtype(g.dtype, 'g')
    xcode = L.float_code_of_dtype(x_dtype, 'x_dtype')
    K, w_, _ = _sh_params(weight, None, C)
    p_ = _f32(pooled, (B, C), 'pooled', dense=True)
    if tuple(g.shape) != (B, K) or not g.is_contiguous() or min(B, C, H, W) < 1:
        raise TypeError(f'g must be contiguous [{B}, {K}] for a non-empty map, got {tuple(g.shape)}')
    gd = g.detach()
    dev = gd.device
    gx = torch.empty((B, C, H, W), dtype=x_dtype, device=dev) if need[0] else None
    gw = torch.empty((K, C), dtype=torch.float32, device=dev) if need[1] else None
    gb = torch.empty((K,), dtype=torch.float32, device=dev) if need[2] else None
    L.check(L.lib().nmsa_scene_head_bwd(L.ptr(gd), gcode, L.ptr(p_), L.ptr(w_), B, C, H, W, K, L.ptr(gx), xcode,
                                        L.ptr(gw), L.ptr(gb), L.stream_ptr(dev)), 'nmsa_scene_head_bwd')
    return gx, gw, gb


def scene_head_route(x: torch.Tensor, n_classes: int = 1) -> int:
    """The route a call whose map (x forward, gx backward) is `x` [B, C, H, W] takes (`nmsa_scene_head_route`):
    L.NMSA_SH_ROUTE_UNIT, L.NMSA_SH_ROUTE_VECTOR or L.NMSA_SH_ROUTE_ELEMENT.  Only the shape, the dtype and the
    address are looked at, nothing is launched."""
    if x.ndim != 4:
        raise ValueError('a [B, C, H, W] map')
    B, C, H, W = (int(n) for n in x.shape)
    return _route('nmsa_scene_head_route', x.data_ptr(), L.float_dtype_code(x), B, C, H, W, int(n_classes))


# ------------------------------------------------------------- orientation MAE on device tables
def _orientation_table_args(table, name: str, B: int) -> tuple:
    """(keys, angle, valid, n, K, status) of a utils.OrientationTable as the C ABI takes them"""
    if table.batch_size != B:
        raise ValueError(f'{name} holds {table.batch_size} images, expected {B}')
    tensors = [table.keys, table.angle, table.valid, table.n, table.status]
    for t in tensors:
        if t is not None:
            _require_on_device(t, name)
    keys, angle, valid, n, status = (None if t is None else t.contiguous() for t in tensors)
    held = (keys, angle, valid, n, status)
    return held, (L.ptr(keys), L.ptr(angle), L.ptr(valid), L.ptr(n), int(angle.shape[1]), L.ptr(status))


def _id_table_args(table, name: str, B: int) -> tuple:
    if table.batch_size != B:
        raise ValueError(f'{name} holds {table.batch_size} images, expected {B}')
    for t in (table.pan, table.ins, table.n):
        _require_on_device(t, name)
    pan, ins, n = table.pan.contiguous(), table.ins.contiguous(), table.n.contiguous()
    return (pan, ins, n), (L.ptr(pan), L.ptr(ins), L.ptr(n), int(pan.shape[1]), int(table.ascending))


def _maae_states(sum_state, count_state, status) -> None:
    for name, t in (('sum_state', sum_state), ('count_state', count_state), ('status', status)):
        _require_on_device(t, name)
    if sum_state.dtype != torch.float64 or count_state.dtype != torch.int64 or \
            status.dtype != torch.int32 or sum_state.numel() != 1 or count_state.numel() != 1:
        raise TypeError('the states are one float64 and one int64 element, the status an int32 word')


def maae_update_keyed(sum_state: torch.Tensor, count_state: torch.Tensor, status: torch.Tensor,
                      preds, target) -> None:
    """reference: `MeanAbsoluteAngularError.update` (metric/mae.py:40-64) on two
    `utils.OrientationTable`s, into the metric's device states: no host sync.  A prediction key
    the target lacks raises status bit 64 (the reference's KeyError) and is skipped."""
    _maae_states(sum_state, count_state, status)
    B = preds.batch_size
    if B == 0:
        return
    held_p, args_p = _orientation_table_args(preds, 'preds', B)
    held_t, args_t = _orientation_table_args(target, 'target', B)
    L.check(L.lib().nmsa_maae_update_keyed(
        *args_p, *args_t, B, L.ptr(sum_state), L.ptr(count_state), L.ptr(status),
        L.stream_ptr(sum_state.device)), 'nmsa_maae_update_keyed')


def maae_update_matched(sum_state: torch.Tensor, count_state: torch.Tensor, status: torch.Tensor,
                        matches: torch.Tensor, n_matches: torch.Tensor,
                        pred_ids, preds, target_ids, target) -> None:
    """reference: `PanopticQualityWithOrientationMAE.update_mae` (metric/mae.py:129-162) for every
    image of a batch: `matches` i64 [B,cap,2] / `n_matches` i32 [B] as `nmsa_pq_update` leaves
    them, `utils.IdTable`s and `utils.OrientationTable`s of both sides.  More matches than `cap`
    raise status bit 128; the image then contributes its first `cap` rows."""
    _maae_states(sum_state, count_state, status)
    _require_on_device(matches, 'matches')
    _require_on_device(n_matches, 'n_matches')
    if matches.dtype != torch.int64 or n_matches.dtype != torch.int32 or matches.ndim != 3 or \
            matches.shape[2] != 2 or n_matches.shape != matches.shape[:1]:
        raise TypeError('matches is int64 [B, cap, 2], n_matches int32 [B]')
    B, cap = int(matches.shape[0]), int(matches.shape[1])
    if B == 0:
        return
    m, nm = matches.contiguous(), n_matches.contiguous()
    held_pi, args_pi = _id_table_args(pred_ids, 'pred_ids', B)
    held_p, args_p = _orientation_table_args(preds, 'preds', B)
    held_ti, args_ti = _id_table_args(target_ids, 'target_ids', B)
    held_t, args_t = _orientation_table_args(target, 'target', B)
    L.check(L.lib().nmsa_maae_update_matched(
        L.ptr(m), L.ptr(nm), cap, *args_pi, *args_p, *args_ti, *args_t, B,
        L.ptr(sum_state), L.ptr(count_state), L.ptr(status), L.stream_ptr(sum_state.device)),
        'nmsa_maae_update_matched')


# ----------------------------------------------------------------------------- a5
def panoptic_merge(
    semantic: torch.Tensor,
    instance: torch.Tensor,
    thing_seg: torch.Tensor,
    is_thing_class: torch.Tensor,           # u8/bool [n_classes] (class VALUE domain)
    max_instances_per_category: int,
    void_label: int = 0,
) -> Dict[str, torch.Tensor]:
    """reference: deeplab_merge_batch (panoptic_merge.py:18-40,172-225)"""
    sem = L.require_device_tensor(semantic, 'semantic')
    ins = L.require_device_tensor(instance, 'instance')
    if sem.dtype == torch.bool:
        sem = sem.view(torch.uint8)
    B, H, W = sem.shape
    dev = sem.device
    thing = _u8(thing_seg)
    lut = _u8(is_thing_class)
    n_classes = int(lut.numel())
    votes = torch.empty((B, 256, n_classes), dtype=torch.int32, device=dev)
    pan_of_inst = torch.empty((B, 256), dtype=torch.int64, device=dev)
    pan = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    ids_pan = torch.empty((B, 256), dtype=torch.int64, device=dev)
    ids_ins = torch.empty((B, 256), dtype=torch.int64, device=dev)
    n_ids = torch.empty((B,), dtype=torch.int32, device=dev)
    L.check(L.lib().nmsa_panoptic_merge(
        L.ptr(sem), L.int_dtype_code(sem), L.ptr(ins), L.int_dtype_code(ins), L.ptr(thing),
        L.ptr(lut), B, n_classes, H, W, int(max_instances_per_category), int(void_label),
        L.ptr(votes), L.ptr(pan_of_inst), L.ptr(pan), L.ptr(ids_pan), L.ptr(ids_ins),
        L.ptr(n_ids), L.stream_ptr(dev)), 'nmsa_panoptic_merge')
    return {'panoptic': pan, 'ids_pan': ids_pan, 'ids_ins': ids_ins, 'n_ids': n_ids}


def panoptic_merge_wide(
    semantic: torch.Tensor,
    instance: torch.Tensor,
    thing_seg: torch.Tensor,
    is_thing_class: torch.Tensor,
    max_instances_per_category: int,
    void_label: int = 0,
    max_segments: int = 1024,
) -> Dict[str, torch.Tensor]:
    """deeplab_merge_batch for instance ids 0..65535 (ground-truth maps)."""
    sem = L.require_device_tensor(semantic, 'semantic')
    ins = L.require_device_tensor(instance, 'instance')
    B, H, W = sem.shape
    dev = sem.device
    thing = _u8(thing_seg)
    lut = _u8(is_thing_class)
    n_classes = int(lut.numel())
    cap = ((max_segments + 1023) // 1024) * 1024
    pan = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    ids_pan = torch.empty((B, cap), dtype=torch.int64, device=dev)
    ids_ins = torch.empty((B, cap), dtype=torch.int64, device=dev)
    n_ids = torch.empty((B,), dtype=torch.int32, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws_bytes = L.lib().nmsa_panoptic_merge_wide_workspace_bytes(B, n_classes, max_segments)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    L.check(L.lib().nmsa_panoptic_merge_wide(
        L.ptr(sem), L.int_dtype_code(sem), L.ptr(ins), L.int_dtype_code(ins), L.ptr(thing),
        L.ptr(lut), B, n_classes, H, W, int(max_instances_per_category), int(void_label),
        int(max_segments), L.ptr(pan), L.ptr(ids_pan), L.ptr(ids_ins), L.ptr(n_ids), L.ptr(status),
        L.ptr(ws), ws_bytes, L.stream_ptr(dev)), 'nmsa_panoptic_merge_wide')
    return {'panoptic': pan, 'ids_pan': ids_pan, 'ids_ins': ids_ins, 'n_ids': n_ids,
            'status': status}


# ------------------------------------------------------------------------- next-1
def instance_orientation_sums(
    orientation: torch.Tensor,
    instance: torch.Tensor,
    mask: Optional[torch.Tensor] = None,
) -> Dict[str, torch.Tensor]:
    """reference: InstancePostprocessing._get_instance_orientation (instance.py:271-319)"""
    o = L.require_device_tensor(orientation, 'orientation')
    if o.dtype != torch.float32:
        o = o.float()
    ins = L.require_device_tensor(instance, 'instance')
    assert ins.dtype == torch.uint8
    B, two, H, W = o.shape
    dev = o.device
    sums = torch.empty((B, 256, 2), dtype=torch.float64, device=dev)
    count = torch.empty((B, 256), dtype=torch.int32, device=dev)
    L.check(L.lib().nmsa_instance_orientation(
        L.ptr(o), L.ptr(ins), L.ptr(_u8(mask)), B, H, W, L.ptr(sums), L.ptr(count),
        L.stream_ptr(dev)), 'nmsa_instance_orientation')
    return {'sums': sums, 'count': count}


def instance_orientation_sums_wide(
    orientation: torch.Tensor,
    instance: torch.Tensor,
    mask: Optional[torch.Tensor] = None,
    max_instances: int = 1024,
) -> Dict[str, torch.Tensor]:
    """`instance_orientation_sums` for ground-truth instance maps (ids 0..65535, any integer
    dtype): sums / counts by position in the ascending `ids` list."""
    o = L.require_device_tensor(orientation, 'orientation')
    if o.dtype != torch.float32:
        o = o.float()
    ins = L.require_device_tensor(instance, 'instance')
    B, two, H, W = o.shape
    dev = o.device
    cap = ((int(max_instances) + 1023) // 1024) * 1024
    ids = torch.empty((B, cap), dtype=torch.int32, device=dev)
    n_ids = torch.empty((B,), dtype=torch.int32, device=dev)
    sums = torch.empty((B, cap, 2), dtype=torch.float64, device=dev)
    count = torch.empty((B, cap), dtype=torch.int32, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws, ws_bytes, _ = _targets_workspace(B, 1, int(max_instances), dev)
    L.check(L.lib().nmsa_instance_orientation_wide(
        L.ptr(o), L.ptr(ins), L.int_dtype_code(ins), L.ptr(_u8(mask)), B, H, W, int(max_instances),
        L.ptr(ids), L.ptr(n_ids), L.ptr(sums), L.ptr(count), L.ptr(status), L.ptr(ws), ws_bytes,
        L.stream_ptr(dev)), 'nmsa_instance_orientation_wide')
    return {'ids': ids, 'n_ids': n_ids, 'sums': sums, 'count': count, 'status': status}
