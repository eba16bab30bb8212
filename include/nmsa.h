/*
 * nmsa.h — C ABI of libnmsa_hip.so: the MI355X (gfx950) implementation of the
 * dense-prediction hot path of nicr-mt-scene-analysis.
 *
 * The reference is pure Python (no FFI of its own); each entry point below names
 * the reference Python symbol whose ATen-op chain it replaces
 * (paths relative to src/nicr_mt_scene_analysis/ of the reference).  The Python
 * mirror of the reference API (package nicr_mt_scene_analysis_amd) binds these
 * with ctypes; INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (contiguous, NCHW /
 *    row-major as noted), unless the parameter name ends in _host;
 *  - all work is enqueued on `stream` (a hipStream_t); nothing synchronises,
 *    nothing allocates; scratch is passed in by the caller and sized with the
 *    matching *_workspace_bytes() query;
 *  - return value: NMSA_OK (0) or a negative NMSA_ERR_* code; nothing throws.
 *  - "bool" tensors are uint8 (torch.bool storage), 0 / non-0.
 */
#ifndef NMSA_H
#define NMSA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* nmsa_stream_t; /* hipStream_t */

enum {
    NMSA_OK = 0,
    NMSA_ERR_ARG = -1,         /* invalid argument (shape, null pointer, range)      */
    NMSA_ERR_LAUNCH = -2,      /* HIP launch / runtime error (see nmsa_last_hip_error) */
    NMSA_ERR_WORKSPACE = -3,   /* workspace too small                                  */
    NMSA_ERR_UNSUPPORTED = -4  /* valid in the reference, not implemented here        */
};

/* floating-point element types of prediction tensors */
enum { NMSA_F32 = 0, NMSA_BF16 = 1, NMSA_F16 = 2 };
/* integer element types of label / id tensors */
enum { NMSA_U8 = 0, NMSA_I16 = 1, NMSA_I32 = 2, NMSA_I64 = 3 };
/* nmsa_resize_nearest also moves f32 maps (scores): */
#define NMSA_ELEM_F32 8

#define NMSA_MAX_INSTANCE_IDS 256 /* instance ids are uint8 in the reference (instance.py:236) */

int nmsa_version(void);
const char* nmsa_strerror(int code);
int nmsa_last_hip_error(void); /* last hipError_t seen by this library (thread-local) */
/* What the library sizes its grids from: compute units, XCDs and LDS bytes per CU of the CURRENT
 * device, queried once per device from the HIP runtime (no literal 256 / 8: a partitioned MI355X
 * shows fewer).  The environment variables NMSA_ASSUME_CUS / NMSA_ASSUME_XCDS override the
 * queried numbers (tests).  Any pointer may be NULL.  Host pointers. */
int nmsa_device_geometry(int* cus_host, int* xcds_host, size_t* lds_per_cu_host);

/* ---------------------------------------------------------------------------
 * a2  InstancePostprocessing._get_instance_centers
 *     model/postprocessing/instance.py:79-168
 * threshold -> k x k max-pool NMS (first maximum in the window wins, border of
 * (k-1)/2 px never a center) -> per-image top-k value (before the optional
 * foreground mask) -> keep >= kth (ties kept) -> raster-ordered coordinates.
 *   center        f32 [B,H,W]           (the [B,1,H,W] head output)
 *   fg            u8  [B,H,W] or NULL   (required iff apply_fg)
 *   centers_yx    i32 [B,max_centers,2] (y,x) raster order, first n_centers[b] valid
 *   n_centers     i32 [B]  TRUE count (may exceed max_centers: caller re-runs larger)
 *   scores        f32 [B,max_centers]   raw heatmap value at each center (meta 'score')
 *   center_mask   u8  [B,H,W] or NULL   the boolean map the reference also returns
 * ------------------------------------------------------------------------- */
size_t nmsa_center_nms_workspace_bytes(int B, int H, int W);
int nmsa_center_nms_topk(const float* center, const uint8_t* fg,
                         int B, int H, int W,
                         float threshold, int ksize, int topk, int apply_fg,
                         int max_centers,
                         int32_t* centers_yx, int32_t* n_centers, float* scores,
                         uint8_t* center_mask,
                         void* workspace, size_t workspace_bytes,
                         nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * a3  InstancePostprocessing._get_instance_segmentation (grouping part)
 *     model/postprocessing/instance.py:187-253
 * For every foreground pixel: loc = (y,x) + offset*(scale_y,scale_x); id =
 * 1 + argmin_i ||center_i - loc||_2 (fp32, lowest index on ties, uint8 wrap);
 * optional `min_dist > dist_thr -> 0`.
 *   offset  f32 [B,2,H,W] (dy,dx); scale = (H,W) for normalized offsets, else 1
 *   inst    u8  [B,H,W]   (0 outside fg)
 *   area    i32 [B,256]   bincount of ids over fg (meta 'area'); may be NULL
 * ------------------------------------------------------------------------- */
int nmsa_group_offsets(const float* offset, const uint8_t* fg,
                       const int32_t* centers_yx, const int32_t* n_centers,
                       int B, int H, int W, int max_centers,
                       float scale_y, float scale_x,
                       int use_dist_thr, float dist_thr,
                       uint8_t* inst, int32_t* area,
                       nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * a1  SemanticPostprocessing._postprocess_inference (argmax + score)
 *     model/postprocessing/semantic.py:52-53
 *   logits  f32|bf16|f16 [B,C,H,W];  any of the outputs may be NULL
 *   idx_u8 [B,H,W] (C <= 256), idx_i64 [B,H,W], score f32 [B,H,W] = max softmax
 * ------------------------------------------------------------------------- */
int nmsa_semantic_argmax(const void* logits, int logits_dtype,
                         int B, int C, int H, int W,
                         uint8_t* idx_u8, int64_t* idx_i64, float* score,
                         nmsa_stream_t stream);

/* softmax over C (semantic.py:52 'semantic_softmax_scores'), f32 out [B,C,H,W] */
int nmsa_semantic_softmax(const void* logits, int logits_dtype,
                          int B, int C, int H, int W, float* probs,
                          nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * a1+a3+a4+a5  PanopticPostprocessing._postprocess_inference (core)
 *     model/postprocessing/panoptic.py:77-168 with
 *     utils/panoptic_merge.py:172-225 (deeplab_merge_semantic_and_instance)
 *
 * nmsa_panoptic_fused: one pass over the logits: per-pixel argmax (a1),
 * foreground = is_thing[class] (panoptic.py:123-127), offset grouping (a3) and
 * the per-instance class-vote histogram of the merge (panoptic_merge.py:201).
 *   is_thing   u8 [C]
 *   sem_u8     u8 [B,H,W]   class index 0..C-1 (required: paint reads it)
 *   inst       u8 [B,H,W]
 *   fg_out     u8 [B,H,W] or NULL ('panoptic_foreground_mask')
 *   score      f32 [B,H,W] or NULL
 *   votes      u32 [B,256,C+1]; votes[b,id,c] = #px of instance id whose (class+1) == c.
 *              Zeroed by this call unless votes_are_zero != 0 (the caller keeps a
 *              persistent table that nmsa_panoptic_assign(clear_votes=1) left clean)
 *   vote_rows_hint  kept for ABI stability, ignored: the per-workgroup vote counters are a
 *              fixed-size LDS hash table keyed by (instance id, class); 0 is fine
 * nmsa_panoptic_assign: per instance: class = mode (smallest on ties), running
 * per-class counter in ascending id order -> panoptic id (panoptic_merge.py:
 * 192-210).
 *   pan_of_inst i64 [B,256]  (void_label where the instance is dropped)
 *   area        i32 [B,256]  row sums of votes (meta 'area'; index 0 unused)
 *   ids_pan/ids_ins i64 [B,256], n_ids i32 [B]: the id dict in insertion order
 * nmsa_panoptic_paint: pan[p] = inst ? pan_of_inst[inst] :
 *                               (is_thing[sem] ? void : (sem+1)*max_inst)
 *   pan i64 [B,H,W]; pan_sem i64 [B,H,W] or NULL (= pan // max_inst, panoptic.py:160)
 * ------------------------------------------------------------------------- */
int nmsa_panoptic_fused(const void* logits, int logits_dtype, const float* offset,
                        const int32_t* centers_yx, const int32_t* n_centers,
                        const uint8_t* is_thing,
                        int B, int C, int H, int W, int max_centers,
                        float scale_y, float scale_x,
                        int use_dist_thr, float dist_thr,
                        uint8_t* sem_u8, uint8_t* inst, uint8_t* fg_out, float* score,
                        uint32_t* votes, int votes_are_zero, int vote_rows_hint,
                        nmsa_stream_t stream);

int nmsa_panoptic_assign(uint32_t* votes, int B, int n_vote_classes, int clear_votes,
                         int64_t max_instances_per_category, int64_t void_label,
                         int64_t* pan_of_inst, int32_t* area,
                         int64_t* ids_pan, int64_t* ids_ins, int32_t* n_ids,
                         nmsa_stream_t stream);

int nmsa_panoptic_paint(const uint8_t* sem_u8, const uint8_t* inst,
                        const int64_t* pan_of_inst, const uint8_t* is_thing,
                        int B, int C, int H, int W,
                        int64_t max_instances_per_category, int64_t void_label,
                        int64_t* pan, int64_t* pan_sem,
                        nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * a5  deeplab_merge_batch   utils/panoptic_merge.py:18-40,172-225
 * Generic entry (GT path / InstanceTaskHelper): arbitrary integer dtypes.
 *   sem        [B,H,W] sem_dtype, class values 0..n_classes-1 (0 = void)
 *   ins        [B,H,W] ins_dtype, instance ids 0..255
 *   thing_seg  u8 [B,H,W]
 *   is_thing_class u8 [n_classes]  (class value c is in thing_ids)
 *   votes      u32 [B,256,n_classes] scratch, zeroed by this call
 * Outputs as for assign + paint.
 * ------------------------------------------------------------------------- */
int nmsa_panoptic_merge(const void* sem, int sem_dtype, const void* ins, int ins_dtype,
                        const uint8_t* thing_seg, const uint8_t* is_thing_class,
                        int B, int n_classes, int H, int W,
                        int64_t max_instances_per_category, int64_t void_label,
                        uint32_t* votes, int64_t* pan_of_inst,
                        int64_t* pan, int64_t* ids_pan, int64_t* ids_ins, int32_t* n_ids,
                        nmsa_stream_t stream);

/* Same merge for instance ids beyond uint8 (ground-truth maps: uint16 ids stored as
 * int32, e.g. > 256 instances per image; task_helper/instance.py:61).  Ids 0..65535
 * are ranked per image first (ascending order preserved), at most max_segments
 * (<= 65536: every id such a map can hold; n_classes <= 65535) distinct thing ids per image.
 *   ids_pan / ids_ins  i64 [B, cap] with cap = max_segments rounded up to 1024
 *   status  i32 [1]: NMSA_ST_TABLE_OVERFLOW (more ids than max_segments),
 *                    32 = instance id outside [0, 65535]
 */
size_t nmsa_panoptic_merge_wide_workspace_bytes(int B, int n_classes, int max_segments);
int nmsa_panoptic_merge_wide(const void* sem, int sem_dtype, const void* ins, int ins_dtype,
                             const uint8_t* thing_seg, const uint8_t* is_thing_class,
                             int B, int n_classes, int H, int W,
                             int64_t max_instances_per_category, int64_t void_label,
                             int max_segments,
                             int64_t* pan, int64_t* ids_pan, int64_t* ids_ins, int32_t* n_ids,
                             int32_t* status, void* workspace, size_t workspace_bytes,
                             nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * f2  DensePostprocessingBase._crop_to_valid_region_and_resize_prediction
 *     model/postprocessing/dense_base.py:15-58   (the full-resolution step)
 * Every plane of `src` ([planes,Hs,Ws], planes = B or B*C) is cropped to the valid
 * region [y0:y0+h, x0:x0+w] and resized to [Ho,Wo]; dst is [planes,Ho,Wo].
 * The arithmetic is bit-for-bit the one of ATen's CPU kernels (see csrc/resize.hip):
 *   nearest : src = min(int(floorf(dst * float(in)/float(out))), in-1); i32 / i64 maps
 *             take the reference's float32 round trip (dense_base.py:38-40, :52)
 *   bilinear: align_corners=False, width first; dst has the dtype of src
 *   elem_type: NMSA_U8 (also bool) | NMSA_I16 | NMSA_I32 | NMSA_I64 | NMSA_ELEM_F32
 * ------------------------------------------------------------------------- */
int nmsa_resize_nearest(const void* src, int elem_type, int planes, int Hs, int Ws,
                        int y0, int x0, int h, int w, int Ho, int Wo, void* dst,
                        nmsa_stream_t stream);
int nmsa_resize_bilinear(const void* src, int dtype, int planes, int Hs, int Ws,
                         int y0, int x0, int h, int w, int Ho, int Wo, void* dst,
                         nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * f2  SemanticPostprocessing full-resolution argmax   model/postprocessing/semantic.py:61-80
 * crop + bilinear resize + argmax + max-softmax score of the logits in ONE pass; the
 * [B,C,Ho,Wo] full-resolution logits are not materialised (nmsa_resize_bilinear makes
 * them when `semantic_output_fullres` itself is read).  Same outputs / NULL rules as
 * nmsa_semantic_argmax; logits [B,C,Hs,Ws].
 * ------------------------------------------------------------------------- */
int nmsa_semantic_argmax_resized(const void* logits, int logits_dtype, int B, int C,
                                 int Hs, int Ws, int y0, int x0, int h, int w, int Ho, int Wo,
                                 uint8_t* idx_u8, int64_t* idx_i64, float* score,
                                 nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * f3  PanopticPostprocessing `compute_scores` branch   model/postprocessing/panoptic.py:171-239
 * Dense semantic / instance / panoptic score maps and the per-instance mean semantic score,
 * without the [B,C,H,W] softmax tensor and without the per-instance Python loop.
 *   logits      f32|bf16|f16 [B,C,H,W]
 *   sem_idx     u8  [B,H,W]  argmax class (nmsa_panoptic_fused / nmsa_semantic_argmax)
 *   sem_prob    f32 [B,H,W]  its softmax probability (the `score` output of the same calls)
 *   inst        u8  [B,H,W]; pan i64 [B,H,W] = class_value * max_instances_per_category + k
 *   pan_of_inst i64 [B,256]  panoptic id of every instance id (nmsa_panoptic_assign)
 *   inst_score_tab f32 [B,256]  instance score by instance id (meta 'score'; entry 0 unused)
 * outputs (f32 [B,H,W]):
 *   semantic score = softmax probability of the pixel's PANOPTIC class (0 on void),
 *   instance score = the instance's score on its painted pixels, else 0,
 *   panoptic score = mean semantic score of the instance x instance score on painted pixels,
 *                    else the semantic score;
 *   mean_semantic_score f32 [B,256] (meta 'semantic_score'; NaN for unused ids), may be NULL
 * ------------------------------------------------------------------------- */
size_t nmsa_panoptic_scores_workspace_bytes(int B);
int nmsa_panoptic_scores(const void* logits, int logits_dtype,
                         const uint8_t* sem_idx, const float* sem_prob,
                         const uint8_t* inst, const int64_t* pan,
                         const int64_t* pan_of_inst, const float* inst_score_tab,
                         int B, int C, int H, int W, int64_t max_instances_per_category,
                         float* out_semantic_score, float* out_instance_score,
                         float* out_panoptic_score, float* mean_semantic_score,
                         void* workspace, size_t workspace_bytes, nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * next-1  InstancePostprocessing._get_instance_orientation
 *     model/postprocessing/instance.py:271-319
 *   orientation f32 [B,2,H,W]; inst u8; mask u8 or NULL
 *   sums f64 [B,256,2] (sum of channel 0 / 1 per id), count i32 [B,256]; both
 *   zeroed by this call
 *   (angle = atan2(sum1, sum0) is taken on the host over <= 255 entries)
 * ------------------------------------------------------------------------- */
int nmsa_instance_orientation(const float* orientation, const uint8_t* inst,
                              const uint8_t* mask, int B, int H, int W,
                              double* sums, int32_t* count, nmsa_stream_t stream);
/* the same for ground-truth instance maps (ids 0..65535 in any integer dtype, at most
 * max_instances <= 4096 distinct masked ids per image; instance.py:432-438 passes
 * batch['instance']): ids i32 [B,cap] ascending, n_ids i32 [B], sums f64 [B,cap,2],
 * count i32 [B,cap] by position in `ids` (cap = max_instances rounded up to 1024);
 * status bits: 1 too many ids, 32 id out of range;
 * workspace: nmsa_targets_workspace_bytes(B, 1, max_instances) */
int nmsa_instance_orientation_wide(const float* orientation, const void* instance, int ins_dtype,
                                   const uint8_t* mask, int B, int H, int W, int max_instances,
                                   int32_t* ids, int32_t* n_ids, double* sums, int32_t* count,
                                   int32_t* status, void* workspace, size_t workspace_bytes,
                                   nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * f4  ground-truth target generation on the device (per batch instead of per sample in the
 *     dataloader workers).  Label maps in their on-wire dtypes (data/preprocessing/torch.py:60-66:
 *     semantic uint8, instance uint16 -> int32); instance ids in [0, 65535], at most
 *     `max_instances` (<= 4096) distinct ids per image.
 *  status bits (OR-ed into *status): 1 too many distinct ids (more non-zero ids in one image than
 *     `cap` = max_instances rounded up to a multiple of 1024: the tables are sized by cap, so the
 *     bit starts at cap + 1 ids, not at max_instances + 1), 32 id out of range (negative ids of
 *     the signed dtypes included), 64 semantic label outside [0, n_classes) on a pixel that carries
 *     an instance id, 128 id table overflow (an image has more (instance, class) segments than
 *     max_segments; n_ids is then max_segments and the lists hold the first max_segments).
 *  workspace: nmsa_targets_workspace_bytes(B, n_classes, max_instances), 8-byte aligned (16-byte
 *     aligned for the one-launch front end of the on-wire layout, see below).
 *     workspace_is_clean (nmsa_instance_targets / nmsa_panoptic_targets): 1 = this very workspace
 *     (same B, n_classes, max_instances) was last used by one of these two calls on the on-wire
 *     layout and nothing else wrote to it since — they leave their tables zeroed, so the call
 *     skips its memset; 0 = unknown contents (first use): the call zeroes what it needs.
 *  status: on the on-wire layout the word is SET by the call (no need to zero it); on any other
 *     layout the bits are OR-ed into it (zero it first).
 *  launches: the on-wire layout (semantic uint8, instance int32, 16-byte aligned rows of 4 pixels,
 *     W % 4 == 0, n_classes <= 16384) runs as [memset +] ONE scan launch (presence, statistics,
 *     rank, decide / naive ranks: k_tg_scan) + the paint launch; any other layout as memset + 5.
 *
 *  nmsa_instance_clear_stuff   InstanceClearStuffIDs._preprocess   data/preprocessing/instance.py:46-93
 *     instance[is_stuff_class[semantic]] = 0, in place (is_stuff_class includes void)
 *  nmsa_instance_targets       InstanceTargetGenerator._preprocess data/preprocessing/instance.py:157-286
 *     is_thing_class u8 [n_classes] or NULL (every instance encoded); is_stuff_class u8 [n_classes]
 *     or NULL (center mask = foreground); gauss_lut f32 [2*(3*sigma+1)^2 + 1]: heat-map value by
 *     integer squared distance to the center, float32(exp(-d2 / (2 sigma^2)));
 *     center f32 [B,H,W]; offset [B,2,H,W] (dy,dx): f32 divided by (H,W) when normalized_offset,
 *     else i16; foreground / center_mask u8 [B,H,W] (center_mask may be NULL);
 *     encoded_ids / skipped_ids i32 [B, cap] ascending (cap = max_instances rounded up to 1024),
 *     n_encoded / n_skipped i32 [B]   (the reference's dynamic parameters; any may be NULL)
 *  nmsa_panoptic_targets       PanopticTargetGenerator._preprocess data/preprocessing/panoptic.py:48-85
 *                              = naive_merge_semantic_and_instance_np utils/panoptic_merge.py:43-107
 *     panoptic i64 [B,H,W]; ids_pan / ids_ins i64 [B,max_segments] in the reference's dict order
 *     (instance ascending, then class ascending), n_ids i32 [B]
 *  nmsa_dve_targets            DenseVisualEmbeddingTargetGenerator  data/preprocessing/
 *                              dense_visual_embedding.py:22-93
 *     keys i64 [B,K] (first n_keys[b] valid), embeddings f32 [B,K,D], image_embedding f32 [B,D];
 *     lut f32 [B,K,D] = normalise(embedding - diff_factor * image_embedding) (NULL: indices only);
 *     indices i32 [B,H,W] = 1 + position of the pixel's panoptic id in keys (0 = none)
 *  nmsa_orientation_targets    OrientationTargetGenerator._preprocess data/preprocessing/orientation.py:37-97
 *     estimate_class u8 [n_classes] or NULL (no class test); keys i32 [B,K] (K <= 4096): per image
 *     the instance ids that have an orientation, strictly ascending, the first n_keys[b] valid;
 *     n_keys i32 [B]; biternion f32 [B,K,2] = (cos, sin) per key, 8-byte aligned.
 *     An id > 0 is painted over its whole mask iff it occurs in the map, is one of the image's keys
 *     and (estimate_class given) its majority class over the whole mask (void counts, a tie goes
 *     to the smaller class) is flagged.  orientation f32 [B,2,H,W] (channel 0 cos, 1 sin: the
 *     collated CHW form of the reference's HWC image), foreground u8 [B,H,W], present u8 [B,K]
 *     (1 for exactly the painted keys); everything else +0.0 / 0: every byte of the three outputs
 *     is written.  status bits 1, 32, 64; workspace and workspace_is_clean as for
 *     nmsa_instance_targets (the three calls may share one workspace in any order).
 *     launches: the scan of nmsa_instance_targets (or memset + 4 on any other layout) + one paint
 *     launch (k_ot_paint: ids looked up in the scan's id table; NMSA_OT_LOOKUP=search, read per call:
 *     binary search over the keys in LDS); no host synchronisation, no allocation.
 *
 *  nmsa_targets_route: which kernels the three generators run for these arguments, as a mask of
 *     NMSA_TG_ROUTE_* bits, or a negative NMSA_ERR_* for arguments the generators refuse.  The
 *     dispatchers switch on the same predicates and on nothing else; the pointers are only looked
 *     at for NULL and alignment, nothing is launched and no device is touched.
 *       SCAN          the one-launch front end (k_tg_scan) of all three generators; the status word
 *                     is then SET and the workspace left clean.  Without it: memset + the classic
 *                     launches (presence, rank, statistics, decide / naive ranks)
 *       FAST_LOADERS  the front end loads 4 labels per thread with one 16-byte and one 4-byte load
 *                     (semantic uint8 4-byte aligned, instance int32 16-byte aligned, H*W % 4 == 0);
 *                     always set with SCAN
 *       PAINT_TILED   nmsa_instance_targets paints 128 x 16 pixel tiles (FAST_LOADERS labels,
 *                     W % 4 == 0, center / offset 16-byte and foreground / center_mask 4-byte aligned)
 *       PAINT_VECTOR  ... 1024 consecutive pixels per workgroup with vector stores (the same without
 *                     W % 4 == 0: a group of 4 pixels may straddle a row end); neither bit: per element
 *       LUT_LDS       the paint keeps the heat-map table in LDS (2*(3*sigma+1)^2 + 1 <= 4096 entries:
 *                     sigma <= 14); without it the table is read from global memory
 *       SCAN_16       the scan keeps 16 table slots per thread instead of 4 (max_instances > 1024)
 *     sigma, center, offset, foreground, center_mask only matter to the paint bits (the outputs
 *     may be NULL: counted as aligned); workspace only to SCAN (16-byte aligned; NULL: aligned).
 * ------------------------------------------------------------------------- */
#define NMSA_TG_ROUTE_SCAN 1
#define NMSA_TG_ROUTE_FAST_LOADERS 2
#define NMSA_TG_ROUTE_PAINT_TILED 4
#define NMSA_TG_ROUTE_PAINT_VECTOR 8
#define NMSA_TG_ROUTE_LUT_LDS 16
#define NMSA_TG_ROUTE_SCAN_16 32
size_t nmsa_targets_workspace_bytes(int B, int n_classes, int max_instances);
int nmsa_targets_route(const void* semantic, int sem_dtype, const void* instance, int ins_dtype,
                       int n_classes, int H, int W, int sigma, int max_instances,
                       const float* center, const void* offset, const uint8_t* foreground,
                       const uint8_t* center_mask, const void* workspace);
int nmsa_instance_clear_stuff(const void* semantic, int sem_dtype, void* instance, int ins_dtype,
                              const uint8_t* is_stuff_class, int n_classes, int64_t n_px,
                              nmsa_stream_t stream);
int nmsa_instance_targets(const void* semantic, int sem_dtype, const void* instance, int ins_dtype,
                          const uint8_t* is_thing_class, const uint8_t* is_stuff_class,
                          int B, int n_classes, int H, int W,
                          int sigma, const float* gauss_lut, int normalized_offset, int max_instances,
                          float* center, void* offset, uint8_t* foreground, uint8_t* center_mask,
                          int32_t* encoded_ids, int32_t* n_encoded,
                          int32_t* skipped_ids, int32_t* n_skipped,
                          int32_t* status, void* workspace, size_t workspace_bytes, int workspace_is_clean,
                          nmsa_stream_t stream);
int nmsa_panoptic_targets(const void* semantic, int sem_dtype, const void* instance, int ins_dtype,
                          const uint8_t* is_thing_class, int B, int n_classes, int H, int W,
                          int64_t max_instances_per_category, int64_t void_label,
                          int max_instances, int max_segments,
                          int64_t* panoptic, int64_t* ids_pan, int64_t* ids_ins, int32_t* n_ids,
                          int32_t* status, void* workspace, size_t workspace_bytes, int workspace_is_clean,
                          nmsa_stream_t stream);
int nmsa_orientation_targets(const void* semantic, int sem_dtype, const void* instance, int ins_dtype,
                             const uint8_t* estimate_class, const int32_t* keys, const int32_t* n_keys,
                             const float* biternion, int B, int n_classes, int H, int W, int K,
                             int max_instances,
                             float* orientation, uint8_t* foreground, uint8_t* present,
                             int32_t* status, void* workspace, size_t workspace_bytes, int workspace_is_clean,
                             nmsa_stream_t stream);
int nmsa_dve_targets(const int64_t* panoptic, const int64_t* keys, const int32_t* n_keys,
                     const float* embeddings, const float* image_embedding, float diff_factor,
                     int B, int K, int D, int H, int W,
                     float* lut, int32_t* indices, nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * a11  MeanIntersectionOverUnion.update   metric/miou.py:44-56
 *   confmat[t, p] += 1 for every element (bincount(t*n + p, minlength=n*n)).
 *   preds / target: any integer dtype, n_px elements each.
 *   pred_div : preds are used as raw // pred_div (1 = as is; 65536 gives the
 *              `pan // max_instances_per_category` of task_helper/panoptic.py:123)
 *   mode 0   : every element counts
 *   mode 1   : elements with target == 0 are skipped and target-1 is used
 *              (the void masking of task_helper/semantic.py:124-128)
 *   confmat  : i64 [n_classes, n_classes], accumulated into (not zeroed)
 *   status   : i32 [1] device word, OR-ed with NMSA_ST_* bits (value out of range
 *              = what makes the reference's bincount/reshape raise)
 * ------------------------------------------------------------------------- */
#define NMSA_ST_TABLE_OVERFLOW 1
#define NMSA_ST_CATEGORY_RANGE 2
#define NMSA_ST_MISSING_KEY 4
#define NMSA_ST_VALUE_RANGE 8
#define NMSA_ST_SENTINEL_KEY 16
size_t nmsa_confmat_workspace_bytes(int n_classes);
int nmsa_confmat_update(const void* preds, int pred_dtype, int64_t pred_div,
                        const void* target, int target_dtype,
                        int64_t n_px, int n_classes, int mode,
                        int64_t* confmat, int32_t* status,
                        void* workspace, size_t workspace_bytes, nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * a12/a13  compare_and_accumulate + PanopticQuality.update
 *     metric/pq.py:60-179, :262-296
 *   pred, target : i64 [B,H,W] panoptic maps (category*max_inst + instance)
 *   iou/tp/fn/fp : f64 [num_categories] states, accumulated into (image order;
 *                  the IoU sums are bit-identical to the reference's fp64 sums)
 *   matches      : i64 [B,match_capacity,2] (gt id, pred id) of the TP pairs in
 *                  ascending intersection-id order, or NULL; n_matches i32 [B]
 *   status       : i32 [1] device word, OR-ed with NMSA_ST_* bits
 *   limits       : <= 2048 distinct ids per image and side, num_categories <= 1024;
 *                  distinct (target, pred) intersections per image <= cap / 2 with
 *                  cap = H*W / 24 rounded up to a power of two in [4096, 131072]
 *                  (640x480: 8192 intersections, 1024x768: 16384); beyond that
 *                  NMSA_ST_TABLE_OVERFLOW is raised
 *   workspace_is_clean : non-zero when `workspace` was last used by a completed
 *                  nmsa_pq_update of the same B, H, W (which leaves the tables empty); the
 *                  per-call table initialisation is then skipped
 * ------------------------------------------------------------------------- */
size_t nmsa_pq_workspace_bytes(int B, int H, int W, int num_categories);
int nmsa_pq_update(const int64_t* pred, const int64_t* target, int B, int H, int W,
                   int num_categories, int64_t ignored_label,
                   int64_t max_instances_per_category, int64_t offset,
                   int64_t void_segment_id,
                   double* iou_per_class, double* tp_per_class,
                   double* fn_per_class, double* fp_per_class,
                   int64_t* matches, int match_capacity, int32_t* n_matches,
                   int32_t* status, void* workspace, size_t workspace_bytes,
                   int workspace_is_clean, nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * Host hand-over of the per-image tables of one pipeline run (the Python objects of
 *     panoptic.py:118-167 — id dicts, instance meta — are built on the host): packs
 *     [n_centers, n_ids, centers_yx[kc][2], scores[kc], area[min(kc+1,256)],
 *      ids_pan[min(kc,256)], ids_ins[min(kc,256)]], kc = min(columns, max_centers), into one
 *     f64 row per image (exact: ids < 2^53, f32 scores) -> ONE device->host copy per batch.
 *     n_ids / ids_pan / ids_ins may be NULL together (instance-only postprocessing): the row
 *     then ends after the areas and its second entry is 0.
 *     `out` may also be pinned host memory (hipHostMalloc: mapped into the device's address space
 *     at the same address): the kernel then stores the rows where the host reads them — valid
 *     once an event recorded behind the call has completed — and no copy is needed at all.
 * ------------------------------------------------------------------------- */
int nmsa_pack_tables(const int32_t* n_centers, const int32_t* n_ids,
                     const int32_t* centers_yx, const float* scores,
                     const int32_t* area, const int64_t* ids_pan, const int64_t* ids_ins,
                     int B, int max_centers, int columns, double* out, nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * a11 + a12 in ONE pass over the prediction (PanopticTaskHelper.validation_step,
 *     task_helper/panoptic.py:104-126, updates both metrics from the same panoptic map):
 *     PQ exactly as nmsa_pq_update, plus confmat[target_semantic, pred // pred_div] += 1
 *     exactly as nmsa_confmat_update(mode 0) — the i64 prediction map is read once.
 *   target_semantic u8 [B,H,W]; confmat i64 [n,n] with n = confmat_classes <= 64;
 *   confmat_status: the status word of the mIoU metric (label outside [0, n) -> bit 8);
 *   confmat_workspace: nmsa_pq_confmat_workspace_bytes(B,H,W,n) bytes (0 = not supported).
 * ------------------------------------------------------------------------- */
size_t nmsa_pq_confmat_workspace_bytes(int B, int H, int W, int n_classes);
int nmsa_pq_update_with_confmat(
    const int64_t* pred, const int64_t* target, const uint8_t* target_semantic,
    int B, int H, int W,
    int num_categories, int64_t ignored_label, int64_t max_instances_per_category, int64_t offset,
    int64_t void_segment_id,
    double* iou_per_class, double* tp_per_class, double* fn_per_class, double* fp_per_class,
    int64_t* matches, int match_capacity, int32_t* n_matches,
    int32_t* status, void* workspace, size_t workspace_bytes, int workspace_is_clean,
    int confmat_classes, int64_t pred_div, int64_t* confmat, int32_t* confmat_status,
    void* confmat_workspace, size_t confmat_workspace_bytes, nmsa_stream_t stream);
/* The same update with the prediction given as the PARTS nmsa_panoptic_paint paints the map from
 * (the fused pipeline's outputs) instead of the painted int64 map: the predicted panoptic id of
 * a pixel is pan_of_inst[b][pred_instance] where pred_instance != 0, else (pred_semantic + 1) *
 * max_instances_per_category when that class is stuff, else void_label — 2 B/px read instead of
 * 8 B/px; results are bit-identical to nmsa_pq_update_with_confmat on the painted map
 * (task_helper/panoptic.py:104-126 at network resolution; no match list).
 *   pred_semantic u8 [B,H,W] class index 0..n_sem_classes-1 (<= 255), pred_instance u8 [B,H,W],
 *   pan_of_inst i64 [B,256], is_thing_class u8 [n_sem_classes].
 *   confmat_classes = 0 with target_semantic = confmat = confmat_status = NULL: the PQ update
 *   alone (nmsa_pq_update on the painted map, read as its parts) — for class counts beyond the
 *   fused matrix (64) */
int nmsa_pq_update_with_confmat_parts(
    const uint8_t* pred_semantic, const uint8_t* pred_instance, const int64_t* pan_of_inst,
    const uint8_t* is_thing_class, int n_sem_classes, int64_t void_label,
    const int64_t* target, const uint8_t* target_semantic,
    int B, int H, int W,
    int num_categories, int64_t ignored_label, int64_t max_instances_per_category, int64_t offset,
    int64_t void_segment_id,
    double* iou_per_class, double* tp_per_class, double* fn_per_class, double* fp_per_class,
    int32_t* status, void* workspace, size_t workspace_bytes, int workspace_is_clean,
    int confmat_classes, int64_t pred_div, int64_t* confmat, int32_t* confmat_status,
    void* confmat_workspace, size_t confmat_workspace_bytes, nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * a6-a10  per-pixel multi-task losses (forward + backward)
 * Common conventions: predictions f32|bf16|f16 (code in `dtype`), targets f32,
 * labels / masks u8, planar NCHW.  Forward returns device scalars
 * loss_sum (f64) and the element count (i64) — the task helpers divide
 * (task_helper/base.py:161-182); nothing is copied to the host.  Backward
 * recomputes from the inputs and multiplies by the upstream gradient read from
 * the device scalar *grad_scale; gradients are written in the prediction dtype.
 * workspace: nmsa_loss_workspace_bytes(B,H,W) bytes (block partials; the final
 * sum is taken in a fixed order -> run-to-run deterministic).
 *
 * nmsa_loss_ce_*       CrossEntropyLossSemantic._compute_loss  loss/ce.py:40-68
 *     target u8 [B,H,W], 0 = void (ignored); weights f32 [C] or NULL;
 *     weight_sum (f64, may be NULL) = sum over non-void px of w[label]: the divisor
 *     of the ESANet `weighted_reduction` (ce.py:57-68);
 *     lse2 f32 [2,B,H,W] (optional, NULL = off): the forward pass stores max_c x_c (plane 0) and
 *     log2(sum_c exp(x_c - max)) (plane 1) per pixel and the backward pass, given the same buffer,
 *     reads the logits ONCE instead of twice (what autograd's saved log_softmax buys the
 *     reference); two planes, since one float max * log2(e) + log2(sum) rounds to an ulp of |max|
 * nmsa_loss_masked_*   MSELoss / L1Loss (reduction='sum') loss/mse.py:21-41, l1.py:21-41
 *     with the masking of task_helper/instance.py:129-139,154-167:
 *     sum_px mean_c f(pred*mask - target), n = sum(mask); mask u8 [B,H,W] or NULL;
 *     kind 0 = MSE, 1 = L1; C = 1 for [B,H,W] inputs
 *     kind 2 = center focal loss — EXTENSION, not in the reference: CenterNet's penalty-reduced
 *     focal loss (alpha 2, beta 4, pred clamped to [1e-4, 1-1e-4]) over the masked pixels;
 *     n_mask then counts the positive (target == 1) masked pixels
 * nmsa_loss_vonmises_* VonMisesLossBiternion  loss/vonmises.py:27-51 over the px
 *     where mask != 0 (gather of task_helper/instance.py:186-216), pred/target [B,2,H,W]
 * nmsa_loss_*_fwd_grad / nmsa_loss_*_bwd_unless  forward and gradient in ONE pass:
 *     the reference's losses are sums that the caller divides (`loss / n`,
 *     task_helper/base.py:161-182: sum_scales loss / sum_scales n), so the upstream gradient
 *     of a loss sum is known before backward runs once n is (nmsa_count_u8 over the labels /
 *     mask, 1 B/px).  *_fwd_grad takes that EXPECTED scale as a device scalar and writes
 *     expected * d loss_sum / d pred into grad_* while it computes the forward sum: the
 *     prediction is read once and the gradient written once (CE at C = 40, bf16: 162 B/px
 *     instead of 250).  Backward then calls *_bwd_unless with the real upstream gradient:
 *     when *grad_scale is bit-equal to *computed_for the gradient buffer is already right and
 *     the kernel returns at once (counters[0]++), otherwise it recomputes the gradient from
 *     the inputs (counters[1]++), so the result never depends on the expectation.
 *     The CE variant keeps a pixel's whole class column in registers up to C = 48; for 49..256
 *     classes the four waves of a workgroup share the column (wave w holds a quarter of the
 *     classes of the same pixels; maximum and sum of exponentials are exchanged through LDS):
 *     logits read once, gradient written once.  A recomputing backward launch (*_bwd_unless on
 *     a wrong expectation) is the same single pass: it never costs more than nmsa_loss_ce_bwd.
 *     Beyond 256 classes the launch walks the column twice through the caches.
 *     nmsa_loss_ce_fwd_grad_supported(dtype, C): 1 for every valid dtype and C <= 4096.
 * nmsa_count_u8        *count = #{i : lo <= values[i] <= hi}  (labels 1..C, mask bytes 1..255);
 *     *mean_scale (optional) = weight / (float)count, the correctly rounded fp32 division
 *     autograd performs for `weight * loss_sum / count`;
 *     workspace: nmsa_count_workspace_bytes()
 * nmsa_loss_cos_emb_*  CosineEmbeddingLoss  loss/cos_emb.py:21-56 with the LUT gather of
 *     task_helper/dense_visual_embedding.py:110-171: pred [B,D,H,W], indices i32
 *     [B,H,W] (0 = no target), lut f32 [B,L,D];
 *     dots f32 [B,2,H,W] (optional, NULL = off; needs H*W % 8 == 0 and 16-B aligned
 *     pointers, NMSA_ERR_ARG otherwise — see nmsa_loss_cos_emb_can_keep_dots): the forward
 *     pass stores x.y and |x|^2 per pixel and the backward pass, given the same buffer, reads
 *     the prediction ONCE (for the gradient) instead of twice
 * ------------------------------------------------------------------------- */
size_t nmsa_loss_workspace_bytes(int B, int H, int W);
/* NaN / +-inf logits: the classes of F.cross_entropy(ignore_index=-1), a void pixel's column included */
int nmsa_loss_ce_fwd(const void* logits, int dtype, const uint8_t* target, const float* weights,
                     int B, int C, int H, int W, float label_smoothing,
                     double* loss_sum, int64_t* n_elements, double* weight_sum, float* lse2_out,
                     int32_t* status, void* workspace, size_t workspace_bytes, nmsa_stream_t stream);
int nmsa_loss_ce_bwd(const void* logits, int dtype, const uint8_t* target, const float* weights,
                     int B, int C, int H, int W, float label_smoothing,
                     const float* grad_scale, const float* lse2, void* grad_logits,
                     nmsa_stream_t stream);
/* the same two kernels for more than 255 classes (reference ce.py:40-68 takes any number): labels
 * as int16 (0 = void, 1..C), C <= 4096 */
int nmsa_loss_ce_fwd_i16(const void* logits, int dtype, const int16_t* target,
                         const float* weights, int B, int C, int H, int W,
                         float label_smoothing,
                         double* loss_sum, int64_t* n_elements, double* weight_sum,
                         float* lse2_out,
                         int32_t* status, void* workspace, size_t workspace_bytes,
                         nmsa_stream_t stream);
int nmsa_loss_ce_bwd_i16(const void* logits, int dtype, const int16_t* target,
                         const float* weights, int B, int C, int H, int W,
                         float label_smoothing, const float* grad_scale, const float* lse2,
                         void* grad_logits, nmsa_stream_t stream);
int nmsa_loss_ce_fwd_grad_supported(int dtype, int C);
/* pinned as nmsa_loss_ce_fwd / _bwd: loss and gradient classes of F.cross_entropy; exponents are (x - max) * log2(e), finite logits up to 1e30 are pinned */
int nmsa_loss_ce_fwd_grad(const void* logits, int dtype, const uint8_t* target, const float* weights,
                          int B, int C, int H, int W, float label_smoothing,
                          const float* expected_grad_scale,
                          double* loss_sum, int64_t* n_elements, double* weight_sum,
                          void* grad_logits, int32_t* status,
                          void* workspace, size_t workspace_bytes, nmsa_stream_t stream);
int nmsa_loss_ce_bwd_unless(const void* logits, int dtype, const uint8_t* target,
                            const float* weights, int B, int C, int H, int W,
                            float label_smoothing, const float* grad_scale, void* grad_logits,
                            const float* computed_for, int32_t* counters, nmsa_stream_t stream);
size_t nmsa_count_workspace_bytes(void);
int nmsa_count_u8(const uint8_t* values, int64_t n, int lo, int hi, int64_t* count,
                  float* mean_scale, float weight,
                  void* workspace, size_t workspace_bytes, nmsa_stream_t stream);
/* a masked-out pixel is never read: a NaN / infinity there leaves sum, count and gradient clean (the reference multiplies: NaN); kind 2 (focal) clamps by
 * comparisons, so a NaN prediction gives a NaN sum and a zero gradient at its element, +-inf are clamped */
int nmsa_loss_masked_fwd(const void* pred, int dtype, const float* target, const uint8_t* mask,
                         int B, int C, int H, int W, int kind,
                         double* loss_sum, int64_t* n_mask,
                         void* workspace, size_t workspace_bytes, nmsa_stream_t stream);
int nmsa_loss_masked_bwd(const void* pred, int dtype, const float* target, const uint8_t* mask,
                         int B, int C, int H, int W, int kind,
                         const float* grad_scale, void* grad_pred, nmsa_stream_t stream);
int nmsa_loss_masked_fwd_grad(const void* pred, int dtype, const float* target,
                              const uint8_t* mask, int B, int C, int H, int W, int kind,
                              const float* expected_grad_scale,
                              double* loss_sum, int64_t* n_mask, void* grad_pred,
                              void* workspace, size_t workspace_bytes, nmsa_stream_t stream);
int nmsa_loss_masked_bwd_unless(const void* pred, int dtype, const float* target,
                                const uint8_t* mask, int B, int C, int H, int W, int kind,
                                const float* grad_scale, void* grad_pred,
                                const float* computed_for, int32_t* counters, nmsa_stream_t stream);
/* a masked-out pixel is never read; NaN / +-inf at a masked one answer as 1 - exp(kappa (x.y - 1)) does */
int nmsa_loss_vonmises_fwd(const void* pred, int dtype, const float* target, const uint8_t* mask,
                           int B, int H, int W, float kappa,
                           double* loss_sum, int64_t* n_rows,
                           void* workspace, size_t workspace_bytes, nmsa_stream_t stream);
int nmsa_loss_vonmises_bwd(const void* pred, int dtype, const float* target, const uint8_t* mask,
                           int B, int H, int W, float kappa,
                           const float* grad_scale, void* grad_pred, nmsa_stream_t stream);
int nmsa_loss_vonmises_fwd_grad(const void* pred, int dtype, const float* target,
                                const uint8_t* mask, int B, int H, int W, float kappa,
                                const float* expected_grad_scale,
                                double* loss_sum, int64_t* n_rows, void* grad_pred,
                                void* workspace, size_t workspace_bytes, nmsa_stream_t stream);
int nmsa_loss_vonmises_bwd_unless(const void* pred, int dtype, const float* target,
                                  const uint8_t* mask, int B, int H, int W, float kappa,
                                  const float* grad_scale, void* grad_pred,
                                  const float* computed_for, int32_t* counters,
                                  nmsa_stream_t stream);
/* a pixel with index 0 is never read: a NaN / infinity there leaves sum, count and gradient clean, its gradient column exactly 0 */
int nmsa_loss_cos_emb_fwd(const void* pred, int dtype, const int32_t* indices, const float* lut,
                          int B, int D, int H, int W, int L,
                          double* loss_sum, int64_t* n_rows, float* dots_out, int32_t* status,
                          void* workspace, size_t workspace_bytes, nmsa_stream_t stream);
int nmsa_loss_cos_emb_bwd(const void* pred, int dtype, const int32_t* indices, const float* lut,
                          int B, int D, int H, int W, int L,
                          const float* grad_scale, const float* dots, void* grad_pred,
                          nmsa_stream_t stream);
/* forward + gradient in ONE pass over the prediction: the D-column of a pixel stays in the
 * registers of ceil(D / 64) waves between the reduction and the gradient.  H*W a multiple of 4
 * (2 for f32), 8-byte aligned planes, and either D % 64 == 0, D <= 512 with the image's fp32 LUT +
 * the exchange buffers within the CU's LDS (k_cos_split: one workgroup per column) or D <= 1024,
 * any D (k_cos_parts: the column over ceil(D / 256) cooperating workgroups that exchange their
 * partial sums as 8-byte {value, tag} granules through the workspace; DVEFormer's D = 768; a
 * ragged last wave when D % 64 != 0).  The gradient
 * is written for *expected_gscale; nmsa_loss_cos_emb_bwd_unless confirms it (bit-equal
 * *grad_scale) or recomputes — it takes the forward call's workspace (NULL is fine for
 * D <= 512).  Status bit 32: a cooperating workgroup did not answer within ~2 s (sum and
 * gradient are NaN then). */
int nmsa_loss_cos_emb_fwd_grad_supported(int dtype, int D, int H, int W, int L);
size_t nmsa_loss_cos_emb_fwd_grad_workspace_bytes(int B, int D, int H, int W, int L);
int nmsa_loss_cos_emb_fwd_grad(const void* pred, int dtype, const int32_t* indices, const float* lut,
                               int B, int D, int H, int W, int L, const float* expected_gscale,
                               double* loss_sum, int64_t* n_rows, void* grad_pred, int32_t* status,
                               void* workspace, size_t workspace_bytes, nmsa_stream_t stream);
int nmsa_loss_cos_emb_bwd_unless(const void* pred, int dtype, const int32_t* indices, const float* lut,
                                 int B, int D, int H, int W, int L, const float* grad_scale,
                                 void* grad_pred, const float* computed_for, int32_t* counters,
                                 void* workspace, size_t workspace_bytes, nmsa_stream_t stream);
/* 1 when the (L, D, H*W) combination runs the LDS-LUT kernel that can keep `dots` */
int nmsa_loss_cos_emb_can_keep_dots(int D, int H, int W, int L);

/* ---------------------------------------------------------------------------
 * a7 / a9  the forms of the same loss classes that no task helper calls (csrc/losses_forms.hip)
 * nmsa_loss_elementwise_none_*  MSELoss / L1Loss with reduction='none' (loss/mse.py:21-41 else
 *     branch, loss/l1.py:21-41): out[i] = (pred[i] - target[i])^2 or |pred[i] - target[i]| over n
 *     contiguous elements, op-math in fp32, rounded once to out_dtype (NMSA_F32 or `dtype` — the
 *     type promotion of pred and target); kind 0 = MSE, 1 = L1.  _bwd: grad_pred[i] =
 *     upstream[i] * d out[i] / d pred[i], upstream in upstream_dtype (NMSA_F32 or `dtype`).
 *     The reference's 2-D [N, C] rows with 'sum' / 'mean' need no entry point of their own:
 *     sum_n mean_c f = (1 / C) * nmsa_loss_masked_fwd over the n * C elements as one plane.
 * nmsa_loss_cos_rows_*  CosineEmbeddingLoss on rows with labels (loss/cos_emb.py:21-56 with
 *     `target_similarity`; torch.nn.CosineEmbeddingLoss, margin 0): input [n_rows, D] in `dtype`,
 *     target f32 [n_rows, D], labels f32 [n_rows] (+1 similar: 1 - cos; -1 dissimilar:
 *     max(0, cos - margin); anything else: 0) or NULL (all +1); loss_rows f32 [n_rows] — the
 *     'none' reduction; 'sum' / 'mean' are the sum of that vector.  _bwd: grad_input =
 *     upstream[row] * d loss_rows[row] / d input (upstream f32 [n_rows], or ONE f32 scalar when
 *     upstream_is_scalar != 0). */
int nmsa_loss_elementwise_none_fwd(const void* pred, int dtype, const float* target, int64_t n,
                                   int kind, int out_dtype, void* out, nmsa_stream_t stream);
int nmsa_loss_elementwise_none_bwd(const void* pred, int dtype, const float* target, int64_t n,
                                   int kind, int upstream_dtype, const void* upstream,
                                   void* grad_pred, nmsa_stream_t stream);
/* a NaN cosine stays NaN under label -1 too (clamp_min as ATen's, no fmaxf); a poisoned row touches its own loss and gradient row only */
int nmsa_loss_cos_rows_fwd(const void* input, int dtype, const float* target, const float* labels,
                           int64_t n_rows, int D, float margin, float* loss_rows,
                           nmsa_stream_t stream);
int nmsa_loss_cos_rows_bwd(const void* input, int dtype, const float* target, const float* labels,
                           int64_t n_rows, int D, float margin, const float* upstream,
                           int upstream_is_scalar, void* grad_input, nmsa_stream_t stream);
/* VonMisesLossBiternion with reduction='none' (loss/vonmises.py:27-51): input [n_rows, 2] in
 * `dtype`, target f32 [n_rows, 2] -> loss_rows f32 [n_rows] = 1 - exp(kappa (x.y - 1));
 * _bwd: grad_input = upstream[row] * d loss_rows[row] / d input, upstream f32 [n_rows] */
int nmsa_loss_vonmises_rows_fwd(const void* input, int dtype, const float* target, int64_t n_rows,
                                float kappa, float* loss_rows, nmsa_stream_t stream);
int nmsa_loss_vonmises_rows_bwd(const void* input, int dtype, const float* target, int64_t n_rows,
                                float kappa, const float* upstream, void* grad_input,
                                nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * a10  the losses of a task helper in one call
 *      InstanceTaskHelper._compute_losses  task_helper/instance.py:92-269
 *      SemanticTaskHelper._compute_losses  task_helper/semantic.py:57-90
 *      TaskHelperBase.accumulate_losses    task_helper/base.py:161-182
 * Every (loss, supervision scale) pair is an ITEM; the items whose sums the caller adds and
 * divides by their summed element counts (accumulate_losses) form a TOTAL.  One call
 *   counts the labels / mask bytes of all items (launch 1, 1 B/px); the launch's last workgroup
 *     forms per total the divisor n and the EXPECTED upstream gradient w / n of its loss sums
 *     (w lives in the total's spec record and is learned from the backward passes: loss
 *     weights, AMP scale, ... need no hint from the caller)
 *   computes all forward sums and writes all gradients for that expectation (launch 2: block
 *     ranges per item; cross entropies above 48 classes run k_ce_split as launches of their own)
 *   reduces the block partials per item in a fixed order and forms per item loss_sum / count
 *     and per total sum(loss sums) / divisor (launch 3; the reductions of accumulate_losses, in
 *     item order, float32)
 * A call without any gradient buffer (validation) skips the count and takes the divisors from
 * the finalized counts (2 launches).
 * nmsa_multitask_loss_bwd_unless is ONE launch (+ one per wide cross entropy / cosine item): a
 * small grid that walks the block list; every workgroup turns the upstream gradients of the
 * three outputs into one upstream scale per item and compares it with the expectation,
 * workgroup 0 also updates w; only the items that differ are recomputed and the grid is gone at
 * once when every gradient stands.  A NaN expectation ("the forward
 * pass wrote no gradient") is never confirmed — not even by an upstream gradient that is the same
 * NaN: gradient-only launches always write, so a NaN upstream comes out as NaN gradients.
 * `spec` (and `counters`) may be NULL there: a recompute nobody predicted (a second backward
 * through a retained graph) leaves the caller's record and the tally alone.
 * `workspace`: the forward call's buffer, contents dead by then (used as the granule exchange of
 * cosine items with D > 512; may be NULL without such items).
 *   items        HOST array; pointers inside are device pointers.  kind NMSA_LOSS_*; CE: pred =
 *                logits [B,C,H,W], mask = labels u8 [B,H,W] (0 = void), weights f32 [C] or NULL,
 *                param = label smoothing; MSE / L1 / FOCAL: pred [B,C,H,W] (C = 1 for [B,H,W]),
 *                target f32, mask u8 [B,H,W] or NULL; VONMISES: pred / target [B,2,H,W], mask,
 *                param = kappa; COS_EMB (loss/cos_emb.py:21-56 with the LUT gather of
 *                task_helper/dense_visual_embedding.py:110-171): pred [B,D,H,W] with C = D, target =
 *                LUT f32 [B,L,D] with L in `reserved`, mask = indices i32 [B,H,W] (0 = no target) —
 *                shapes nmsa_loss_cos_emb_fwd_grad_supported accepts, else NMSA_ERR_UNSUPPORTED.
 *                grad = gradient buffer shaped like pred, or NULL (forward only).
 *                clamp_count: the item's count enters its loss and its total as max(count, 1)
 *                (task_helper/instance.py:206-211)
 *   spec         i32 [n_totals + 1][8] device, persistent, owned by the caller (zero it, then store
 *                the fp32 bits of the initial upstream weight, usually 1.0f, at [t][2], t < n_totals):
 *                [0] backward passes that found their gradient written [1] ... that recomputed;
 *                the LAST row is scratch of the calls (the tickets their launches draw to find
 *                their last workgroup): zero it once, every call leaves it zero again.  One
 *                record set serves one stream at a time.
 *   expect       f32 [n_totals][2] device, out: expected upstream gradient (NaN: none) and the
 *                divisor as float; must be handed to nmsa_multitask_loss_bwd_unless unchanged
 *   loss_sums    f64 [n_items], counts i64 [n_items], aux f64 [n_items] or NULL (CE: sum of the
 *                label weights, ce.py:57-68) — device
 *   out_f32      f32 [2 n_items + n_totals] device or NULL: the loss sums as float32, then
 *                item_loss[i] = float32(sum_i) / float32(count_i), then total_loss[t] =
 *                (sum of the float32 sums of its items, in item order) / divisor_t
 *   grad_sums / grad_item_losses / grad_total_losses   f32 [n_items] / [n_items] / [n_totals]
 *                device or NULL: upstream gradients of the three parts of out_f32; item i's
 *                upstream scale is grad_sums[i] + grad_item_losses[i] / count_i +
 *                grad_total_losses[total_i] / divisor_t
 *   grad_scales  f32 [n_items] device, scratch: receives those upstream scales
 *   counters     i32 [2] device or NULL: per total and backward pass, [0] += 1 when the expectation
 *                held, [1] += 1 when it did not (a tally over all callers; the spec records keep
 *                their own)
 * ------------------------------------------------------------------------- */
enum { NMSA_LOSS_CE = 0, NMSA_LOSS_MSE = 1, NMSA_LOSS_L1 = 2, NMSA_LOSS_FOCAL = 3, NMSA_LOSS_VONMISES = 4,
       NMSA_LOSS_COS_EMB = 5 };
#define NMSA_MULTI_MAX_ITEMS 16
#define NMSA_MULTI_MAX_TOTALS 8
typedef struct nmsa_loss_item {
    int32_t kind, dtype, B, C, H, W;
    int32_t total;        /* index of the total this item belongs to */
    int32_t clamp_count;  /* 1: max(count, 1) is the item's divisor and enters the total; 2: the item's divisor only */
    float param;          /* label smoothing | kappa */
    int32_t reserved;     /* COS_EMB: L, the LUT rows per image; otherwise 0 */
    const void* pred;
    const void* target;
    const void* mask;     /* labels (CE) or mask bytes; NULL = every pixel */
    const float* weights;
    void* grad;
} nmsa_loss_item;
size_t nmsa_multitask_loss_workspace_bytes(const nmsa_loss_item* items_host, int n_items);
/* a NaN / infinity in an item of one total leaves every sum, loss and gradient of the other totals bit-equal, and no NaN in the spec records */
int nmsa_multitask_loss_fwd_grad(const nmsa_loss_item* items_host, int n_items, int n_totals,
                                 int32_t* spec, float* expect, double* loss_sums, int64_t* counts,
                                 double* aux, float* out_f32, int32_t* status, void* workspace,
                                 size_t workspace_bytes, nmsa_stream_t stream);
int nmsa_multitask_loss_bwd_unless(const nmsa_loss_item* items_host, int n_items, int n_totals,
                                   const float* grad_sums, const float* grad_item_losses,
                                   const float* grad_total_losses, const int64_t* counts,
                                   const float* expect, int32_t* spec, float* grad_scales,
                                   int32_t* counters, void* workspace, size_t workspace_bytes,
                                   nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * DenseVisualEmbeddingPostprocessing._postprocess_inference, normalisation + projection
 *     model/postprocessing/dense_visual_embedding.py:126 (output /= output.norm(dim=1)) and :81
 *     (F.conv2d with the C x D x 1 x 1 class embeddings), both heads from one pass over `emb`.
 *   emb        f32 [B,D,H,W]  normalised IN PLACE: x * (1 / sqrt(sum_d x^2)) per pixel
 *   weight_a/b f32 [Ca,D] / [Cb,D] or NULL (head off; its C and logits are then ignored)
 *   logits_a/b f32 [B,Ca,H,W] / [B,Cb,H,W]: dot(x, w_c) * (1 / sqrt(sum_d x^2))
 * A zero vector gives NaN in its D channels and in every logit; inf / NaN propagate.  f32 products
 * and accumulation throughout.  D % 4 == 0 (<= 1024), H*W % 4 == 0, C <= 256 per head and 16-byte
 * aligned pointers take the MFMA kernel; every other shape (any D, C >= 1) a plain per-pixel
 * kernel, which NMSA_DVE_ROUTE_GENERIC also selects for shapes the MFMA kernel accepts (tests).
 * Without the 1 / sqrt the reference's x / sqrt(sum) stays finite a little longer: a pixel whose sum
 * of squares leaves the normal float32 range (every |x| below ~1e-19, or one above ~1.8e19) gets
 * inf or 0 as its factor here.  Supported magnitudes are those whose sum of squares is a normal
 * float32.  NMSA_ERR_ARG: NULL / non-positive arguments, H*W above 2^31 - 1, more than 2^31 - 1
 * workgroups.  No workspace.
 *
 * nmsa_dve_project_route: which kernel nmsa_dve_project runs for the same arguments (the launch
 * switches on this function's answer and on nothing else; the pointers are only looked at for
 * NULL and alignment, nothing is launched).  NMSA_DVE_KERNEL_GENERIC (0) for the per-pixel kernel,
 * PT * 16 + NT for the MFMA instantiation with 16 PT pixels per wave and NT tiles of 16 classes
 * per pass (131 = <8,3>, 67 = <4,3>, 70 = <4,6>), or the negative NMSA_ERR_* nmsa_dve_project
 * would return.  Up to three class tiles over both heads: <8,3> when B * ceil(H*W / 128) is at
 * least 8 waves per compute unit (nmsa_device_geometry), else <4,3>; more tiles: <4,6>.
 * ------------------------------------------------------------------------- */
#define NMSA_DVE_ROUTE_AUTO 0
#define NMSA_DVE_ROUTE_GENERIC 1
#define NMSA_DVE_KERNEL_GENERIC 0
int nmsa_dve_project_route(const float* emb, int B, int D, int H, int W,
                           const float* weight_a, int Ca, const float* logits_a,
                           const float* weight_b, int Cb, const float* logits_b, int route);
int nmsa_dve_project(float* emb, int B, int D, int H, int W,
                     const float* weight_a, int Ca, float* logits_a,
                     const float* weight_b, int Cb, float* logits_b,
                     int route, nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * the surface-normal task (csrc/normal.hip)
 *
 * nmsa_normal_valid_mask: _get_valid_gt_normals, task_helper/normal.py:165-167
 *   target f32 [B,3,H,W] -> mask u8 [B,H,W]: 0 iff all three channels compare equal to zero BY
 *   VALUE (-0.0 is zero; a NaN channel makes the pixel valid, as `==` does), else 1.  One pass;
 *   16-byte loads when H*W % 4 == 0 and the pointers are aligned, per-pixel loads otherwise.
 *
 * nmsa_rmse_update: RootMeanSquaredError.update, metric/rmse.py:30-57
 *   *sum_state += sum over the selected pixels of sqrt(mean_c (pred - target)^2), *count_state +=
 *   their number.  Both are DEVICE pointers (the metric's f64 / i64 states); atomic adds, one per
 *   workgroup and state: no host sync, capturable in a hipGraph, a replay adds again.
 *   pred     f32|bf16|f16, widened to f32 before the subtraction (torch's type promotion)
 *   target   f32 [B,C,H,W], 1 <= C <= 8
 *   mask_mode NMSA_RMSE_MASK_NONE (mask NULL: every pixel), _GIVEN (mask u8 [B,H,W], non-0 = use),
 *            _FROM_TARGET (mask NULL, C == 3: the rule of nmsa_normal_valid_mask on `target`)
 *   source   Hs == 0 and Ws == 0: pred is [B,C,H,W].  Otherwise pred is [B,C,Hs,Ws] at the network
 *            resolution and target pixel (y, x) reads pred[.., y0 + sy(y), x0 + sx(x)] with the
 *            nearest-neighbour arithmetic of nmsa_resize_nearest over the valid region (y0, x0, h,
 *            w): `update(resize_nearest(pred[crop]), target)` without the full-resolution map.
 *   Per pixel: float32 subtract, square, sequential channel sum, divide by C, square root, every
 *   step IEEE-rounded; the sums are float64.  A pixel the mask leaves out contributes nothing
 *   whatever it holds (the reference gathers).  NMSA_ERR_ARG: NULL / non-positive arguments, C
 *   outside 1..8, a mask pointer that does not fit the mode, a valid region outside the source,
 *   planes above 2^30 pixels.  No workspace.
 * ------------------------------------------------------------------------- */
#define NMSA_RMSE_MASK_NONE 0
#define NMSA_RMSE_MASK_GIVEN 1
#define NMSA_RMSE_MASK_FROM_TARGET 2
int nmsa_normal_valid_mask(const float* target, int B, int H, int W, uint8_t* mask,
                           nmsa_stream_t stream);
int nmsa_rmse_update(const void* pred, int pred_dtype, const float* target, const uint8_t* mask,
                     int mask_mode, int B, int C, int H, int W,
                     int Hs, int Ws, int y0, int x0, int h, int w,
                     double* sum_state, int64_t* count_state, nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * orientation MAE on device tables (csrc/maae.hip)
 *
 * An ORIENTATION TABLE holds, per image, {integer key: angle in rad}:
 *   keys   i32 [B,K] ascending within the first n[b] columns, or NULL for a dense table (key =
 *          column index, every column looked at; n may then be NULL too)
 *   angle  f32 [B,K], valid u8 [B,K] (0: the column is no entry), n i32 [B], K > 0
 *   status i32 [1] or NULL: the status word of nmsa_instance_orientation_wide when that call made
 *          the table; its bits 1 / 32 are OR-ed into `status` as NMSA_ST_MAAE_WIDE_OVERFLOW /
 *          NMSA_ST_MAAE_WIDE_RANGE
 * An ID TABLE holds, per image, {panoptic id: instance id}: pan i64 [B,K], ins i64 [B,K], n i32 [B];
 *   `ascending` != 0 promises ascending pan rows (binary search), 0 makes every lookup walk the row
 *   (the tables of the merge kernels are in insertion order).
 *
 * nmsa_maae_update_keyed: MeanAbsoluteAngularError.update, metric/mae.py:40-64.  For every valid
 *   key of the prediction table the target angle under the same key of the same image is looked
 *   up; a key the target lacks (KeyError in the reference) raises NMSA_ST_MAAE_MISSING_TARGET and
 *   the pair is skipped.
 * nmsa_maae_update_matched: PanopticQualityWithOrientationMAE.update_mae, metric/mae.py:129-162, on
 *   the match table of nmsa_pq_update (matches i64 [B,match_capacity,2] (target id, pred id),
 *   n_matches i32 [B]).  Target id 0 is skipped; target id -> target instance -> target angle, then
 *   pred id -> pred instance -> pred angle; a pair counts when all four lookups hit.
 *   n_matches[b] > match_capacity raises NMSA_ST_MAAE_MATCH_OVERFLOW and the image contributes its
 *   first match_capacity rows.
 *
 * Both add to *sum_state (f64) the |angle error| of every counted pair and to *count_state (i64)
 * their number: DEVICE pointers into the metric's states.  The error is the float32 chain
 *   rem(x, m) = fmodf(x, m), plus m when the result is non-zero and negative
 *   e = fabsf(rem((rem(p, m) - rem(t, m)) + pi, m) - pi),  m = (float)(2 pi), pi = (float)M_PI
 * every step IEEE-rounded, e widened to f64.  One workgroup, fixed reduction order: two runs on the
 * same input give bit-identical states.  No workspace, no host sync; capturable in a hipGraph, a
 * replay adds again.  NMSA_ERR_ARG: NULL / non-positive arguments.
 * ------------------------------------------------------------------------- */
#define NMSA_ST_MAAE_MISSING_TARGET 64
#define NMSA_ST_MAAE_MATCH_OVERFLOW 128
#define NMSA_ST_MAAE_WIDE_OVERFLOW 256
#define NMSA_ST_MAAE_WIDE_RANGE 512
int nmsa_maae_update_keyed(const int32_t* pred_keys, const float* pred_angle, const uint8_t* pred_valid,
                           const int32_t* pred_n, int pred_K, const int32_t* pred_status,
                           const int32_t* target_keys, const float* target_angle,
                           const uint8_t* target_valid, const int32_t* target_n, int target_K,
                           const int32_t* target_status,
                           int B, double* sum_state, int64_t* count_state, int32_t* status,
                           nmsa_stream_t stream);
int nmsa_maae_update_matched(const int64_t* matches, const int32_t* n_matches, int match_capacity,
                             const int64_t* pred_ids_pan, const int64_t* pred_ids_ins,
                             const int32_t* pred_ids_n, int pred_ids_K, int pred_ids_ascending,
                             const int32_t* pred_keys, const float* pred_angle, const uint8_t* pred_valid,
                             const int32_t* pred_n, int pred_K, const int32_t* pred_status,
                             const int64_t* target_ids_pan, const int64_t* target_ids_ins,
                             const int32_t* target_ids_n, int target_ids_K, int target_ids_ascending,
                             const int32_t* target_keys, const float* target_angle,
                             const uint8_t* target_valid, const int32_t* target_n, int target_K,
                             const int32_t* target_status,
                             int B, double* sum_state, int64_t* count_state, int32_t* status,
                             nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * side-output targets (csrc/multiscale.hip)
 *
 * nmsa_multiscale_nearest: MultiscaleSupervisionGenerator._preprocess
 *   (data/preprocessing/multiscale_supervision.py:41-67) -> resize() with cv2.INTER_NEAREST
 *   (data/preprocessing/resize.py:95-161), for every key and every downscale of a batch in ONE
 *   launch: per descriptor, dst[p, y, x] = src[p, maps[row_map + y], maps[col_map + x]].
 *   staging_host   PINNED host memory, n_words 32-bit words, 8-byte aligned: n_desc descriptors
 *                  (16 words each) followed by the concatenated i32 index maps.  The maps are the
 *                  caller's: OpenCV's nearest rule evaluated on the host in double arithmetic.
 *   staging_device device memory of the same size; the call enqueues ONE asynchronous copy of the
 *                  staging buffer and the launch.  `block_begin` of every descriptor is written by
 *                  the call (into staging_host) before the copy.
 *   Elements move as raw bits of 1 << log2_size bytes (1, 2, 4, 8): no conversion of any kind.
 *   Every field and every map entry is checked on the host copy before anything is enqueued:
 *   NMSA_ERR_ARG for NULL / non-positive fields, a log2_size outside 0..3, misaligned pointers,
 *   map offsets outside the buffer, a map entry outside [0, H) / [0, W), planes * h * w above
 *   2^31 - 1, n_desc above NMSA_MULTISCALE_MAX_DESC.  No workspace, no host synchronisation;
 *   capturable in a hipGraph (a replay copies the pinned buffer again: a captured call needs a
 *   staging buffer that no later call rewrites).
 * ------------------------------------------------------------------------- */
#define NMSA_MULTISCALE_MAX_DESC 1024
typedef struct nmsa_multiscale_desc {
    uint64_t src;         /* device address of the source, [planes, H, W]                     */
    uint64_t dst;         /* device address of the destination, [planes, h, w]                */
    int32_t planes;       /* leading planes B * C                                             */
    int32_t H, W;         /* source side lengths                                              */
    int32_t h, w;         /* destination side lengths                                         */
    int32_t log2_size;    /* log2 of the element size in bytes                                */
    int32_t row_map;      /* word offset of the h row indices within the maps                 */
    int32_t col_map;      /* word offset of the w column indices within the maps              */
    int32_t block_begin;  /* first workgroup of this descriptor: written by the call          */
    int32_t reserved[3];
} nmsa_multiscale_desc;
int nmsa_multiscale_nearest(void* staging_host, void* staging_device, int n_desc, int n_words,
                            nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * batch augmentation (csrc/augment.hip)
 *
 * nmsa_batch_augment: RandomCrop (data/preprocessing/crop.py:57-73, the slices), then
 *   RandomHorizontalFlip (flip.py:40-47, np.flip(axis=1) of the crop), NormalizeRGB /
 *   NormalizeDepth (normalize.py:13-31, 109-122) and ToTorchTensors' HWC -> CHW (torch.py:31-38),
 *   for every key of a collated batch in ONE launch: per descriptor, sample b, channel c and
 *   output pixel (y, x),
 *     dst[b, c, y, x] = f(src[b, y0[b] + y, flip[b] ? x0[b] + w - 1 - x : x0[b] + x, c]).
 *   staging_host   PINNED host memory, n_words 32-bit words, 8-byte aligned: n_desc descriptors
 *                  (24 words each) followed by the per-sample parameters, n_samples triples of
 *                  int32 (y0, x0, flip), shared by all descriptors.
 *   staging_device device memory of the same size; the call enqueues ONE asynchronous copy of the
 *                  staging buffer and the launch.  `block_begin` and `pixels_per_lane` of every
 *                  descriptor are written by the call (into staging_host) before the copy.
 *   mode NMSA_AUGMENT_MOVE        elements move as raw bits of 1 << log2_size bytes (1, 2, 4, 8),
 *                                 [B,H,W,C] -> [B,C,h,w] ([B,H,W] is C == 1): no conversion of
 *                                 any kind, NaN payloads and -0.0 survive.
 *        NMSA_AUGMENT_RGB_NORM    uint8 [B,H,W,3] -> float32 [B,3,h,w], (float(v) - mean[c]) /
 *                                 std[c]: one IEEE subtract, then one IEEE divide.  mean / std are
 *                                 the caller's float32 values (numpy's float32(0.485) * 255, ...).
 *        NMSA_AUGMENT_DEPTH_NORM  uint16 (log2_size 1) or float32 (log2_size 2) [B,H,W] -> float32
 *                                 [B,1,h,w], (float(v) - mean[0]) / std[0]; with raw_depth, a
 *                                 source element with float(v) == invalid_depth_value is written
 *                                 as invalid_depth_value itself (-0.0 against 0.0 gives +0.0).
 *   Every field and every sample's window are checked on the host copy before anything is
 *   enqueued: NMSA_ERR_ARG for NULL or misaligned pointers (source: its element size,
 *   destination: its element size), non-positive fields, B != n_samples, h > H or w > W, a
 *   negative y0 / x0, y0 + h > H or x0 + w > W, a flip outside {0, 1}, an unknown mode, a
 *   log2_size the mode does not take, C != 3 for RGB_NORM or C != 1 for DEPTH_NORM, a std of 0,
 *   an out_dtype other than NMSA_F32 / NMSA_F16, B * C * h * w above 2^31 - 1, n_desc above
 *   NMSA_AUGMENT_MAX_DESC, n_words below the table and the parameters.  NMSA_ERR_UNSUPPORTED for
 *   out_dtype NMSA_F16 (the reference's `output_dtype='float16'`).  out_dtype is read for the
 *   two normalising modes only.  No workspace, no host synchronisation; capturable in a hipGraph
 *   (a replay copies the pinned buffer again: a captured call needs a staging buffer that no
 *   later call rewrites; parameters written into it between replays are NOT checked again, the
 *   writer keeps them inside the windows above).
 * ------------------------------------------------------------------------- */
#define NMSA_AUGMENT_MAX_DESC 256
#define NMSA_AUGMENT_MOVE 0
#define NMSA_AUGMENT_RGB_NORM 1
#define NMSA_AUGMENT_DEPTH_NORM 2
typedef struct nmsa_augment_desc {
    uint64_t src;               /* device address of the source, [B, H, W, C]                  */
    uint64_t dst;               /* device address of the destination, [B, C, h, w]             */
    int32_t B;                  /* samples: equals n_samples                                   */
    int32_t H, W;               /* source side lengths                                         */
    int32_t C;                  /* interleaved channels of the source, planes of the result    */
    int32_t h, w;               /* crop side lengths                                           */
    int32_t mode;               /* NMSA_AUGMENT_*                                              */
    int32_t log2_size;          /* log2 of the SOURCE element size in bytes                    */
    int32_t out_dtype;          /* NMSA_F32 (the normalising modes)                            */
    int32_t raw_depth;          /* DEPTH_NORM: keep invalid_depth_value                        */
    int32_t block_begin;        /* first workgroup of this descriptor: written by the call     */
    int32_t pixels_per_lane;    /* 4 where w % 4 == 0 and dst allows vector stores, else 1:
                                   written by the call                                         */
    float mean[3];              /* RGB_NORM: per channel; DEPTH_NORM: [0]                      */
    float std[3];
    float invalid_depth_value;
    int32_t reserved;
} nmsa_augment_desc;
int nmsa_batch_augment(void* staging_host, void* staging_device, int n_desc, int n_samples,
                       int n_words, nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * batch augmentation behind a resize (csrc/augment_resize.hip)
 *
 * nmsa_batch_augment_resized: the chain of nmsa_batch_augment behind RandomResize
 *   (data/preprocessing/resize.py:311-340) or behind RandomCrop's upscale of an image smaller
 *   than the crop (crop.py:43-55), in ONE launch that never forms the resized image: only the
 *   pixels of the crop window are resampled.  `rgb` is resized with cv2.INTER_LINEAR, everything
 *   else with cv2.INTER_NEAREST (resize.py:113-120).  The kernel sees no offset, flip or scale:
 *   the caller evaluates OpenCV's index and weight rules on the host and supplies, per sample, the
 *   tables of the crop window in OUTPUT coordinates (the column tables of a flipped sample
 *   reversed).  A batch that needs no resize takes nmsa_batch_augment.
 *   staging_host   PINNED host memory, n_words 32-bit words, 16-byte aligned: n_desc descriptors
 *                  (24 words each), then six int32 tables for the n_samples samples and the h x w
 *                  window that all descriptors share:
 *                    col_near [n_samples, w]   nearest source column
 *                    col_taps [n_samples, w]   i0 | i1 << 16: the two source columns of INTER_LINEAR
 *                    col_wts  [n_samples, w]   a0 | a1 << 16: their weights, a0 + a1 == 2048
 *                    row_near, row_taps, row_wts [n_samples, h]   the same for the rows
 *   staging_device device memory of the same size, 16-byte aligned; the call enqueues ONE
 *                  asynchronous copy of the staging buffer and the launch.  `block_begin` and
 *                  `pixels_per_lane` of every descriptor are written by the call.
 *   mode NMSA_AUGMENT_MOVE        dst[b, c, y, x] = src[b, row_near[b, y], col_near[b, x], c] as
 *                                 raw bits of 1 << log2_size bytes, any channel count
 *        NMSA_AUGMENT_DEPTH_NORM  the same gather, then as nmsa_batch_augment
 *        NMSA_AUGMENT_RGB_NORM    uint8 only.  Per channel, with (i0, i1, a0, a1) of the column
 *                                 and (j0, j1, b0, b1) of the row, in integer arithmetic as
 *                                 OpenCV's 8-bit INTER_LINEAR:
 *                                   R0 = S[j0, i0] * a0 + S[j0, i1] * a1, R1 the same in row j1,
 *                                   v = (((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16) + 2) >> 2
 *                                 then (float(v) - mean[c]) / std[c] as nmsa_batch_augment.
 *   Every field and every table entry is checked on the host copy before anything is enqueued:
 *   NMSA_ERR_ARG for what nmsa_batch_augment refuses in a descriptor, for descriptors that do not
 *   share one h x w, for a nearest entry outside [0, H) / [0, W) of any descriptor, a tap outside
 *   [0, H) / [0, W) of an RGB_NORM descriptor, an RGB_NORM source side above 65536, a weight above
 *   2048, staging that is not 16-byte aligned, n_words below the descriptors and the tables.
 *   NMSA_ERR_UNSUPPORTED for out_dtype NMSA_F16.  No workspace, no host synchronisation;
 *   capturable in a hipGraph (tables written into the pinned buffer between replays are NOT
 *   checked again: the writer runs these checks).
 * ------------------------------------------------------------------------- */
typedef struct nmsa_augment_resize_desc {
    uint64_t src;               /* device address of the source, [B, H, W, C]                  */
    uint64_t dst;               /* device address of the destination, [B, C, h, w]             */
    int32_t B;                  /* samples: equals n_samples                                   */
    int32_t H, W;               /* source side lengths (what the table entries index)          */
    int32_t C;                  /* interleaved channels of the source, planes of the result    */
    int32_t h, w;               /* crop window side lengths: the same in every descriptor      */
    int32_t mode;               /* NMSA_AUGMENT_*                                              */
    int32_t log2_size;          /* log2 of the SOURCE element size in bytes                    */
    int32_t out_dtype;          /* NMSA_F32 (the normalising modes)                            */
    int32_t raw_depth;          /* DEPTH_NORM: keep invalid_depth_value                        */
    int32_t block_begin;        /* first workgroup of this descriptor: written by the call     */
    int32_t pixels_per_lane;    /* 4 where w % 4 == 0 and dst allows vector stores, else 1:
                                   written by the call                                         */
    float mean[3];              /* RGB_NORM: per channel; DEPTH_NORM: [0]                      */
    float std[3];
    float invalid_depth_value;
    int32_t reserved;
} nmsa_augment_resize_desc;
int nmsa_batch_augment_resized(void* staging_host, void* staging_device, int n_desc, int n_samples,
                               int n_words, nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * scene classification (csrc/scene.hip)
 *
 * nmsa_scene_step: the scene task's whole step in ONE launch of one workgroup — softmax score and
 *   argmax (model/postprocessing/scene.py:42-44), the loss and its gradient (task_helper/scene.py:
 *   37-42, 61-63: torch.nn.CrossEntropyLoss(weight, label_smoothing, ignore_index=-1,
 *   reduction='mean') on labels - 1) and the confusion-matrix update (scene.py:104-108).
 *   logits        [B, C] contiguous, NMSA_F32 | NMSA_BF16 | NMSA_F16; 1 <= C <=
 *                 NMSA_SCENE_MAX_CLASSES, B >= 1.  Values are promoted exactly; the row arithmetic
 *                 is float64 and every output is rounded once to its type.
 *   labels        [B], NMSA_U8 | NMSA_I32 | NMSA_I64, or NULL: batch['scene'], 0 = void, class c
 *                 is label c + 1.  A label outside 0..C raises NMSA_ST_VALUE_RANGE in `status`
 *                 and its row is treated as void.
 *   class_weights float [C] or NULL; label_smoothing in [0, 1]: as torch.nn.CrossEntropyLoss.
 *   Outputs, each may be NULL (= not wanted, nothing is written for it):
 *   score    float [B]    max(softmax(logits, dim=1))
 *   idx      i64 [B]      index of the largest logit, the first one among equal logits
 *   loss     float [3]    numerator (sum of the rows' weighted terms), divisor (sum of
 *                         w[target] over the non-void rows, their count without weights) and the
 *                         quotient, which is the loss; no non-void row: 0 / 0 = NaN, as torch
 *   grad     [B, C] in the logits' dtype: d loss / d logits for an upstream gradient of 1; zero
 *                         in void rows
 *   confmat  i64 [C, C]   ACCUMULATED: confmat[label - 1, idx] += 1 for every non-void row
 *   status   i32 [1]      device word, OR-ed with NMSA_ST_VALUE_RANGE
 *   loss, grad and confmat need labels.  Deterministic: a fixed order of summation, no float
 *   atomics.  No workspace, no host synchronisation; capturable in a hipGraph (a replay adds to
 *   `confmat` again).  Everything is checked before anything is enqueued, with or without a
 *   device: NMSA_ERR_ARG for NULL logits, B < 1, C outside 1..NMSA_SCENE_MAX_CLASSES, a
 *   label_smoothing outside [0, 1] (NaN included), loss / grad / confmat without labels;
 *   NMSA_ERR_UNSUPPORTED for any other logits_dtype or (with labels) label_dtype.
 * ------------------------------------------------------------------------- */
#define NMSA_SCENE_MAX_CLASSES 4096
/* a row holding a NaN or a +inf, or all -inf: score NaN, idx 0 (softmax -> max), confusion-matrix column 0; its gradient row is NaN, also when void */
int nmsa_scene_step(const void* logits, int logits_dtype, const void* labels, int label_dtype,
                    int B, int C, const float* class_weights, float label_smoothing,
                    float* score, int64_t* idx, float* loss, void* grad, int64_t* confmat,
                    int32_t* status, nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * learned x2 upsampling of the decoder heads (csrc/upsampling.hip)
 *     model/upsampling.py:39-96, modes 'learned-3x3' (zeropad = 0) and 'learned-3x3-zeropad'
 *     (zeropad = 1): nearest x2, replication / zero pad, depthwise 3x3 convolution.
 *
 *   y[n,c,Y,X] = b[c] + sum_{i,j in 0..2} W[c,0,i,j] * U(Y+i-1, X+j-1)
 *   U(p,q)     = x[n,c,p>>1,q>>1] for 0 <= p < 2h, 0 <= q < 2w;  replicate: p, q clamped to that
 *                range first;  zeropad: 0 outside it
 *
 *   x, gx      [B,C,h,w]   NMSA_F32 | NMSA_BF16 | NMSA_F16, contiguous; one dtype per call
 *   y, gy      [B,C,2h,2w] the same dtype
 *   weight, gweight  f32 [C,1,3,3];  bias, gbias  f32 [C] (bias may be NULL: no bias)
 *   Products and sums are float32 (fused multiply-adds on pre-added weight pairs); a half output
 *   is rounded once, to nearest even.
 *
 * nmsa_upsample2x_dw3x3_fwd: one launch, x read once, y written once, no workspace.
 * nmsa_upsample2x_dw3x3_bwd: gx = d/dx, gweight = d/dW, gbias = d/db of sum(gy * y); each of the
 *   three may be NULL (not wanted; all NULL: NMSA_OK after the checks, nothing is launched).  One
 *   launch over gy and x writes gx and ten partial sums per workgroup into `workspace`; a second,
 *   small launch sums them per channel in a fixed order.  No float atomics: two calls on the same
 *   inputs give the same bits.  `workspace` (16-byte aligned, at least
 *   nmsa_upsample2x_dw3x3_bwd_workspace_bytes(B, C, h, w) bytes, any dtype) is needed only with
 *   gweight or gbias; its contents are scratch.  zeropad: the gy of an edge row / column also enters the taps
 *   that lie on the padding there, times 0: nothing for a finite gy, NaN for a NaN or an infinity, as the
 *   zero-padded convolution of torch gives.
 * nmsa_upsample2x_dw3x3_route (host only, nothing is launched, no device is touched): the route a
 *   call with these two tensors takes.  NMSA_UP_ROUTE_VECTOR: a lane owns 2 (f32) or 4 (half)
 *   consecutive input pixels and moves 16-byte vectors; taken when w % 2 == 0 (f32) / w % 4 == 0
 *   (half) and EVERY tensor of the call (x and y; gy, x and gx) starts on 16 bytes.
 *   NMSA_UP_ROUTE_PIXEL: one input pixel per lane, element-wise accesses, any width and any
 *   element-aligned pointer.  `x` is an input-sized tensor of the call, `y_or_gx` another of its
 *   tensors (forward: y; backward: gx, and once more with gy — the call takes the vector route
 *   when every answer is NMSA_UP_ROUTE_VECTOR).
 *
 * Everything is checked before anything is enqueued, with or without a device.  NMSA_ERR_ARG: a
 * NULL x / y / gy / weight, a dtype other than the three, B, C, h or w below 1, zeropad other than
 * 0 / 1, a pointer that is not aligned to its element, a NULL or misaligned workspace where one is
 * needed.  NMSA_ERR_WORKSPACE: a workspace that is too small.  NMSA_ERR_UNSUPPORTED: a single
 * output plane of 2^31 elements or more (4hw; offsets inside a plane are 32-bit, the plane base is
 * 64-bit, so B*C*4hw may exceed 2^31), B*C above 2^31 - 1, 2^31 or more workgroup items.  No host
 * synchronisation, no allocation; capturable in a hipGraph as a single chain.
 * ------------------------------------------------------------------------- */
#define NMSA_UP_ROUTE_VECTOR 1
#define NMSA_UP_ROUTE_PIXEL 2
int nmsa_upsample2x_dw3x3_route(const void* x, const void* y_or_gx, int dtype,
                                int B, int C, int h, int w);
int nmsa_upsample2x_dw3x3_fwd(const void* x, int dtype, const float* weight, const float* bias,
                              int B, int C, int h, int w, int zeropad, void* y,
                              nmsa_stream_t stream);
size_t nmsa_upsample2x_dw3x3_bwd_workspace_bytes(int B, int C, int h, int w);
int nmsa_upsample2x_dw3x3_bwd(const void* gy, const void* x, int dtype, const float* weight,
                              int B, int C, int h, int w, int zeropad,
                              void* gx, float* gweight, float* gbias,
                              void* workspace, size_t workspace_bytes, nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * Swin encoder-decoder fusion (csrc/ln_transpose.hip)
 *     model/encoder_decoder_fusion.py:123-148, names 'swin-ln-*': LayerNorm over C of the encoder's
 *     NHWC skip tensor, NHWC -> NCHW, optionally the addition of the decoder features.
 *
 *   y[b,c,p]  = ((x[b,p,c] - mean_bp) * rstd_bp) * gamma[c] + beta[c] (+ add[b,c,p])
 *   gx[b,p,:] = rstd * (a - mean_c(a) - xh * mean_c(a * xh)),   a = gy * gamma, xh = (x - mean) * rstd
 *   ggamma[c] = sum_bp gy * xh,   gbeta[c] = sum_bp gy
 *
 *   x, gx         [B,P,C], P = H*W, C contiguous   NMSA_F32 | NMSA_BF16 | NMSA_F16 (dtype_x)
 *   y, gy, add    [B,C,P]                          dtype_y = dtype_x or NMSA_F32
 *   gamma, beta, ggamma, gbeta   f32 [C];   mean, rstd   f32 [B*P]
 *   Arithmetic: float32 after converting the inputs, no fused multiply-adds.  Every sum over C is a
 *   tree of depth at most ceil(log2 C) + 2 (a lane's values pairwise, the lanes by halves);
 *   mean = S / (float)C, var = sum((x - mean)^2) / (float)C (two passes over the row, IEEE division),
 *   rstd = 1.0f / sqrtf(var + eps), correctly rounded.  A half output is rounded once, to nearest even.
 *
 * nmsa_ln_nhwc_nchw_fwd: one launch; x is read twice, the second time right after the first
 *   (from cache where the tiles in flight fit it), y written once in runs of 32 pixels.  `add` may be NULL.  mean and rstd are written when both are
 *   non-NULL (training) and must both be NULL otherwise.
 * nmsa_ln_nhwc_nchw_bwd: gx, ggamma, gbeta of sum(gy * y); each of the three may be NULL (not wanted;
 *   all NULL: NMSA_OK after the checks, nothing is launched).  One launch over gy and x writes gx
 *   and one line [2][C] of partial sums per workgroup into `workspace`; a second, small launch adds
 *   the lines in a fixed order.  No float atomics: two calls on the same inputs give the same bits;
 *   the grid depends on (B, P, C) and the device geometry only.  `workspace` (16-byte aligned, at
 *   least nmsa_ln_nhwc_nchw_bwd_workspace_bytes(B, P, C) bytes) is needed only with ggamma or gbeta;
 *   its contents are scratch.  The gradient of `add` is gy itself.
 * nmsa_ln_nhwc_nchw_route (host only, nothing is launched, no device is touched): the route a call
 *   with these two tensors takes.  NMSA_LNT_ROUTE_VECTOR: 16-byte accesses on both sides; taken when
 *   C % vx == 0 and P % vy == 0 (vx, vy = 4 for a float32, 8 for a half dtype_x / dtype_y) and EVERY
 *   tensor of the call (fwd: x, y and add; bwd: gy, x and gx) starts on 16 bytes.
 *   NMSA_LNT_ROUTE_ELEMENT: element-wise accesses, any C <= 2048, any P, any element-aligned
 *   pointer.  `x` is an [B,P,C] tensor of the call, `y` a [B,C,P] one; a call takes the vector route
 *   when the answer is NMSA_LNT_ROUTE_VECTOR for every such pair of its tensors.
 *
 * Everything is checked before anything is enqueued, with or without a device.  NMSA_ERR_ARG: a
 * NULL x / y / gy / gamma / beta, in bwd a NULL mean / rstd, in fwd exactly one of mean / rstd NULL,
 * dtype_x not one of the three, dtype_y neither dtype_x nor NMSA_F32, B, P or C below 1, eps negative
 * or not finite (0 is legal), a pointer that is not aligned to its element, a NULL or misaligned
 * workspace where one is needed.  NMSA_ERR_WORKSPACE: a workspace that is too small.
 * NMSA_ERR_UNSUPPORTED: C above 2048, B*P*C of 2^31 or more.  No host synchronisation, no
 * allocation; capturable in a hipGraph as a single chain.
 * ------------------------------------------------------------------------- */
#define NMSA_LNT_ROUTE_VECTOR 1
#define NMSA_LNT_ROUTE_ELEMENT 2
#define NMSA_LNT_MAX_CHANNELS 2048
int nmsa_ln_nhwc_nchw_route(const void* x, const void* y, int dtype_x, int dtype_y,
                            int B, int P, int C);
int nmsa_ln_nhwc_nchw_fwd(const void* x, int dtype_x, const float* gamma, const float* beta, float eps,
                          const void* add, int B, int P, int C, void* y, int dtype_y,
                          float* mean, float* rstd, nmsa_stream_t stream);
size_t nmsa_ln_nhwc_nchw_bwd_workspace_bytes(int B, int P, int C);
int nmsa_ln_nhwc_nchw_bwd(const void* gy, int dtype_y, const void* x, int dtype_x, const float* gamma,
                          const float* mean, const float* rstd, int B, int P, int C,
                          void* gx, float* ggamma, float* gbeta,
                          void* workspace, size_t workspace_bytes, nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * context module: pyramid pooling and its concatenation (csrc/context_module.hip)
 *     model/context_module/ppm.py, appm.py: n adaptive average pools of x, (torch: a 1x1
 *     ConvNormAct per branch), every branch resized back to H x W and concatenated behind x.
 *
 *   x, gx      [B,C,H,W]             NMSA_F32 | NMSA_BF16 | NMSA_F16, contiguous; ONE dtype per call
 *   pooled_i, gp_i  [B,C,ph_i,pw_i]  i < n_bins <= NMSA_PPM_MAX_BINS, each its own contiguous tensor
 *   y_i, gy_i  [B,cr_i,ph_i,pw_i]    the branch outputs
 *   out, g_out [B, C + sum(cr_i), H, W]
 *   ph, pw, cr and the pointer arrays are HOST arrays of n_bins entries, read during the call and
 *   carried in the kernel arguments: they may be reused or freed when the call returns.
 *   Arithmetic: float32 after converting the inputs; a half output is rounded once, to nearest even.
 *
 * nmsa_ppm_pool_fwd: ONE launch, x read once.  ATen's windows: rows floor(i*H/ph) .. ceil((i+1)*H/ph)-1,
 *   columns alike (ph > H included).  pooled = S / float(area), IEEE division, S = the row sums of
 *   the window added top to bottom, a row sum = its elements added left to right, both from 0.
 * nmsa_ppm_pool_bwd: ONE launch, gather form: gx[h,w] = the sum over the bins in order, within a
 *   bin over the cells whose window holds (h,w) in row-major order, of gp_i[cell] / float(area(cell)),
 *   added from 0.  A NULL gp_i: that branch adds nothing (its gradient is zero).
 * nmsa_ppm_upcat_fwd: ONE launch.  out[:, 0..C) = x, element for element; behind it branch i,
 *   y_i resized to H x W with `mode` NMSA_PPM_NEAREST or NMSA_PPM_BILINEAR (align_corners = False)
 *   in ATen's float arithmetic: scale = float(ph)/float(H); nearest: src = min(int(floorf(dst*scale)),
 *   ph-1); bilinear: s = max(scale*(dst+0.5f)-0.5f, 0), i0 = min(int(s), ph-1), i1 = min(i0+1, ph-1),
 *   w1 = s-i0, w0 = 1-w1, value = (a*wx0 + b*wx1)*wy0 + (c*wx0 + d*wx1)*wy1 with one fused
 *   multiply-add per sum.
 * nmsa_ppm_upcat_bwd: ONE launch, the transposed resize in gather form:
 *   gy_i[p,q] = sum_h wy(h,p) * (sum_w wx(w,q) * g_out[C+off_i+c, h, w]) over the output rows h that
 *   read p (ascending) and the columns w that read q (ascending), fused multiply-adds from 0; wy, wx
 *   are the weights above (1 for nearest; w0 + w1 where i0 == i1 at the border).  A NULL gy_i: not
 *   wanted (all NULL: NMSA_OK after the checks, nothing is launched).  The gradient of x through the
 *   concatenation is the view g_out[:, 0..C) and needs no kernel.
 * No atomics, no workspace: two calls on the same inputs give the same bits.
 *
 * nmsa_ppm_route (host only, nothing is launched, no device is touched): the route pool_fwd and
 *   upcat_bwd take for this geometry (pool_bwd and upcat_fwd have one route).  NMSA_PPM_ROUTE_LDS: a
 *   wave stages its plane in LDS and the lanes share the row segments, then the cells; taken when
 *   H*W <= 2048 and H*pw_i <= 512 for every branch.  NMSA_PPM_ROUTE_GLOBAL: a lane owns a cell and
 *   walks its window in memory; any size.  Both routes add in the same order and give the same bits.
 *
 * Everything is checked before anything is enqueued, with or without a device.  NMSA_ERR_ARG: a
 * dtype other than the three, B, C, H or W below 1, n_bins outside 1..NMSA_PPM_MAX_BINS, a NULL
 * ph / pw / cr / pointer array, a ph_i, pw_i or cr_i below 1, a mode other than the two, a NULL x /
 * gx / out / g_out / pooled_i / y_i, a pointer that is not aligned to its element.
 * NMSA_ERR_UNSUPPORTED: H, W, ph_i or pw_i above 32768 (offsets inside a plane are 32-bit, the
 * plane base is 64-bit), B*C or B*(C + sum cr_i) above 2^31 - 1, 2^31 or more work items.  No host
 * synchronisation, no allocation; every call is capturable in a hipGraph.
 * ------------------------------------------------------------------------- */
#define NMSA_PPM_MAX_BINS 4
#define NMSA_PPM_NEAREST 0
#define NMSA_PPM_BILINEAR 1
#define NMSA_PPM_ROUTE_LDS 1
#define NMSA_PPM_ROUTE_GLOBAL 2
int nmsa_ppm_route(int H, int W, int n_bins, const int* ph, const int* pw);
int nmsa_ppm_pool_fwd(const void* x, int dtype, int B, int C, int H, int W, int n_bins,
                      const int* ph, const int* pw, void* const* pooled, nmsa_stream_t stream);
int nmsa_ppm_pool_bwd(const void* const* gp, int dtype, int B, int C, int H, int W, int n_bins,
                      const int* ph, const int* pw, void* gx, nmsa_stream_t stream);
int nmsa_ppm_upcat_fwd(const void* x, const void* const* ys, int dtype, int B, int C, int H, int W,
                       int n_bins, const int* cr, const int* ph, const int* pw, int mode,
                       void* out, nmsa_stream_t stream);
int nmsa_ppm_upcat_bwd(const void* g_out, int dtype, int B, int C, int H, int W, int n_bins,
                       const int* cr, const int* ph, const int* pw, int mode, void* const* gys,
                       nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * MLP decoders: every branch resized into the concatenation (csrc/mlp_decoder.hip)
 *     model/decoder/mlp_base.py: the embedded main map (1/32) and skips (1/16, 1/8, 1/4) resized to
 *     the 1/4-resolution grid and concatenated in front of the 1x1 `fuse` convolution (torch: one
 *     interpolate per branch and a cat).
 *
 *   out[b, off_i + c, Y, X] = resize(y_i[b, c], H x W),   off_i = c_0 + ... + c_(i-1)
 *   y_i, gy_i  [B, c_i, H >> s_i, W >> s_i]   i < n <= NMSA_MLPDEC_MAX_BRANCHES, s_i in 0..4, each its
 *                                             own contiguous tensor
 *   out, g_out [B, sum(c_i), H, W]            NMSA_F32 | NMSA_BF16 | NMSA_F16, ONE dtype per call
 *   c, s and the pointer arrays are HOST arrays of n entries, read during the call and carried in the
 *   kernel arguments: they may be reused or freed when the call returns.  H and W are multiples of
 *   1 << s_i for every branch.
 *   Arithmetic: exactly that of nmsa_ppm_upcat_fwd / _bwd above (ATen's float index arithmetic with
 *   scale = float(h)/float(H), the blend (a*wx0 + b*wx1)*wy0 + (c*wx0 + d*wx1)*wy1 with one fused
 *   multiply-add per sum, backward in gather form with fused multiply-adds from 0, left to right,
 *   then top to bottom, weights w0 + w1 where i0 == i1); float32 inside, a half output is rounded
 *   once.  `mode` is NMSA_MLPDEC_NEAREST or NMSA_MLPDEC_BILINEAR (align_corners = False).
 *   A branch with s_i == 0 is copied element for element.  Stated deviation: ATen's scale-1 bilinear
 *   turns -0 into +0 and an inf next to a zero weight into NaN; the copy keeps both.
 *
 * nmsa_mlpdec_upcat_fwd: ONE launch, every output element written once.
 * nmsa_mlpdec_upcat_bwd: ONE launch; a lane owns a source pixel and gathers its footprint (at most
 *   2f x 2f output pixels bilinear, f x f nearest, f = 1 << s_i).  A NULL gy_i: not wanted (all NULL:
 *   NMSA_OK after the checks, nothing is launched).  The gradient of a branch with s_i == 0 is the view
 *   g_out[:, off_i .. off_i + c_i) and needs no kernel: pass NULL for it (a pointer gets the same
 *   values through the gather, one pixel per lane; a -0 arrives as +0).
 * No atomics, no workspace: every call and every route gives the same bits.
 *
 * nmsa_mlpdec_route (host only, nothing is launched, no device is touched): the route upcat_fwd takes
 *   with these tensors (upcat_bwd has one route).  NMSA_MLPDEC_ROUTE_VECTOR: a lane produces 4
 *   (float32) or 8 (half) consecutive pixels of a row and stores 16 bytes; taken when W is a multiple
 *   of that count and EVERY tensor of the call (out and every y_i) starts on 16 bytes.
 *   NMSA_MLPDEC_ROUTE_ELEMENT: one pixel per lane, any width, any element-aligned pointer.  Both
 *   routes give the same bits.
 *
 * Everything is checked before anything is enqueued, with or without a device.  NMSA_ERR_ARG: a
 * dtype other than the three, a mode other than the two, B, H, W or a c_i below 1, n outside
 * 1..NMSA_MLPDEC_MAX_BRANCHES, an s_i outside 0..4, H or W not a multiple of 1 << s_i, a NULL c / s /
 * pointer array, a NULL out / g_out / y_i, a pointer that is not aligned to its element.
 * NMSA_ERR_UNSUPPORTED (after those): H or W above 32768 (offsets inside a plane are 32-bit, the plane
 * base is 64-bit), B * sum(c_i) above 2^31 - 1, 2^31 or more work items.  No host synchronisation, no
 * allocation; both calls are capturable in a hipGraph.
 * ------------------------------------------------------------------------- */
#define NMSA_MLPDEC_MAX_BRANCHES 4
#define NMSA_MLPDEC_NEAREST 0
#define NMSA_MLPDEC_BILINEAR 1
#define NMSA_MLPDEC_ROUTE_VECTOR 1
#define NMSA_MLPDEC_ROUTE_ELEMENT 2
int nmsa_mlpdec_route(const void* const* ys, const void* out, int dtype, int H, int W, int n,
                      const int* s);
int nmsa_mlpdec_upcat_fwd(const void* const* ys, int dtype, int B, int H, int W, int n, const int* c,
                          const int* s, int mode, void* out, nmsa_stream_t stream);
int nmsa_mlpdec_upcat_bwd(const void* g_out, int dtype, int B, int H, int W, int n, const int* c,
                          const int* s, int mode, void* const* gys, nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * encoder RGB-D fusion: SE-weighted add (csrc/encoder_fusion.hip)
 *     model/encoder_fusion.py, names 'se-add*': per modality m (0 = rgb, 1 = depth) a squeeze-and-
 *     excitation weighting of the feature map, then the sum of the two weighted maps.
 *
 *   s_m[b,c]  = mean over the plane of x_m[b,c]
 *   z1_m = W1_m s_m + b1_m,   h_m = act(z1_m),   w_m = sigmoid(W2_m h_m + b2_m)       R = C / 16 (floor)
 *   y[b,c,p]  = x_rgb[b,c,p] * w_rgb[b,c] + x_depth[b,c,p] * w_depth[b,c]
 *   gw_m[b,c] = sum over the plane of gy * x_m
 *   gz2_m = gw_m * w_m * (1 - w_m),  gh_m = W2_m^T gz2_m,  gz1_m = gh_m * act'(z1_m),  gs_m = W1_m^T gz1_m
 *   gx_m[b,c,p] = gy[b,c,p] * w_m[b,c] + gs_m[b,c] / (H*W)
 *
 *   x_rgb, x_depth, y, gy, gx_rgb, gx_depth  [B,C,H,W] contiguous, NMSA_F32 | NMSA_BF16 | NMSA_F16,
 *                                            ONE dtype per call
 *   s, w, gw, gz2, gs  f32 [2,B,C];   z1, gz1, h  f32 [2,B,R];   the modality is the outer index
 *   W1 f32 [R,C], b1 f32 [R], W2 f32 [C,R], b2 f32 [C] per modality.  `params` is a HOST array of 8
 *   pointers (W1, b1, W2, b2 of rgb, then of depth), `weights` one of 4 (W1, W2 of rgb, then of
 *   depth); both are read during the call and may be reused when it returns.
 *   `act` is NMSA_SEFUSE_ACT_RELU (h = 0 at z1 <= 0 and z1 elsewhere, a NaN included; gz1 = 0 at z1 <= 0 whatever gh
 *   is and gh elsewhere, a NaN z1 included: a selection, ATen's threshold backward) or
 *   NMSA_SEFUSE_ACT_SILU (z sig(z); act' = sig(z) * (1 + z * (1 - sig(z)))).
 *
 *   Arithmetic: float32 after converting the inputs; a half output is rounded once, to nearest even.
 *   Plane sums (squeeze, weight_grad): the plane is cut into chunks of V = 4 (float32) / 8 (half)
 *   consecutive elements; with T = 64 lanes (NMSA_SEFUSE_ROUTE_WAVE, H*W <= NMSA_SEFUSE_WAVE_PLANE_MAX)
 *   or T = 1024 lanes (NMSA_SEFUSE_ROUTE_BLOCK) lane t owns chunks t, t + T, ... and keeps V partial
 *   sums, one per position in the chunk, each added in ascending chunk order from 0 (weight_grad: fused
 *   multiply-adds of gy and x).  A lane's partials are added pairwise ((a0 + a1) + (a2 + a3)) + ...,
 *   the 64 lanes of a wave by halves (l += l + 32, 16, 8, 4, 2, 1), the 16 waves of the BLOCK route in
 *   wave order.  s = S / float(H*W), IEEE division.  The order depends on H*W and the dtype only.
 *   excite: z1[r] = (sum_c W1[r,c] s[c]) + b1[r], lane l of a wave adding c = l, l + 64, ... as fused
 *   multiply-adds from 0, the lanes by halves; w[c] = 1 / (1 + expf(-((sum_r W2[c,r] h[r]) + b2[c]))),
 *   fused multiply-adds from 0 in ascending r, IEEE division.  excite_bwd: gz2 = (gw * w) * (1 - w);
 *   gh like z1 (over c), gs like the sum of w (over r).
 *   scale_add: the two products and their sum, each rounded to float32.  apply_bwd: the product, the
 *   IEEE quotient gs / float(H*W) and their sum, each rounded to float32.
 *
 * nmsa_sefuse_squeeze: ONE launch, s of both modalities.
 * nmsa_sefuse_excite: ONE launch, one workgroup per (modality, image); writes w and, when z1 is not
 *   NULL (training), z1.
 * nmsa_sefuse_scale_add: ONE launch.
 * nmsa_sefuse_weight_grad: ONE launch, both modalities from one read of gy.  A NULL x_m: that half of
 *   gw is not wanted and not written (both NULL: NMSA_OK after the checks, nothing is launched).
 * nmsa_sefuse_excite_bwd: ONE launch; writes gz2, gz1, gs and h (= act(z1), recomputed) of the
 *   modalities whose W1 and W2 are both given; both NULL: that modality is not wanted and its halves
 *   are not written (all four NULL: NMSA_OK after the checks, nothing is launched).
 * nmsa_sefuse_apply_bwd: ONE launch.  A NULL gx_m: not wanted (both NULL: NMSA_OK after the checks).
 * No atomics, no workspace, no hand-off between workgroups: two calls on the same inputs give the same
 * bits.  The four map kernels launch at most 8 workgroups of 256 lanes (BLOCK route: 2 of 1024) per
 * compute unit of nmsa_device_geometry and LOOP over the rest of their items.
 *
 * nmsa_sefuse_route (host only, nothing is launched, no device is touched): the routes a map call
 *   with the tensors t0, t1, t2 (t1, t2 may be NULL: not part of the call) takes, two bits or-ed.
 *   NMSA_SEFUSE_ROUTE_VECTOR: 16-byte accesses; taken when H*W is a multiple of V and EVERY tensor of
 *   the call starts on 16 bytes.  NMSA_SEFUSE_ROUTE_ELEMENT: element-wise accesses, any H*W, any
 *   element-aligned pointer.  Both give the same bits (in the plane sums a lane reads the same chunks
 *   either way).  NMSA_SEFUSE_ROUTE_WAVE / NMSA_SEFUSE_ROUTE_BLOCK: how squeeze and weight_grad cut a
 *   plane (see above; scale_add and apply_bwd have no such split).
 *
 * Everything is checked before anything is enqueued, with or without a device.  NMSA_ERR_ARG: a dtype
 * other than the three, an activation other than the two, B, H or W below 1, C below 16, a NULL
 * pointer where none is allowed (every tensor except x_m of weight_grad, gx_m of apply_bwd, z1 of
 * excite and whole modalities of `weights`), only one of W1 / W2 of a modality in `weights`, a pointer
 * that is not aligned to its element.  NMSA_ERR_UNSUPPORTED (after those): B*C*H*W of 2^31 or more
 * (map calls), C above NMSA_SEFUSE_MAX_CHANNELS (excite, excite_bwd).  No host synchronisation, no
 * allocation; every call is capturable in a hipGraph as a single chain.
 * ------------------------------------------------------------------------- */
#define NMSA_SEFUSE_ACT_RELU 0
#define NMSA_SEFUSE_ACT_SILU 1
#define NMSA_SEFUSE_ROUTE_VECTOR 1
#define NMSA_SEFUSE_ROUTE_ELEMENT 2
#define NMSA_SEFUSE_ROUTE_WAVE 4
#define NMSA_SEFUSE_ROUTE_BLOCK 8
#define NMSA_SEFUSE_WAVE_PLANE_MAX 2048
#define NMSA_SEFUSE_MAX_CHANNELS 2048
int nmsa_sefuse_route(const void* t0, const void* t1, const void* t2, int dtype, int H, int W);
int nmsa_sefuse_squeeze(const void* x_rgb, const void* x_depth, int dtype, int B, int C, int H, int W,
                        float* s, nmsa_stream_t stream);
int nmsa_sefuse_excite(const float* s, const float* const* params, int act, int B, int C, float* w,
                       float* z1, nmsa_stream_t stream);
int nmsa_sefuse_scale_add(const void* x_rgb, const void* x_depth, int dtype, const float* w, int B,
                          int C, int H, int W, void* y, nmsa_stream_t stream);
int nmsa_sefuse_weight_grad(const void* gy, const void* x_rgb, const void* x_depth, int dtype, int B,
                            int C, int H, int W, float* gw, nmsa_stream_t stream);
int nmsa_sefuse_excite_bwd(const float* gw, const float* w, const float* z1,
                           const float* const* weights, int act, int B, int C, float* gz2, float* gz1,
                           float* gs, float* h, nmsa_stream_t stream);
int nmsa_sefuse_apply_bwd(const void* gy, int dtype, const float* w, const float* gs, int B, int C,
                          int H, int W, void* gx_rgb, void* gx_depth, nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * residual blocks: the fused batch-norm tail (csrc/block_tail.hip)
 *     model/block.py, every norm-to-activation segment of BasicBlock, Bottleneck and NonBottleneck1D:
 *     batch normalization, the Dropout2d scale, the residual add and the activation.
 *
 *   training: mean_c = sum(x) / M,  var_c = sum((x - mean_c)^2) / M,  M = B*H*W      eval: running_mean, running_var
 *   invstd = 1 / sqrt(var + eps)    xh = (x - mean) * invstd    u = xh * gamma + beta
 *   v = u * s[b,c]  (s NULL: u)     z = v + id  (id NULL: v)    y = act(z)
 *   gz = gy * act'(z)    gid = gz    gu = gz * s    dbeta = sum(gu)    dgamma = sum(gu * xh)
 *   training: gx = (gamma * invstd) * ((gu - dbeta / M) - xh * (dgamma / M))     eval: gx = (gamma * invstd) * gu
 *
 *   x, identity, y, gy, gx, gid  [B,C,H,W] contiguous, NMSA_F32 | NMSA_BF16 | NMSA_F16, ONE dtype per call
 *   scale  [B,C] of the same dtype (the Dropout2d scale, 0 or 1 / (1 - p))
 *   gamma, beta, running_mean, running_var, save_mean, save_invstd, mean, invstd, dgamma, dbeta  f32 [C]
 *   part  f32 [C, U, 2], U = B * ceil(H*W / NMSA_BNTAIL_SEGMENT): the caller's workspace of
 *         nmsa_bntail_workspace_bytes(B, C, H, W) bytes, written by a reduction and read by the launch behind it
 *   `act` is NMSA_BNTAIL_ACT_RELU (y = 0 where z <= 0 and z elsewhere, so a NaN z gives NaN as torch.relu does;
 *   act' = 0 where the SAVED OUTPUT y <= 0 and 1 elsewhere, a NaN y included: ATen's threshold backward on the
 *   in-place result; `aux` is y) or NMSA_BNTAIL_ACT_SILU (z sig(z); act' = sig(z) * (1 + z * (1 - sig(z))) with z RECOMPUTED
 *   from x, scale and the identity; `aux` is the identity or NULL).
 *
 *   Arithmetic: float32 after converting the inputs, every operation above rounded on its own (no contraction
 *   except where stated); a half output is rounded once, to nearest even.
 *   Summation order.  A plane is cut into segments of NMSA_BNTAIL_SEGMENT = 2048 consecutive elements; a segment of
 *   a plane is a UNIT, u = b * segments + segment.  A unit is cut into chunks of V = 4 (float32) / 8 (half)
 *   elements; lane t of 64 owns chunks t, t + 64, ... of the segment and keeps V partial sums, one per position in
 *   the chunk, each added in ascending chunk order from 0; they are added pairwise ((a0 + a1) + (a2 + a3)) + ...,
 *   then the 64 lanes by halves (l += l + 32, 16, 8, 4, 2, 1).
 *   stats: mean_u = S_u / float(n_u) (IEEE division), then M2_u = sum (x - mean_u)^2 over the SAME values as fused
 *   multiply-adds in the same order (two passes over registers; never E[x^2] - E[x]^2).
 *   Merging the U units of a channel: lane l of 64 takes the units l, l + 64, ... in ascending order, then the lanes by
 *   halves.  (n, mean, M2) pairs merge by Chan's formula, a <- a + b: n = na + nb, d = mb - ma, r = nb / n,
 *   mean = ma + d * r, M2 = (M2a + M2b) + (d * d) * (na * r); an empty side is skipped.  (sum gu, sum gu * xh) pairs
 *   merge by addition.  var = M2 / float(M); the running update is rm = (1 - m) * rm + m * mean,
 *   rv = (1 - m) * rv + m * (M2 / float(M - 1)).  invstd = 1 / sqrt(var + eps), IEEE square root and division.
 *   The order depends on B, H*W and the dtype only: not on the route, the grid or the device.
 *
 * nmsa_bntail_stats: ONE launch; part[c, u] = (mean_u, M2_u).
 * nmsa_bntail_apply: ONE launch.  part given: training (the partials of nmsa_bntail_stats on the same x are merged by
 *   every wave; the running statistics are UPDATED; B*H*W below 2: NMSA_ERR_ARG); part NULL: eval (the running
 *   statistics are READ).  save_mean / save_invstd (both or neither): the statistics the backward pass takes.
 * nmsa_bntail_bwd_reduce: ONE launch; part[c, u] = (sum gu, sum gu * xh).  With dgamma / dbeta (both or neither) it
 *   FINISHES ALONE, for a backward pass without a map gradient and for eval mode: one workgroup per channel, the
 *   same merge, the same bits.
 * nmsa_bntail_bwd_apply: ONE launch.  part given: the training formula (the partials of nmsa_bntail_bwd_reduce are
 *   merged by every wave, dgamma / dbeta written when given); part NULL: the eval formula, no sums, dgamma / dbeta
 *   must be NULL.  A NULL gx / gid: not wanted (nothing wanted: NMSA_OK after the checks, nothing is launched).
 * No atomics, nothing handed between workgroups inside a launch: two calls on the same inputs give the same bits.
 * Every kernel launches at most 8 workgroups of 256 lanes per compute unit of nmsa_device_geometry and LOOPS over
 * the rest of its units, four per workgroup and trip.
 *
 * nmsa_bntail_route (host only, nothing is launched, no device is touched): NMSA_BNTAIL_ROUTE_VECTOR (16-byte
 *   accesses: H*W a multiple of V and EVERY map of the call, t0 .. t4, NULL: not part of it, on 16 bytes) or
 *   NMSA_BNTAIL_ROUTE_ELEMENT (element-wise accesses, any H*W, any element-aligned pointer); both give the same
 *   bits.  *segments (may be NULL): the units a plane is cut into.
 *
 * Everything is checked before anything is enqueued, with or without a device.  NMSA_ERR_ARG: a dtype other than
 * the three, an activation other than the two, B, C, H or W below 1, B*C*H*W of 2^31 or more (32-bit offsets), a
 * NULL pointer where none is allowed (allowed: identity, scale, save_*, part of apply; aux under SiLU, beta under
 * ReLU, scale, dgamma, dbeta, gx, gid, part of bwd_apply), only one of a pair, a pointer that is not aligned to
 * its element, a workspace smaller than nmsa_bntail_workspace_bytes.  No host synchronisation, no allocation;
 * every call is capturable in a hipGraph as a single chain.
 * ------------------------------------------------------------------------- */
#define NMSA_BNTAIL_ACT_RELU 0
#define NMSA_BNTAIL_ACT_SILU 1
#define NMSA_BNTAIL_ROUTE_VECTOR 1
#define NMSA_BNTAIL_ROUTE_ELEMENT 2
#define NMSA_BNTAIL_SEGMENT 2048
size_t nmsa_bntail_workspace_bytes(int B, int C, int H, int W);
int nmsa_bntail_route(const void* t0, const void* t1, const void* t2, const void* t3, const void* t4,
                      int dtype, int H, int W, int* segments);
int nmsa_bntail_stats(const void* x, int dtype, int B, int C, int H, int W, float* part,
                      size_t part_bytes, nmsa_stream_t stream);
int nmsa_bntail_apply(const void* x, const void* identity, const void* scale, int dtype, int B, int C,
                      int H, int W, const float* gamma, const float* beta, const float* part,
                      size_t part_bytes, float* running_mean, float* running_var, float eps,
                      float momentum, int act, float* save_mean, float* save_invstd, void* y,
                      nmsa_stream_t stream);
int nmsa_bntail_bwd_reduce(const void* gy, const void* x, const void* aux, const void* scale, int dtype,
                           int B, int C, int H, int W, const float* gamma, const float* beta,
                           const float* mean, const float* invstd, int act, float* part,
                           size_t part_bytes, float* dgamma, float* dbeta, nmsa_stream_t stream);
int nmsa_bntail_bwd_apply(const void* gy, const void* x, const void* aux, const void* scale, int dtype,
                          int B, int C, int H, int W, const float* gamma, const float* beta,
                          const float* mean, const float* invstd, int act, const float* part,
                          size_t part_bytes, void* gx, void* gid, float* dgamma, float* dbeta,
                          nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * the stem max pool of the ResNet backbones (csrc/maxpool.hip)
 *     model/backbone/resnet.py, `maxpool` = nn.MaxPool2d(kernel_size=3, stride=2, padding=1): dilation 1, floor
 *     mode, Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1.
 *
 *   x, gx   [B,C,H,W]    NMSA_F32 | NMSA_BF16 | NMSA_F16, contiguous; ONE dtype per call
 *   y, gy   [B,C,Ho,Wo]  the same dtype
 *   code    u8 [B,C,Ho,Wo]: 3 * (r - (2 oy - 1)) + (c - (2 ox - 1)), 0..8, the window position of the input pixel
 *           (r, c) that ATen's max_pool2d_with_indices names with its int64 index r * W + c
 *
 *   Selection (ATen's rule, explicit comparisons, no fmax): the window positions inside the map in row-major
 *   order, starting at the first, the choice replaced when `val > max || isnan(val)`.  Ties, signed zeros
 *   included, keep the first position; a window holding NaNs selects its last NaN; an all -inf window its first
 *   position.  y carries the selected element's bits.
 *
 * nmsa_maxpool3x3s2_fwd: ONE launch, x read once, y written once, no workspace.  `code` may be NULL: no code is
 *   written (inference).
 * nmsa_maxpool3x3s2_bwd: ONE launch in gather form.  gx[r,c] = the sum of gy[oy,ox] over the at most four windows
 *   that cover (r, c) and whose code points at it, oy ascending, then ox ascending, added in float32 from 0; a
 *   half output is rounded once, to nearest even.  EVERY gx element is written (no memset is needed), no atomics:
 *   two calls on the same inputs give the same bits.  A code above 8 points nowhere.
 * nmsa_maxpool3x3s2_route (host only, nothing is launched, no device is touched): the route a call with these two
 *   tensors takes.  NMSA_MP_ROUTE_VECTOR: a lane owns 2 (f32) or 4 (half) consecutive output pixels and moves its
 *   4 / 8 input (gx) elements of a row as one 16-byte vector; taken when W % 4 == 0 (f32) / W % 8 == 0 (half) and
 *   EVERY tensor of the call (x, y and code; gy, code and gx) starts on 16 bytes.  NMSA_MP_ROUTE_PIXEL: one
 *   output pixel per lane, element-wise accesses, any width and any element-aligned pointer.  Both give the
 *   same bits.  `x` is an input-sized tensor of the call, `y_or_gx` another of its tensors (the call takes the
 *   vector route when every answer is NMSA_MP_ROUTE_VECTOR).
 * Every kernel launches at most 8 workgroups of 256 lanes per compute unit of nmsa_device_geometry and LOOPS over
 * the rest of the planes and tiles.
 *
 * Everything is checked before anything is enqueued, with or without a device.  NMSA_ERR_ARG: a NULL x / y / gy /
 * gx, a NULL code in the backward call, a dtype other than the three, B, C, H or W below 1, a pointer that is
 * not aligned to its element.  NMSA_ERR_UNSUPPORTED: a plane of 2^31 elements or more (H W; offsets inside a
 * plane are 32-bit, the plane base is 64-bit, so B*C*H*W may exceed 2^31), B*C above 2^31 - 1, 2^31 or more lane
 * units (B*C * ceil(Ho / 8) * Wo on the one-pixel route).  No host synchronisation, no allocation; capturable in
 * a hipGraph as a single chain.
 * ------------------------------------------------------------------------- */
#define NMSA_MP_ROUTE_VECTOR 1
#define NMSA_MP_ROUTE_PIXEL 2
int nmsa_maxpool3x3s2_route(const void* x, const void* y_or_gx, int dtype, int B, int C, int H, int W);
int nmsa_maxpool3x3s2_fwd(const void* x, int dtype, int B, int C, int H, int W, void* y, uint8_t* code,
                          nmsa_stream_t stream);
int nmsa_maxpool3x3s2_bwd(const void* gy, const uint8_t* code, int dtype, int B, int C, int H, int W, void* gx,
                          nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * the scene classification decoder (csrc/scene_head.hip)
 *     model/decoder/scene.py: adaptive_avg_pool2d(x, 1) -> flatten -> nn.Linear, the producer of the [B,K] logits
 *     nmsa_scene_step consumes.
 *
 *   x, gx            [B,C,H,W]  NMSA_F32 | NMSA_BF16 | NMSA_F16 (dtype_x), contiguous
 *   weight, gweight  f32 [K,C]
 *   bias, gbias      f32 [K]; bias may be NULL (no bias is added)
 *   pooled           f32 [B,C]; NULL in the forward call: not wanted (inference)
 *   logits, g        [B,K] in dtype_out / dtype_g, any of the three, independent of dtype_x
 *
 * nmsa_scene_head_fwd: ONE launch (one workgroup per image), no workspace.  With V = 4 (f32) / 8 (half) the plane
 *   of H W elements is cut into chunks of V consecutive elements (the last one short); chunk j belongs to lane
 *   j % 64.  A lane adds the elements of its chunks in ascending order to a float32 0; the 64 lane sums are
 *   combined by halves (v[l] += v[l + o] for o = 32, 16, 8, 4, 2, 1); pooled[b,c] = S / float(H W), IEEE
 *   division.  H W == 1: pooled = x, converted, no division and no sum.  logits[b,k]: lane l starts from a
 *   float32 0 and takes acc = fma(weight[k,c], pooled[b,c], acc) for c = l, l + 64, ..; the 64 lane sums are
 *   combined by halves as above; then + bias[k] (one add, skipped for a NULL bias) and ONE rounding to dtype_out.
 * nmsa_scene_head_bwd: ONE launch, no atomics, no workspace, no hand-off between workgroups; any of gx, gweight
 *   and gbias may be NULL (not wanted; all three NULL: NMSA_OK after the checks, nothing is launched).
 *     gs[b,c]      = fma(g[b,k], weight[k,c], gs) from a float32 0, k ascending
 *     gx[b,c,:]    = gs[b,c] / float(H W) (H W == 1: gs[b,c]), rounded once to dtype_x, the whole plane written
 *     gweight[k,c] = fma(g[b,k], pooled[b,c], acc) from a float32 0, b ascending
 *     gbias[k]     = acc + g[b,k] from a float32 0, b ascending
 *   g is converted to float32 exactly.  Every order above depends on (H W, C, K, B, dtypes) alone: two calls on the
 *   same inputs give the same bits, on every route and with any grid.  The grid is at most 8 workgroups of 256
 *   lanes per compute unit of nmsa_device_geometry and LOOPS over the rest of the items (a wave per plane — a
 *   lane per plane when H W == 1 —, a lane per gweight element, a lane per gbias element).
 * nmsa_scene_head_route (host only, nothing is launched, no device is touched): the route of a call whose map (x
 *   in the forward, gx in the backward call) is `x_or_gx`.  NMSA_SH_ROUTE_UNIT: H W == 1.  NMSA_SH_ROUTE_VECTOR: a
 *   chunk is one 16-byte access; taken when H W % 4 == 0 (f32) / H W % 8 == 0 (half) and the map starts on 16
 *   bytes.  NMSA_SH_ROUTE_ELEMENT: element-wise accesses, any size and any element-aligned pointer.  All give the
 *   same bits.
 *
 * Everything is checked before anything is enqueued, with or without a device.  NMSA_ERR_ARG: a dtype other than
 * the three, B, C, H, W or K below 1, a NULL x / weight / logits (forward), g / pooled / weight (backward) or map
 * (route), a pointer that is not aligned to its element.  NMSA_ERR_UNSUPPORTED: C above
 * NMSA_SCENE_HEAD_MAX_CHANNELS (pooled[b,:] is kept in the forward's LDS), K above NMSA_SCENE_MAX_CLASSES, a plane
 * of 2^31 elements or more, 2^31 or more wave items (B C + ceil(K C / 64) + ceil(K / 64)).  No host
 * synchronisation, no allocation; capturable in a hipGraph as a single chain.
 * ------------------------------------------------------------------------- */
#define NMSA_SCENE_HEAD_MAX_CHANNELS 2048
#define NMSA_SH_ROUTE_UNIT 1
#define NMSA_SH_ROUTE_VECTOR 2
#define NMSA_SH_ROUTE_ELEMENT 4
int nmsa_scene_head_route(const void* x_or_gx, int dtype_x, int B, int C, int H, int W, int K);
int nmsa_scene_head_fwd(const void* x, int dtype_x, int B, int C, int H, int W, const float* weight,
                        const float* bias, float* pooled, void* logits, int dtype_out, int K,
                        nmsa_stream_t stream);
int nmsa_scene_head_bwd(const void* g, int dtype_g, const float* pooled, const float* weight, int B, int C, int H,
                        int W, int K, void* gx, int dtype_x, float* gweight, float* gbias, nmsa_stream_t stream);

/* ---------------------------------------------------------------------------
 * dense decoders: x2 upsampling and the addition of the encoder skip (csrc/up_add.hip)
 *     model/decoder/dense_base.py: the end of every decoder module, `Upsampling` (x2), and the `add` of
 *     model/encoder_decoder_fusion.py that follows it (torch: an upsampling pass and an addition pass).
 *
 *   y[n,c,Y,X] = u[n,c,Y,X] + skip[n,c,Y,X],   u = up(x)
 *   x          [B,C,h,w]    NMSA_F32 | NMSA_BF16 | NMSA_F16, contiguous; ONE dtype per call
 *   skip, y    [B,C,2h,2w]  the same dtype, contiguous
 *   weight f32 [C,1,3,3], bias f32 [C] (may be NULL: no bias): read in the two learned modes only
 *   mode  NMSA_UPADD_NEAREST          u = x[n,c,Y>>1,X>>1]: y is one IEEE addition
 *         NMSA_UPADD_BILINEAR         ATen's align_corners = False rule at scale 0.5 (source indices and
 *                                     weights of every output row and column as ATen computes them, the
 *                                     blend (a*wx0 + b*wx1)*wy0 + (c*wx0 + d*wx1)*wy1 with one fused
 *                                     multiply-add per sum).  A clamped border tap is multiplied by its
 *                                     zero weight: an infinity next to the border gives ATen's NaN.
 *         NMSA_UPADD_LEARNED          u of nmsa_upsample2x_dw3x3_fwd with zeropad = 0: the same formula,
 *         NMSA_UPADD_LEARNED_ZEROPAD  halo rules and operation order; with zeropad = 1
 *   Everything is float32 inside; a half output is rounded once, to nearest even, AFTER the addition
 *   (the composition rounds u as well).
 *
 * nmsa_up2x_add_fwd: ONE launch, x and skip read once, y written once; no workspace, no atomics.  There
 *   is no backward entry point: the gradient of skip is the upstream gradient itself, the gradient of x
 *   (weight, bias) is that of the upsampling alone (nmsa_upsample2x_dw3x3_bwd; nmsa_mlpdec_upcat_bwd with
 *   one branch of factor 2 for nearest / bilinear).
 * nmsa_up2x_add_route (host only, nothing is launched, no device is touched): the route the forward call
 *   takes with these tensors.  NMSA_UPADD_ROUTE_VECTOR: a lane owns 2 (f32) or 4 (half) consecutive input
 *   pixels and moves 16-byte vectors of skip and y; taken when w % 2 == 0 (f32) / w % 4 == 0 (half) and x,
 *   skip and y all start on 16 bytes.  NMSA_UPADD_ROUTE_PIXEL: one input pixel per lane, element-wise
 *   accesses, any width and any element-aligned pointer.  Both routes give the same bits.
 *
 * Everything is checked before anything is enqueued, with or without a device.  NMSA_ERR_ARG: a NULL
 * x / skip / y, a NULL weight in a learned mode, a dtype other than the three, a mode other than the
 * four, B, C, h or w below 1, a pointer that is not aligned to its element, a y whose bytes overlap
 * those of x or skip.  NMSA_ERR_UNSUPPORTED: a single output plane of 2^31 elements or more (4hw; offsets
 * inside a plane are 32-bit, the plane base is 64-bit, so B*C*4hw may exceed 2^31), B*C above 2^31 - 1,
 * 2^31 or more workgroup items.  No host synchronisation, no allocation; capturable in a hipGraph.
 * ------------------------------------------------------------------------- */
#define NMSA_UPADD_NEAREST 0
#define NMSA_UPADD_BILINEAR 1
#define NMSA_UPADD_LEARNED 2
#define NMSA_UPADD_LEARNED_ZEROPAD 3
#define NMSA_UPADD_ROUTE_VECTOR 1
#define NMSA_UPADD_ROUTE_PIXEL 2
int nmsa_up2x_add_route(const void* x, const void* skip, const void* y, int dtype, int B, int C, int h, int w);
int nmsa_up2x_add_fwd(const void* x, int dtype, int mode, const float* weight, const float* bias,
                      const void* skip, int B, int C, int h, int w, void* y, nmsa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NMSA_H */
