// augment_resize.hip — batch augmentation behind a resize: RandomResize (or the upscale of an image
// smaller than the crop), crop, horizontal flip, normalise and HWC -> CHW of every key of a
// collated batch in ONE launch, without ever forming the resized image.
//
// Sibling of augment.hip (which a batch that needs no resize keeps taking) for the chain
//   RandomResize._preprocess          (data/preprocessing/resize.py:311-340)
//   RandomCrop._preprocess            (data/preprocessing/crop.py:41-73, the upscale included)
//   RandomHorizontalFlip, NormalizeRGB / NormalizeDepth, ToTorchTensors as in augment.hip
// where resize() (resize.py:95-161) is cv2.INTER_LINEAR for `rgb` and cv2.INTER_NEAREST for
// everything else.  Only the pixels of the crop window are resampled.
//
//   k_batch_augment_resized   one descriptor per key; the kernel never sees a crop offset, a flip
//                     or a scale: per sample b the caller supplies, in OUTPUT coordinates of the
//                     crop window (the column tables of a flipped sample already reversed),
//                       col_near[b, x], row_near[b, y]   nearest source column / row
//                       col_taps[b, x], row_taps[b, y]   i0 | i1 << 16, the two linear taps
//                       col_wts[b, x],  row_wts[b, y]    a0 | a1 << 16, their weights of 2048
//                     MOVE        raw bits of 1, 2, 4 or 8 bytes through the nearest tables
//                     DEPTH_NORM  u16 / f32 through the nearest tables, then as augment.hip
//                     RGB_NORM    u8 through the linear tables, OpenCV's 8-bit fixed-point passes
//                                   R  = S[i0] * a0 + S[i1] * a1                      (per row tap)
//                                   v  = (((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16) + 2) >> 2
//                                 then (float(v) - mean[c]) / std[c].  All resampling arithmetic is
//                                 integer: R <= 255 * 2048, b * (R >> 4) <= 2048 * 32640 < 2^31.
//
// Lane mapping: augment.hip's.  A lane owns `pixels_per_lane` consecutive output pixels of one output
// row and all their channels; with w % 4 == 0 and a 16-byte aligned destination it owns 4, loads its
// four column entries of a table as ONE 16-byte load (the tables start on 16 bytes and every row of
// them is a multiple of 16 bytes long then) and stores one 16-byte vector per plane.  The row entries
// are the same for every lane of a row.  The gathers are per pixel: neighbouring output pixels of an
// upscaled sample share source pixels, which the caches serve; no tap is kept across pixels.
//
// Every table entry that left the source would be a GPU fault, so the entry point checks every
// entry, with every descriptor field, on the host copy BEFORE anything is enqueued; whoever rewrites
// the tables between replays of a captured call owns those checks.
#include "augment_ops.hpp"

namespace nmsa {
namespace {

constexpr int AUGR_THREADS = 256;
constexpr int AUGR_DESC_WORDS = 24;
constexpr int AUGR_WEIGHT_ONE = 2048;           // OpenCV's INTER_RESIZE_COEF_SCALE

static_assert(sizeof(nmsa_augment_resize_desc) == AUGR_DESC_WORDS * 4, "the staging layout is 24 words per descriptor");
static_assert(AUGR_DESC_WORDS % 4 == 0, "the tables behind the descriptors start on 16 bytes");

// the six tables behind the descriptors, [B, w] x 3 then [B, h] x 3
struct window_tables {
    const int32_t *col_near, *col_taps, *col_wts, *row_near, *row_taps, *row_wts;
    __device__ __forceinline__ window_tables(const int32_t* t, uint32_t B, uint32_t h, uint32_t w)
        : col_near(t), col_taps(t + (size_t)B * w), col_wts(t + 2 * (size_t)B * w),
          row_near(t + 3 * (size_t)B * w), row_taps(t + 3 * (size_t)B * w + (size_t)B * h),
          row_wts(t + 3 * (size_t)B * w + 2 * (size_t)B * h) {}
};

// where pixel group g of a descriptor lies
struct group_at {
    uint32_t x, row, b;         // first output column; b * h + y; sample
    template <int NP>
    __device__ __forceinline__ static group_at of(const nmsa_augment_resize_desc& d, uint32_t g)
    {
        const uint32_t G = (uint32_t)d.w / NP;                    // NP == 4 only where w % 4 == 0
        const uint32_t row = g / G;
        return {(g % G) * NP, row, row / (uint32_t)d.h};
    }
};

// S source element, D destination element, CT channels (0: read from the descriptor), NP pixels per lane
template <typename S, typename D, int CT, int NP, typename Op>
__device__ __forceinline__ void resized_nearest(const nmsa_augment_resize_desc& d, const window_tables& t,
                                                uint32_t g, const Op& op)
{
    const group_at at = group_at::of<NP>(d, g);
    const uint32_t w = (uint32_t)d.w, h = (uint32_t)d.h;
    const uint32_t C = CT ? (uint32_t)CT : (uint32_t)d.C;
    const pack<int32_t, NP> cx = *(const pack<int32_t, NP>*)(t.col_near + (size_t)at.b * w + at.x);
    const uint32_t sy = (uint32_t)t.row_near[at.row];
    const S* src = (const S*)d.src + ((size_t)at.b * d.H + sy) * d.W * C;
    const size_t plane = (size_t)h * w;
    D* dst = (D*)d.dst + (size_t)at.b * C * plane + (size_t)(at.row - at.b * h) * w + at.x;
    if constexpr (CT != 0) {
        S in[NP][CT];
#pragma unroll
        for (int j = 0; j < NP; ++j) __builtin_memcpy(in[j], src + (size_t)(uint32_t)cx.v[j] * CT, sizeof(in[j]));
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            pack<D, NP> out;
#pragma unroll
            for (int j = 0; j < NP; ++j) out.v[j] = op(in[j][c], c);
            *(pack<D, NP>*)(dst + c * plane) = out;
        }
    } else {
        for (uint32_t c = 0; c < C; ++c) {
            pack<D, NP> out;
#pragma unroll
            for (int j = 0; j < NP; ++j) out.v[j] = op(src[(size_t)(uint32_t)cx.v[j] * C + c], (int)c);
            *(pack<D, NP>*)(dst + c * plane) = out;
        }
    }
}

// OpenCV's INTER_LINEAR on 8-bit pixels: the horizontal pass of one source row for one output pixel
__device__ __forceinline__ void linear_row(const uint8_t* row, uint32_t i0, uint32_t i1, int a0, int a1, int (&R)[3])
{
    uint8_t p0[3], p1[3];
    __builtin_memcpy(p0, row + (size_t)i0 * 3, 3);
    __builtin_memcpy(p1, row + (size_t)i1 * 3, 3);
#pragma unroll
    for (int c = 0; c < 3; ++c) R[c] = (int)p0[c] * a0 + (int)p1[c] * a1;
}

template <int NP>
__device__ __forceinline__ void resized_linear_rgb(const nmsa_augment_resize_desc& d, const window_tables& t,
                                                   uint32_t g, const op_rgb_norm& op)
{
    const group_at at = group_at::of<NP>(d, g);
    const uint32_t w = (uint32_t)d.w, h = (uint32_t)d.h;
    const pack<int32_t, NP> ct = *(const pack<int32_t, NP>*)(t.col_taps + (size_t)at.b * w + at.x);
    const pack<int32_t, NP> cw = *(const pack<int32_t, NP>*)(t.col_wts + (size_t)at.b * w + at.x);
    const uint32_t rt = (uint32_t)t.row_taps[at.row], rw = (uint32_t)t.row_wts[at.row];
    const int b0 = (int)(rw & 0xffffu), b1 = (int)(rw >> 16);
    const uint8_t* image = (const uint8_t*)d.src + (size_t)at.b * d.H * d.W * 3;
    const uint8_t* row0 = image + (size_t)(rt & 0xffffu) * d.W * 3;
    const uint8_t* row1 = image + (size_t)(rt >> 16) * d.W * 3;
    const size_t plane = (size_t)h * w;
    float* dst = (float*)d.dst + (size_t)at.b * 3 * plane + (size_t)(at.row - at.b * h) * w + at.x;
    pack<float, NP> out[3];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const uint32_t taps = (uint32_t)ct.v[j], wts = (uint32_t)cw.v[j];
        const uint32_t i0 = taps & 0xffffu, i1 = taps >> 16;
        const int a0 = (int)(wts & 0xffffu), a1 = (int)(wts >> 16);
        int R0[3], R1[3];
        linear_row(row0, i0, i1, a0, a1, R0);
        linear_row(row1, i0, i1, a0, a1, R1);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int v = (((b0 * (R0[c] >> 4)) >> 16) + ((b1 * (R1[c] >> 4)) >> 16) + 2) >> 2;
            out[c].v[j] = op((uint8_t)v, c);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) *(pack<float, NP>*)(dst + c * plane) = out[c];
}

template <typename S, typename D, int CT, typename Op>
__device__ __forceinline__ void resized_ppl(const nmsa_augment_resize_desc& d, const window_tables& t,
                                            uint32_t g, const Op& op)
{
    if (d.pixels_per_lane == 4) resized_nearest<S, D, CT, 4>(d, t, g, op);
    else resized_nearest<S, D, CT, 1>(d, t, g, op);
}

template <typename T>
__device__ __forceinline__ void resized_move(const nmsa_augment_resize_desc& d, const window_tables& t, uint32_t g)
{
    if (d.C == 1) resized_ppl<T, T, 1>(d, t, g, op_move{});
    else if (d.C == 3) resized_ppl<T, T, 3>(d, t, g, op_move{});
    else resized_ppl<T, T, 0>(d, t, g, op_move{});
}

__global__ __launch_bounds__(AUGR_THREADS) void k_batch_augment_resized(
    const nmsa_augment_resize_desc* __restrict__ table, int n_desc, const int32_t* __restrict__ tables)
{
    // table[i].block_begin <= blockIdx.x < table[i + 1].block_begin; the same for every lane
    int lo = 0, hi = n_desc;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((uint32_t)table[mid].block_begin <= blockIdx.x) lo = mid; else hi = mid;
    }
    const nmsa_augment_resize_desc d = table[lo];
    // pixel groups of the descriptor: B * h * (w / pixels_per_lane) <= B * C * h * w < 2^31, checked
    const uint32_t groups = (uint32_t)d.B * (uint32_t)d.h * ((uint32_t)d.w / (uint32_t)d.pixels_per_lane);
    const uint32_t g = (blockIdx.x - (uint32_t)d.block_begin) * AUGR_THREADS + threadIdx.x;
    if (g >= groups) return;
    const window_tables t(tables, (uint32_t)d.B, (uint32_t)d.h, (uint32_t)d.w);
    if (d.mode == NMSA_AUGMENT_RGB_NORM) {
        const op_rgb_norm op{{d.mean[0], d.mean[1], d.mean[2]}, {d.std[0], d.std[1], d.std[2]}};
        if (d.pixels_per_lane == 4) resized_linear_rgb<4>(d, t, g, op);
        else resized_linear_rgb<1>(d, t, g, op);
    } else if (d.mode == NMSA_AUGMENT_DEPTH_NORM) {
        const op_depth_norm op{d.mean[0], d.std[0], d.invalid_depth_value, d.raw_depth != 0};
        if (d.log2_size == 1) resized_ppl<uint16_t, float, 1>(d, t, g, op);
        else resized_ppl<float, float, 1>(d, t, g, op);
    } else {
        switch (d.log2_size) {
            case 0: resized_move<uint8_t>(d, t, g); break;
            case 1: resized_move<uint16_t>(d, t, g); break;
            case 2: resized_move<uint32_t>(d, t, g); break;
            default: resized_move<uint64_t>(d, t, g); break;
        }
    }
}

// smallest and largest entry of n words; for packed words, of both 16-bit halves
struct span {
    int64_t lo, hi;
};
span span_of(const int32_t* p, int64_t n, bool packed)
{
    span s{INT64_MAX, INT64_MIN};
    for (int64_t i = 0; i < n; ++i) {
        if (packed) {
            const int64_t a = (uint32_t)p[i] & 0xffffu, b = (uint32_t)p[i] >> 16;
            s.lo = a < s.lo ? a : s.lo; s.lo = b < s.lo ? b : s.lo;
            s.hi = a > s.hi ? a : s.hi; s.hi = b > s.hi ? b : s.hi;
        } else {
            s.lo = p[i] < s.lo ? p[i] : s.lo;
            s.hi = p[i] > s.hi ? p[i] : s.hi;
        }
    }
    return s;
}

}  // namespace
}  // namespace nmsa

extern "C" int nmsa_batch_augment_resized(void* staging_host, void* staging_device, int n_desc, int n_samples,
                                          int n_words, nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    // 16 bytes: a lane loads four table entries at once
    if (!staging_host || !staging_device || n_desc <= 0 || n_desc > NMSA_AUGMENT_MAX_DESC || n_samples <= 0 ||
        (uintptr_t)staging_host % 16 != 0 || (uintptr_t)staging_device % 16 != 0)
        return NMSA_ERR_ARG;
    const int64_t table_words = (int64_t)n_desc * AUGR_DESC_WORDS;
    if ((int64_t)n_words < table_words) return NMSA_ERR_ARG;
    nmsa_augment_resize_desc* table = (nmsa_augment_resize_desc*)staging_host;
    // one crop window, so one set of tables, for all descriptors
    const int64_t B = n_samples, h = table[0].h, w = table[0].w;
    if (h <= 0 || w <= 0 || B * h > 0x7fffffffLL || B * w > 0x7fffffffLL ||
        (int64_t)n_words < table_words + 3 * B * (h + w))
        return NMSA_ERR_ARG;
    const int32_t* tabs = (const int32_t*)staging_host + table_words;
    const span col_near = span_of(tabs, B * w, false), col_taps = span_of(tabs + B * w, B * w, true),
               col_wts = span_of(tabs + 2 * B * w, B * w, true);
    const int32_t* rows = tabs + 3 * B * w;
    const span row_near = span_of(rows, B * h, false), row_taps = span_of(rows + B * h, B * h, true),
               row_wts = span_of(rows + 2 * B * h, B * h, true);
    if (col_near.lo < 0 || row_near.lo < 0 || col_wts.hi > AUGR_WEIGHT_ONE || row_wts.hi > AUGR_WEIGHT_ONE)
        return NMSA_ERR_ARG;
    int64_t blocks = 0;
    for (int i = 0; i < n_desc; ++i) {
        nmsa_augment_resize_desc& d = table[i];
        if (!d.src || !d.dst || d.B != n_samples || d.H <= 0 || d.W <= 0 || d.C <= 0 || d.h != h || d.w != w)
            return NMSA_ERR_ARG;
        uint64_t dst_size;
        if (d.mode == NMSA_AUGMENT_MOVE) {
            if (d.log2_size < 0 || d.log2_size > 3) return NMSA_ERR_ARG;
            dst_size = (uint64_t)1 << d.log2_size;
        } else if (d.mode == NMSA_AUGMENT_RGB_NORM || d.mode == NMSA_AUGMENT_DEPTH_NORM) {
            const bool rgb = d.mode == NMSA_AUGMENT_RGB_NORM;
            if (rgb ? (d.C != 3 || d.log2_size != 0) : (d.C != 1 || (d.log2_size != 1 && d.log2_size != 2)))
                return NMSA_ERR_ARG;
            for (int c = 0; c < d.C; ++c)
                if (d.std[c] == 0.0f) return NMSA_ERR_ARG;
            if (d.out_dtype == NMSA_F16) return NMSA_ERR_UNSUPPORTED;     // the reference's output_dtype
            if (d.out_dtype != NMSA_F32) return NMSA_ERR_ARG;
            // the taps are 16-bit halves of a word
            if (rgb && (d.H > 65536 || d.W > 65536 || row_taps.hi >= d.H || col_taps.hi >= d.W)) return NMSA_ERR_ARG;
            dst_size = 4;
        } else {
            return NMSA_ERR_ARG;
        }
        if (row_near.hi >= d.H || col_near.hi >= d.W) return NMSA_ERR_ARG;
        if (d.src % ((uint64_t)1 << d.log2_size) != 0 || d.dst % dst_size != 0) return NMSA_ERR_ARG;
        int64_t elements = (int64_t)d.B * d.C;
        if (elements > 0x7fffffffLL || (elements *= d.h) > 0x7fffffffLL || (elements *= d.w) > 0x7fffffffLL)
            return NMSA_ERR_ARG;
        const uint64_t vec_bytes = dst_size * 4 > 16 ? 16 : dst_size * 4;
        d.pixels_per_lane = (d.w % 4 == 0 && d.dst % vec_bytes == 0) ? 4 : 1;
        d.block_begin = (int32_t)blocks;
        const int64_t groups = (int64_t)d.B * d.h * (d.w / d.pixels_per_lane);
        blocks += (groups + AUGR_THREADS - 1) / AUGR_THREADS;
        if (blocks > 0x7fffffffLL) return NMSA_ERR_ARG;
    }
    if (check_hip(hipMemcpyAsync(staging_device, staging_host, (size_t)n_words * 4,
                                 hipMemcpyHostToDevice, stream)))
        return NMSA_ERR_LAUNCH;
    hipLaunchKernelGGL(k_batch_augment_resized, dim3((unsigned)blocks), dim3(AUGR_THREADS), 0, stream,
                       (const nmsa_augment_resize_desc*)staging_device, n_desc,
                       (const int32_t*)staging_device + table_words);
    return check_launch();
}
