// augment.hip — batch augmentation: crop, horizontal flip, normalise and HWC -> CHW of every key
// of a collated batch in ONE launch.
//
// Replaces, behind the C ABI of include/nmsa.h, the numpy steps of the reference's training chain
// that need no cv2:
//   RandomCrop._preprocess            (data/preprocessing/crop.py:57-73, the slices only)
//   RandomHorizontalFlip._preprocess  (data/preprocessing/flip.py:40-47, np.flip(axis=1))
//   NormalizeRGB / NormalizeDepth     (data/preprocessing/normalize.py:13-31, 109-122)
//   ToTorchTensors._preprocess        (data/preprocessing/torch.py:31-38, HWC -> CHW)
//
//   k_batch_augment   one descriptor per key; for sample b, output pixel (y, x):
//                       source row    y0[b] + y
//                       source column x0[b] + x             (flip[b] == 0)
//                                     x0[b] + w - 1 - x     (flip[b] == 1: crop, then flip the crop)
//                     MOVE        raw bits of 1, 2, 4 or 8 bytes, [B,H,W,C] -> [B,C,h,w]
//                     RGB_NORM    u8 [B,H,W,3] -> f32 [B,3,h,w], (float(v) - mean[c]) / std[c]
//                     DEPTH_NORM  u16 / f32 [B,H,W] -> f32 [B,1,h,w], the same, invalid values kept
//
// Lane mapping.  A lane owns `pixels_per_lane` consecutive output pixels of one output row and all
// channels of them; consecutive lanes own consecutive pixel groups, so every plane's stores are
// consecutive across the wave.  With w % 4 == 0 (the training shapes) a lane owns 4 pixels: it
// fetches the 4 * C interleaved source elements of its pixels as one contiguous span (12 bytes of
// rgb, 48 bytes of a normal; the span's alignment is the element's only, the compiler picks the
// load widths), reverses the pixels in registers when the sample is flipped, and stores one
// 16-byte (4 x f32) vector per plane, aligned because the row length is a multiple of 4.  For any
// other width a lane owns one pixel and the stores are one element per lane: rows then start at
// any alignment and there is nothing to vectorise against.  Channel counts 1 and 3 are unrolled;
// any other count walks the channels with strided element loads.
//
// The table and the per-sample parameters travel in one pinned staging buffer: the entry point
// checks every field and every sample's window on the host copy BEFORE anything is enqueued, fills
// in the block prefix and the pixels per lane, then enqueues one asynchronous copy and the launch.
// No host synchronisation; capturable in a hipGraph (the copy node re-reads the pinned buffer at
// replay: a captured call needs a staging buffer of its own, and whoever rewrites its parameter
// words between replays owns the window checks).
//
// The sibling augment_resize.hip runs the same chain behind RandomResize, or behind the upscale of
// an image smaller than the crop: it reads the source through per-sample index and weight tables
// and shares this file's lane mapping and its element operations (augment_ops.hpp).  A batch that
// needs no resize takes this file's kernel.
#include "augment_ops.hpp"

#include <string.h>

namespace nmsa {
namespace {

constexpr int AUG_THREADS = 256;
constexpr int AUG_DESC_WORDS = 24;

static_assert(sizeof(nmsa_augment_desc) == AUG_DESC_WORDS * 4, "the staging layout is 24 words per descriptor");

// S source element, D destination element, CT channels (0: read from the descriptor), NP pixels per lane
template <typename S, typename D, int CT, int NP, typename Op>
__device__ __forceinline__ void augment_group(const nmsa_augment_desc& d, const int32_t* __restrict__ params,
                                              uint32_t g, const Op& op)
{
    const uint32_t w = (uint32_t)d.w, h = (uint32_t)d.h;
    const uint32_t G = w / NP;                                    // NP == 4 only where w % 4 == 0
    const uint32_t x = (g % G) * NP;
    const uint32_t row = g / G;
    const uint32_t y = row % h, b = row / h;
    const uint32_t y0 = (uint32_t)params[3 * b], x0 = (uint32_t)params[3 * b + 1];
    const bool flip = params[3 * b + 2] != 0;
    const uint32_t s_lo = flip ? x0 + w - NP - x : x0 + x;         // lowest source column of the group
    const uint32_t C = CT ? (uint32_t)CT : (uint32_t)d.C;
    const S* src = (const S*)d.src + (((size_t)b * d.H + (y0 + y)) * d.W + s_lo) * C;
    const size_t plane = (size_t)h * w;
    D* dst = (D*)d.dst + (size_t)b * C * plane + (size_t)y * w + x;
    if constexpr (CT != 0) {
        S in[NP * CT];
        __builtin_memcpy(in, src, sizeof(in));
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            pack<D, NP> out;
#pragma unroll
            for (int j = 0; j < NP; ++j) out.v[j] = op(flip ? in[(NP - 1 - j) * CT + c] : in[j * CT + c], c);
            *(pack<D, NP>*)(dst + c * plane) = out;
        }
    } else {
        for (uint32_t c = 0; c < C; ++c) {
            pack<D, NP> out;
#pragma unroll
            for (int j = 0; j < NP; ++j) out.v[j] = op(src[(size_t)(flip ? NP - 1 - j : j) * C + c], (int)c);
            *(pack<D, NP>*)(dst + c * plane) = out;
        }
    }
}

template <typename S, typename D, int CT, typename Op>
__device__ __forceinline__ void augment_ppl(const nmsa_augment_desc& d, const int32_t* __restrict__ params,
                                            uint32_t g, const Op& op)
{
    if (d.pixels_per_lane == 4) augment_group<S, D, CT, 4>(d, params, g, op);
    else augment_group<S, D, CT, 1>(d, params, g, op);
}

template <typename T>
__device__ __forceinline__ void augment_move(const nmsa_augment_desc& d, const int32_t* __restrict__ params, uint32_t g)
{
    if (d.C == 1) augment_ppl<T, T, 1>(d, params, g, op_move{});
    else if (d.C == 3) augment_ppl<T, T, 3>(d, params, g, op_move{});
    else augment_ppl<T, T, 0>(d, params, g, op_move{});
}

__global__ __launch_bounds__(AUG_THREADS) void k_batch_augment(
    const nmsa_augment_desc* __restrict__ table, int n_desc, const int32_t* __restrict__ params)
{
    // table[i].block_begin <= blockIdx.x < table[i + 1].block_begin; the same for every lane
    int lo = 0, hi = n_desc;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((uint32_t)table[mid].block_begin <= blockIdx.x) lo = mid; else hi = mid;
    }
    const nmsa_augment_desc d = table[lo];
    // pixel groups of the descriptor: B * h * (w / pixels_per_lane) <= B * C * h * w < 2^31, checked
    const uint32_t groups = (uint32_t)d.B * (uint32_t)d.h * ((uint32_t)d.w / (uint32_t)d.pixels_per_lane);
    const uint32_t g = (blockIdx.x - (uint32_t)d.block_begin) * AUG_THREADS + threadIdx.x;
    if (g >= groups) return;
    if (d.mode == NMSA_AUGMENT_RGB_NORM) {
        augment_ppl<uint8_t, float, 3>(d, params, g, op_rgb_norm{{d.mean[0], d.mean[1], d.mean[2]},
                                                                 {d.std[0], d.std[1], d.std[2]}});
    } else if (d.mode == NMSA_AUGMENT_DEPTH_NORM) {
        const op_depth_norm op{d.mean[0], d.std[0], d.invalid_depth_value, d.raw_depth != 0};
        if (d.log2_size == 1) augment_ppl<uint16_t, float, 1>(d, params, g, op);
        else augment_ppl<float, float, 1>(d, params, g, op);
    } else {
        switch (d.log2_size) {
            case 0: augment_move<uint8_t>(d, params, g); break;
            case 1: augment_move<uint16_t>(d, params, g); break;
            case 2: augment_move<uint32_t>(d, params, g); break;
            default: augment_move<uint64_t>(d, params, g); break;
        }
    }
}

}  // namespace
}  // namespace nmsa

extern "C" int nmsa_batch_augment(void* staging_host, void* staging_device, int n_desc, int n_samples,
                                  int n_words, nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    if (!staging_host || !staging_device || n_desc <= 0 || n_desc > NMSA_AUGMENT_MAX_DESC || n_samples <= 0 ||
        (uintptr_t)staging_host % 8 != 0 || (uintptr_t)staging_device % 8 != 0)
        return NMSA_ERR_ARG;
    const int64_t table_words = (int64_t)n_desc * AUG_DESC_WORDS;
    if ((int64_t)n_words < table_words + 3 * (int64_t)n_samples) return NMSA_ERR_ARG;
    nmsa_augment_desc* table = (nmsa_augment_desc*)staging_host;
    const int32_t* params = (const int32_t*)staging_host + table_words;
    for (int b = 0; b < n_samples; ++b)
        if (params[3 * b] < 0 || params[3 * b + 1] < 0 || (params[3 * b + 2] != 0 && params[3 * b + 2] != 1))
            return NMSA_ERR_ARG;
    int64_t blocks = 0;
    for (int i = 0; i < n_desc; ++i) {
        nmsa_augment_desc& d = table[i];
        if (!d.src || !d.dst || d.B != n_samples || d.H <= 0 || d.W <= 0 || d.C <= 0 || d.h <= 0 || d.w <= 0 ||
            d.h > d.H || d.w > d.W)
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
            dst_size = 4;
        } else {
            return NMSA_ERR_ARG;
        }
        if (d.src % ((uint64_t)1 << d.log2_size) != 0 || d.dst % dst_size != 0) return NMSA_ERR_ARG;
        int64_t elements = (int64_t)d.B * d.C;
        if (elements > 0x7fffffffLL || (elements *= d.h) > 0x7fffffffLL || (elements *= d.w) > 0x7fffffffLL)
            return NMSA_ERR_ARG;
        for (int b = 0; b < n_samples; ++b)
            if ((int64_t)params[3 * b] + d.h > d.H || (int64_t)params[3 * b + 1] + d.w > d.W) return NMSA_ERR_ARG;
        const uint64_t vec_bytes = dst_size * 4 > 16 ? 16 : dst_size * 4;
        d.pixels_per_lane = (d.w % 4 == 0 && d.dst % vec_bytes == 0) ? 4 : 1;
        d.block_begin = (int32_t)blocks;
        const int64_t groups = (int64_t)d.B * d.h * (d.w / d.pixels_per_lane);
        blocks += (groups + AUG_THREADS - 1) / AUG_THREADS;
        if (blocks > 0x7fffffffLL) return NMSA_ERR_ARG;
    }
    if (check_hip(hipMemcpyAsync(staging_device, staging_host, (size_t)n_words * 4,
                                 hipMemcpyHostToDevice, stream)))
        return NMSA_ERR_LAUNCH;
    hipLaunchKernelGGL(k_batch_augment, dim3((unsigned)blocks), dim3(AUG_THREADS), 0, stream,
                       (const nmsa_augment_desc*)staging_device, n_desc,
                       (const int32_t*)staging_device + table_words);
    return check_launch();
}
