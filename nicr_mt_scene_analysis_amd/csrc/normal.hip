// normal.hip — the per-pixel work of the surface-normal task on gfx950.
//
// Replaces, behind the C ABI of include/nmsa.h,
//   _get_valid_gt_normals                     (task_helper/normal.py:165-167)
//   RootMeanSquaredError.update               (metric/rmse.py:30-57)
//   ... fed by NormalPostprocessing's crop + nearest resize to the dataset resolution
//                                             (model/postprocessing/normal.py:50-57)
//
//   k_normal_valid_mask   target [B,3,H,W] -> u8 [B,H,W]: 0 iff all three channels == 0 (by value:
//                         -0.0 is zero, a NaN channel makes the pixel valid), one pass, 12 B/px read
//   k_rmse                sum_px sqrt(mean_c (p - t)^2) and the pixel count into the metric's f64 /
//                         i64 states; the mask is absent, given, or derived from the target; the
//                         prediction is read at the target's resolution or — crop + nearest resize
//                         folded in (nearest_src of crop_resize.hpp, the arithmetic of
//                         k_resize_nearest) — at the network resolution, so the full-resolution
//                         prediction is never written
//
// Both walk groups of 4 consecutive pixels of one image (16-byte loads where H*W % 4 == 0 and the
// pointers allow it, per-pixel loads otherwise) in a grid-stride loop over a grid sized from the
// device's compute units.  Per-pixel arithmetic is float32 with IEEE-rounded subtract, multiply,
// add, divide and square root: no contraction (-ffp-contract=off), no fast-math, and the root is
// `sqrtf` and the quotient `/`, which hipcc expands to their correctly rounded sequences
// (v_sqrt_f32 / v_rcp_f32 plus fma refinement) — NOT the __fsqrt_rn / __fdiv_rn intrinsics, of
// which the first is the bare 1-ulp v_sqrt_f32 in this ROCm.  Accumulation is float64 per lane ->
// wave -> workgroup, then ONE atomic add per workgroup and state.
#include "nmsa_common.hpp"
#include "crop_resize.hpp"

namespace nmsa {
namespace {

constexpr int NRM_THREADS = 256;
constexpr int NRM_BLOCKS_PER_CU = 8;
constexpr int RMSE_MAX_C = 8;

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned short u16x4_t __attribute__((ext_vector_type(4)));

// 4 consecutive elements at p + i; VEC: one 16-byte (f32) / 8-byte (bf16, f16) load, else the
// first `n` of them one by one (the others stay 0)
template <int DTYPE, bool VEC>
__device__ __forceinline__ void ld4(const void* p, size_t i, int n, float v[4])
{
    if (DTYPE == NMSA_F32) {
        const float* s = (const float*)p + i;
        if (VEC) {
            const f32x4_t t = *(const f32x4_t*)s;
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (j < n) ? s[j] : 0.f;
        }
    } else {
        const uint16_t* s = (const uint16_t*)p + i;
        uint16_t h[4];
        if (VEC) {
            const u16x4_t t = *(const u16x4_t*)s;
            h[0] = t.x; h[1] = t.y; h[2] = t.z; h[3] = t.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) h[j] = (j < n) ? s[j] : (uint16_t)0;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (DTYPE == NMSA_BF16) ? bf16_to_f32(h[j]) : f16_to_f32(h[j]);
    }
}

// =================================================================================
// valid mask of the ground-truth normals
// =================================================================================
template <bool VEC>
__global__ __launch_bounds__(NRM_THREADS) void k_normal_valid_mask(
    const float* __restrict__ target, uint8_t* __restrict__ mask, int HW, int Q, long long units)
{
    const long long stride = (long long)gridDim.x * NRM_THREADS;
    for (long long u = (long long)blockIdx.x * NRM_THREADS + threadIdx.x; u < units; u += stride) {
        const long long b = u / Q;
        const int p = (int)(u - b * Q) * 4;
        const int n = min(4, HW - p);
        const size_t img = (size_t)b * 3 * HW + p;
        float c0[4], c1[4], c2[4];
        ld4<NMSA_F32, VEC>(target, img, n, c0);
        ld4<NMSA_F32, VEC>(target, img + HW, n, c1);
        ld4<NMSA_F32, VEC>(target, img + 2 * (size_t)HW, n, c2);
        uint8_t m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            m[j] = (c0[j] == 0.f && c1[j] == 0.f && c2[j] == 0.f) ? 0 : 1;
        uint8_t* d = mask + (size_t)b * HW + p;
        if (VEC) {
            *(uint32_t*)d = (uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16) |
                            ((uint32_t)m[3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (j < n) d[j] = m[j];
        }
    }
}

// =================================================================================
// RMSE accumulation
// =================================================================================
// MASK: NMSA_RMSE_MASK_*; RESIZED: the prediction lives at the network resolution (g.Hs x g.Ws,
// valid region g.y0/x0/h/w) and every target pixel fetches its nearest source; otherwise g.Ho x
// g.Wo is the shape of both.  VEC: 16-byte target loads (and whole-group prediction / mask loads
// when !RESIZED).
template <int DTYPE, int MASK, bool RESIZED, bool VEC>
__global__ __launch_bounds__(NRM_THREADS) void k_rmse(
    const void* __restrict__ pred, const float* __restrict__ target,
    const uint8_t* __restrict__ mask, CropResize g, int C, int Q, long long units,
    double* __restrict__ sum_state, long long* __restrict__ count_state)
{
    const int HW = g.Ho * g.Wo;
    const size_t src_plane = (size_t)g.Hs * g.Ws;
    const float fC = (float)C;
    double acc = 0.0;
    long long cnt = 0;
    const long long stride = (long long)gridDim.x * NRM_THREADS;
    for (long long u = (long long)blockIdx.x * NRM_THREADS + threadIdx.x; u < units; u += stride) {
        const long long b = u / Q;
        const int p = (int)(u - b * Q) * 4;
        const int n = min(4, HW - p);
        int soff[4];
        if (RESIZED) {
            int y = p / g.Wo, x = p - y * g.Wo;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // (pixels past the image's end repeat its last pixel: loaded, never counted)
                soff[j] = (g.y0 + nearest_src(g.sy, min(y, g.Ho - 1), g.h)) * g.Ws +
                          g.x0 + nearest_src(g.sx, x, g.w);
                if (++x == g.Wo) { x = 0; ++y; }
            }
        }
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        bool all_zero[4] = {true, true, true, true};
        for (int c = 0; c < C; ++c) {
            const size_t plane = (size_t)b * C + c;
            float t[4], q[4];
            ld4<NMSA_F32, VEC>(target, plane * HW + p, n, t);
            if (RESIZED) {
#pragma unroll
                for (int j = 0; j < 4; ++j) q[j] = ld_at<DTYPE>(pred, plane * src_plane + soff[j]);
            } else {
                ld4<DTYPE, VEC>(pred, plane * HW + p, n, q);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float d = __fsub_rn(q[j], t[j]);
                s[j] = __fadd_rn(s[j], __fmul_rn(d, d));
                if (MASK == NMSA_RMSE_MASK_FROM_TARGET) all_zero[j] = all_zero[j] && (t[j] == 0.f);
            }
        }
        uint8_t m[4] = {1, 1, 1, 1};
        if (MASK == NMSA_RMSE_MASK_GIVEN) {
            const uint8_t* mp = mask + (size_t)b * HW + p;
            if (VEC) {
                const uint32_t w = *(const uint32_t*)mp;
#pragma unroll
                for (int j = 0; j < 4; ++j) m[j] = (uint8_t)(w >> (8 * j));
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) m[j] = (j < n) ? mp[j] : (uint8_t)0;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bool use = j < n;
            if (MASK == NMSA_RMSE_MASK_GIVEN) use = use && m[j] != 0;
            if (MASK == NMSA_RMSE_MASK_FROM_TARGET) use = use && !all_zero[j];
            // a gather in the reference (rmse_per_pixel[mask]): what a masked-out pixel holds,
            // NaN included, never enters the sum
            if (use) {
                acc += (double)sqrtf(s[j] / fC);
                cnt += 1;
            }
        }
    }
    // lane -> wave -> workgroup, then one atomic per state
    acc = wave_reduce_sum(acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
    __shared__ double wave_sum[NRM_THREADS / kWave];
    __shared__ long long wave_cnt[NRM_THREADS / kWave];
    const int wv = threadIdx.x / kWave;
    if (lane_id() == 0) { wave_sum[wv] = acc; wave_cnt[wv] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double bs = 0.0;
        long long bc = 0;
#pragma unroll
        for (int i = 0; i < NRM_THREADS / kWave; ++i) { bs += wave_sum[i]; bc += wave_cnt[i]; }
        if (bc) {
            atomicAdd(sum_state, bs);
            atomicAdd((unsigned long long*)count_state, (unsigned long long)bc);
        }
    }
}

unsigned grid_blocks(long long units)
{
    long long blocks = (units + NRM_THREADS - 1) / NRM_THREADS;
    const long long cap = (long long)device_geometry().cus * NRM_BLOCKS_PER_CU;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return (unsigned)blocks;
}

template <int DTYPE, int MASK, bool RESIZED>
int launch_rmse(const void* pred, const float* target, const uint8_t* mask, const CropResize& g,
                int B, int C, double* sum_state, int64_t* count_state, hipStream_t stream)
{
    const int HW = g.Ho * g.Wo;
    const int Q = (HW + 3) / 4;
    const long long units = (long long)B * Q;
    const size_t esz = (DTYPE == NMSA_F32) ? 4 : 2;
    bool vec = HW % 4 == 0 && (uintptr_t)target % 16 == 0;
    if (!RESIZED) vec = vec && (uintptr_t)pred % (4 * esz) == 0;
    if (MASK == NMSA_RMSE_MASK_GIVEN) vec = vec && (uintptr_t)mask % 4 == 0;
    const unsigned blocks = grid_blocks(units);
#define NMSA_LAUNCH_RMSE(V)                                                                      \
    hipLaunchKernelGGL((k_rmse<DTYPE, MASK, RESIZED, V>), dim3(blocks), dim3(NRM_THREADS), 0,    \
                       stream, pred, target, mask, g, C, Q, units, sum_state,                    \
                       (long long*)count_state)
    if (vec) NMSA_LAUNCH_RMSE(true); else NMSA_LAUNCH_RMSE(false);
#undef NMSA_LAUNCH_RMSE
    return check_launch();
}

template <int DTYPE, int MASK>
int launch_rmse_source(const void* pred, const float* target, const uint8_t* mask, const CropResize& g,
                       bool resized, int B, int C, double* sum_state, int64_t* count_state,
                       hipStream_t stream)
{
    if (resized) return launch_rmse<DTYPE, MASK, true>(pred, target, mask, g, B, C, sum_state, count_state, stream);
    return launch_rmse<DTYPE, MASK, false>(pred, target, mask, g, B, C, sum_state, count_state, stream);
}

template <int DTYPE>
int launch_rmse_mask(const void* pred, const float* target, const uint8_t* mask, int mask_mode,
                     const CropResize& g, bool resized, int B, int C, double* sum_state,
                     int64_t* count_state, hipStream_t stream)
{
    switch (mask_mode) {
        case NMSA_RMSE_MASK_NONE:
            return launch_rmse_source<DTYPE, NMSA_RMSE_MASK_NONE>(pred, target, mask, g, resized, B, C, sum_state, count_state, stream);
        case NMSA_RMSE_MASK_GIVEN:
            return launch_rmse_source<DTYPE, NMSA_RMSE_MASK_GIVEN>(pred, target, mask, g, resized, B, C, sum_state, count_state, stream);
        default:
            return launch_rmse_source<DTYPE, NMSA_RMSE_MASK_FROM_TARGET>(pred, target, mask, g, resized, B, C, sum_state, count_state, stream);
    }
}

}  // namespace
}  // namespace nmsa

using namespace nmsa;

extern "C" int nmsa_normal_valid_mask(const float* target, int B, int H, int W, uint8_t* mask,
                                      nmsa_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!target || !mask || B <= 0 || H <= 0 || W <= 0 || (int64_t)H * W > ((int64_t)1 << 30))
        return NMSA_ERR_ARG;
    const int HW = H * W;
    const int Q = (HW + 3) / 4;
    const long long units = (long long)B * Q;
    const bool vec = HW % 4 == 0 && (uintptr_t)target % 16 == 0 && (uintptr_t)mask % 4 == 0;
    const unsigned blocks = grid_blocks(units);
    if (vec) hipLaunchKernelGGL(k_normal_valid_mask<true>, dim3(blocks), dim3(NRM_THREADS), 0, stream,
                                target, mask, HW, Q, units);
    else hipLaunchKernelGGL(k_normal_valid_mask<false>, dim3(blocks), dim3(NRM_THREADS), 0, stream,
                            target, mask, HW, Q, units);
    return check_launch();
}

extern "C" int nmsa_rmse_update(const void* pred, int pred_dtype, const float* target,
                                const uint8_t* mask, int mask_mode, int B, int C, int H, int W,
                                int Hs, int Ws, int y0, int x0, int h, int w,
                                double* sum_state, int64_t* count_state, nmsa_stream_t stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!pred || !target || !sum_state || !count_state || B <= 0 || C < 1 || C > RMSE_MAX_C)
        return NMSA_ERR_ARG;
    if (mask_mode != NMSA_RMSE_MASK_NONE && mask_mode != NMSA_RMSE_MASK_GIVEN &&
        mask_mode != NMSA_RMSE_MASK_FROM_TARGET)
        return NMSA_ERR_ARG;
    if ((mask_mode == NMSA_RMSE_MASK_GIVEN) != (mask != nullptr)) return NMSA_ERR_ARG;
    if (mask_mode == NMSA_RMSE_MASK_FROM_TARGET && C != 3) return NMSA_ERR_ARG;
    const bool resized = Hs != 0 || Ws != 0;
    if (!resized) { Hs = H; Ws = W; y0 = 0; x0 = 0; h = H; w = W; }
    if ((int64_t)B * C > 0x7fffffffLL || bad_geometry(B * C, Hs, Ws, y0, x0, h, w, H, W))
        return NMSA_ERR_ARG;
    const CropResize g = make_geometry(Hs, Ws, y0, x0, h, w, H, W);
    switch (pred_dtype) {
        case NMSA_F32: return launch_rmse_mask<NMSA_F32>(pred, target, mask, mask_mode, g, resized, B, C, sum_state, count_state, stream);
        case NMSA_BF16: return launch_rmse_mask<NMSA_BF16>(pred, target, mask, mask_mode, g, resized, B, C, sum_state, count_state, stream);
        case NMSA_F16: return launch_rmse_mask<NMSA_F16>(pred, target, mask, mask_mode, g, resized, B, C, sum_state, count_state, stream);
        default: return NMSA_ERR_ARG;
    }
}
