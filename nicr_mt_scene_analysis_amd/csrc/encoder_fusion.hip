// encoder_fusion.hip — the RGB-D fusion after every encoder stage of a two-modality network
// (reference model/encoder_fusion.py, EncoderRGBDFusionWeightedAdd with SqueezeAndExcitation):
//
//   s_m[b,c] = mean over the plane of x_m[b,c]                                   m = rgb (0), depth (1)
//   z1_m = W1_m s_m + b1_m,  h_m = act(z1_m),  w_m = sigmoid(W2_m h_m + b2_m)    W1 [R,C], W2 [C,R], R = C / 16
//   y[b,c,p] = x_rgb[b,c,p] * w_rgb[b,c] + x_depth[b,c,p] * w_depth[b,c]
//   gx_m[b,c,p] = gy[b,c,p] * w_m[b,c] + gs_m[b,c] / (H*W)
//
// THREE launches forward (squeeze, excite, scale-add) and THREE backward (weight gradient, excite
// backward, apply), each serving both modalities; no intermediate map is written: forward 2 maps read
// for the squeeze, then 2 read + 1 written; backward 3 read, then 1 read + 2 written.  No atomics, no
// workspace, no hand-off between workgroups: every call gives the same bits.  The arithmetic contract
// (the order of every sum) is stated in include/nmsa.h and restated at the kernels.
//
// Work split.
//   k_sefuse_squeeze, k_sefuse_wgrad   a plane [H*W] is reduced by ONE wave (WAVE route, H*W <=
//       NMSA_SEFUSE_WAVE_PLANE_MAX, SEF_WAVES planes per workgroup) or by ONE workgroup of
//       SEF_BLOCK_THREADS lanes (BLOCK route).  A plane is cut into chunks of V = 4 float32 / 8 half
//       elements (16 bytes); lane t of the T = 64 / 1024 lanes of the plane owns chunks t, t + T, ...
//       VECTOR route: a chunk is one 16-byte load; ELEMENT route: the SAME lane reads the SAME chunk
//       element by element (any H*W, any element-aligned pointer; what lies behind the plane counts
//       as +0, which changes no partial sum), so both routes add in the same order.
//   k_sefuse_excite, k_sefuse_excite_bwd   one workgroup per (modality, image); the vectors live in LDS.
//   k_sefuse_scale_add, k_sefuse_apply   the tensors are flat streams of B*C*H*W elements; a lane moves
//       V elements at once (VECTOR route: H*W % V == 0, so no vector crosses a plane, and every tensor
//       on 16 bytes) or one (ELEMENT route); an item is SEF_THREADS * SEF_UNROLL such accesses.
// Grids: the map kernels launch min(items, SEF_BLOCKS_PER_CU (SEF_BLOCK_ROUTE_PER_CU for the
// 1024-lane workgroups) per compute unit of nmsa_device_geometry) workgroups and loop over the rest;
// the excite kernels launch 2 * B workgroups.  Addressing: 32-bit, B*C*H*W < 2^31 is checked.
#include "nmsa_common.hpp"
#include <math.h>

namespace nmsa {
namespace {

constexpr int SEF_THREADS = 256;
constexpr int SEF_WAVES = SEF_THREADS / kWave;       // planes of a workgroup on the WAVE route
constexpr int SEF_BLOCK_THREADS = 1024;              // lanes of a plane on the BLOCK route
constexpr int SEF_BLOCK_WAVES = SEF_BLOCK_THREADS / kWave;
constexpr int SEF_BLOCKS_PER_CU = 8;
constexpr int SEF_BLOCK_ROUTE_PER_CU = 2;
constexpr int SEF_UNROLL = 4;
constexpr int SEF_MAX_C = NMSA_SEFUSE_MAX_CHANNELS;
constexpr int SEF_MAX_R = SEF_MAX_C / 16;

// elem, ld, st, pack: nmsa_common.hpp

// the four parameter tensors of both modalities, by value in the kernel arguments
struct SefParams {
    const float* W1[2];
    const float* b1[2];
    const float* W2[2];
    const float* b2[2];
};

__device__ __forceinline__ float sef_sigmoid(float z)
{
    return __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-z)));
}

template <int ACT>
__device__ __forceinline__ float sef_act(float z)
{
    if constexpr (ACT == NMSA_SEFUSE_ACT_RELU) return z <= 0.0f ? 0.0f : z;     // a NaN passes, as torch.relu's
    else return __fmul_rn(z, sef_sigmoid(z));
}

// g * act'(z).  ReLU: ATen's threshold backward, a selection (0 at z <= 0 whatever g is, g at a NaN z);
// SiLU: g * (sig * (1 + z * (1 - sig)))
template <int ACT>
__device__ __forceinline__ float sef_act_grad(float g, float z)
{
    if constexpr (ACT == NMSA_SEFUSE_ACT_RELU) return z <= 0.0f ? 0.0f : g;
    else {
        const float sg = sef_sigmoid(z);
        return __fmul_rn(g, __fmul_rn(sg, __fadd_rn(1.0f, __fmul_rn(z, __fsub_rn(1.0f, sg)))));
    }
}

// chunk `c` (V elements from c * V) of a plane of HW elements as float32; ELEMENT route: what lies
// behind the plane is +0
template <int DTYPE, bool VECTOR>
__device__ __forceinline__ void sef_chunk(const typename elem<DTYPE>::type* __restrict__ plane, uint32_t c,
                                          uint32_t HW, float* out)
{
    typedef typename elem<DTYPE>::type S;
    constexpr int V = 16 / sizeof(S);
    if constexpr (VECTOR) {
        const pack<S, V> p = *(const pack<S, V>*)(plane + c * V);
#pragma unroll
        for (int j = 0; j < V; ++j) out[j] = ld<DTYPE>(p.v[j]);
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const uint32_t e = c * V + j;
            out[j] = e < HW ? ld<DTYPE>(plane[e]) : 0.0f;
        }
    }
}

// a lane's V partial sums pairwise (a0 + a1) + (a2 + a3) ..., then the lanes of the wave by halves
// (lane l += lane l + 32, 16, ..., 1); the sum is in lane 0
template <int V>
__device__ __forceinline__ float sef_lane_wave_sum(float* a)
{
#pragma unroll
    for (int st = 1; st < V; st *= 2)
#pragma unroll
        for (int j = 0; j < V; j += 2 * st) a[j] = __fadd_rn(a[j], a[j + st]);
    return wave_reduce_sum(a[0]);
}

// the wave sums of a BLOCK-route plane added in wave order by lane 0 of the workgroup (valid there)
__device__ __forceinline__ float sef_block_sum(float wave_sum, float* part)
{
    if (lane_id() == 0) part[threadIdx.x / kWave] = wave_sum;
    __syncthreads();
    float s = part[0];
    if (threadIdx.x == 0)
        for (int w = 1; w < SEF_BLOCK_WAVES; ++w) s = __fadd_rn(s, part[w]);
    return s;
}

// ------------------------------------------------------------------------------------ squeeze
// s[m, plane] = S / float(HW), IEEE division; S in the order described in the file header
template <int DTYPE, bool VECTOR, int PT>
__global__ __launch_bounds__(PT == kWave ? SEF_THREADS : SEF_BLOCK_THREADS) void k_sefuse_squeeze(
    const typename elem<DTYPE>::type* __restrict__ x_rgb, const typename elem<DTYPE>::type* __restrict__ x_depth,
    float* __restrict__ s, const uint32_t HW, const uint32_t planes, const uint32_t items)
{
    typedef typename elem<DTYPE>::type S;
    constexpr int V = 16 / sizeof(S);
    __shared__ float part[SEF_BLOCK_WAVES];
    const uint32_t chunks = (HW + V - 1) / V;
    for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t p2 = PT == kWave ? item * SEF_WAVES + threadIdx.x / kWave : item;     // of 2 * planes
        if (PT == kWave && p2 >= 2 * planes) continue;              // wave-uniform, no barrier on this route
        const uint32_t plane = p2 >= planes ? p2 - planes : p2;
        const S* src = (p2 >= planes ? x_depth : x_rgb) + (size_t)plane * HW;
        float a[V];
#pragma unroll
        for (int j = 0; j < V; ++j) a[j] = 0.0f;
#pragma unroll 4
        for (uint32_t c = PT == kWave ? lane_id() : threadIdx.x; c < chunks; c += PT) {
            float v[V];
            sef_chunk<DTYPE, VECTOR>(src, c, HW, v);
#pragma unroll
            for (int j = 0; j < V; ++j) a[j] = __fadd_rn(a[j], v[j]);
        }
        float sum = sef_lane_wave_sum<V>(a);
        if constexpr (PT == kWave) {
            if (lane_id() == 0) s[p2] = __fdiv_rn(sum, (float)HW);
        } else {
            sum = sef_block_sum(sum, part);
            if (threadIdx.x == 0) s[p2] = __fdiv_rn(sum, (float)HW);
            __syncthreads();                                        // `part` is written again next trip
        }
    }
}

// ------------------------------------------------------------------------------ weight gradient
// gw[m, plane] = sum over the plane of gy * x_m, fused multiply-adds from 0 in the squeeze's order;
// both modalities from one read of gy; a NULL x_m: that half of gw is not written
template <int DTYPE, bool VECTOR, int PT>
__global__ __launch_bounds__(PT == kWave ? SEF_THREADS : SEF_BLOCK_THREADS) void k_sefuse_wgrad(
    const typename elem<DTYPE>::type* __restrict__ gy, const typename elem<DTYPE>::type* __restrict__ x_rgb,
    const typename elem<DTYPE>::type* __restrict__ x_depth, float* __restrict__ gw, const uint32_t HW,
    const uint32_t planes, const uint32_t items)
{
    typedef typename elem<DTYPE>::type S;
    constexpr int V = 16 / sizeof(S);
    __shared__ float part[SEF_BLOCK_WAVES];
    const uint32_t chunks = (HW + V - 1) / V;
    for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t plane = PT == kWave ? item * SEF_WAVES + threadIdx.x / kWave : item;
        if (PT == kWave && plane >= planes) continue;
        const S* g = gy + (size_t)plane * HW;
        const S* xr = x_rgb ? x_rgb + (size_t)plane * HW : nullptr;
        const S* xd = x_depth ? x_depth + (size_t)plane * HW : nullptr;
        float ar[V], ad[V];
#pragma unroll
        for (int j = 0; j < V; ++j) ar[j] = ad[j] = 0.0f;
#pragma unroll 2
        for (uint32_t c = PT == kWave ? lane_id() : threadIdx.x; c < chunks; c += PT) {
            float vg[V], v[V];
            sef_chunk<DTYPE, VECTOR>(g, c, HW, vg);
            if (xr) {
                sef_chunk<DTYPE, VECTOR>(xr, c, HW, v);
#pragma unroll
                for (int j = 0; j < V; ++j) ar[j] = __fmaf_rn(vg[j], v[j], ar[j]);
            }
            if (xd) {
                sef_chunk<DTYPE, VECTOR>(xd, c, HW, v);
#pragma unroll
                for (int j = 0; j < V; ++j) ad[j] = __fmaf_rn(vg[j], v[j], ad[j]);
            }
        }
        float sr = sef_lane_wave_sum<V>(ar);
        float sd = sef_lane_wave_sum<V>(ad);
        if constexpr (PT == kWave) {
            if (lane_id() == 0) {
                if (xr) gw[plane] = sr;
                if (xd) gw[planes + plane] = sd;
            }
        } else {
            sr = sef_block_sum(sr, part);
            __syncthreads();
            sd = sef_block_sum(sd, part);
            if (threadIdx.x == 0) {
                if (xr) gw[plane] = sr;
                if (xd) gw[planes + plane] = sd;
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------- excite
// workgroup mb = m * B + b.  z1[r] = (sum_c W1[r,c] s[c]) + b1[r]: lane l of a wave adds c = l, l + 64, ...
// as fused multiply-adds from 0, the lanes by halves; w[c] = sigmoid((sum_r W2[c,r] h[r]) + b2[c]): fused
// multiply-adds from 0 in ascending r
template <int ACT>
__global__ __launch_bounds__(SEF_THREADS) void k_sefuse_excite(
    const float* __restrict__ s, const SefParams p, float* __restrict__ w, float* __restrict__ z1,
    const uint32_t B, const uint32_t C, const uint32_t R)
{
    __shared__ float sh_s[SEF_MAX_C];
    __shared__ float sh_h[SEF_MAX_R];
    const uint32_t mb = blockIdx.x;
    const bool depth = mb >= B;
    const float* W1 = depth ? p.W1[1] : p.W1[0];
    const float* b1 = depth ? p.b1[1] : p.b1[0];
    const float* W2 = depth ? p.W2[1] : p.W2[0];
    const float* b2 = depth ? p.b2[1] : p.b2[0];
    for (uint32_t c = threadIdx.x; c < C; c += SEF_THREADS) sh_s[c] = s[(size_t)mb * C + c];
    __syncthreads();
    for (uint32_t r = threadIdx.x / kWave; r < R; r += SEF_WAVES) {
        float acc = 0.0f;
        for (uint32_t c = lane_id(); c < C; c += kWave) acc = __fmaf_rn(W1[(size_t)r * C + c], sh_s[c], acc);
        acc = wave_reduce_sum(acc);
        if (lane_id() == 0) {
            const float z = __fadd_rn(acc, b1[r]);
            if (z1) z1[(size_t)mb * R + r] = z;
            sh_h[r] = sef_act<ACT>(z);
        }
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < C; c += SEF_THREADS) {
        float acc = 0.0f;
        for (uint32_t r = 0; r < R; ++r) acc = __fmaf_rn(W2[(size_t)c * R + r], sh_h[r], acc);
        w[(size_t)mb * C + c] = sef_sigmoid(__fadd_rn(acc, b2[c]));
    }
}

// gz2[c] = (gw[c] * w[c]) * (1 - w[c]);  gh[r] = sum_c W2[c,r] gz2[c] (lanes over c as above);
// gz1[r] = gh[r] * act'(z1[r]);  h[r] = act(z1[r]);  gs[c] = sum_r W1[r,c] gz1[r] (ascending r)
template <int ACT>
__global__ __launch_bounds__(SEF_THREADS) void k_sefuse_excite_bwd(
    const float* __restrict__ gw, const float* __restrict__ w, const float* __restrict__ z1, const SefParams p,
    float* __restrict__ gz2, float* __restrict__ gz1, float* __restrict__ gs, float* __restrict__ h,
    const uint32_t B, const uint32_t C, const uint32_t R)
{
    __shared__ float sh_g[SEF_MAX_C];
    __shared__ float sh_z[SEF_MAX_R];
    const uint32_t mb = blockIdx.x;
    const bool depth = mb >= B;
    const float* W1 = depth ? p.W1[1] : p.W1[0];
    const float* W2 = depth ? p.W2[1] : p.W2[0];
    if (!W1) return;                                   // this modality is not wanted (workgroup-uniform)
    for (uint32_t c = threadIdx.x; c < C; c += SEF_THREADS) {
        const float wc = w[(size_t)mb * C + c];
        const float g = __fmul_rn(__fmul_rn(gw[(size_t)mb * C + c], wc), __fsub_rn(1.0f, wc));
        gz2[(size_t)mb * C + c] = g;
        sh_g[c] = g;
    }
    __syncthreads();
    for (uint32_t r = threadIdx.x / kWave; r < R; r += SEF_WAVES) {
        float acc = 0.0f;
        for (uint32_t c = lane_id(); c < C; c += kWave) acc = __fmaf_rn(W2[(size_t)c * R + r], sh_g[c], acc);
        acc = wave_reduce_sum(acc);
        if (lane_id() == 0) {
            const float z = z1[(size_t)mb * R + r];
            const float g = sef_act_grad<ACT>(acc, z);
            gz1[(size_t)mb * R + r] = g;
            h[(size_t)mb * R + r] = sef_act<ACT>(z);
            sh_z[r] = g;
        }
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < C; c += SEF_THREADS) {
        float acc = 0.0f;
        for (uint32_t r = 0; r < R; ++r) acc = __fmaf_rn(W1[(size_t)r * C + c], sh_z[r], acc);
        gs[(size_t)mb * C + c] = acc;
    }
}

// ---------------------------------------------------------------------------------- scale-add
// y = round(x_rgb * w_rgb + x_depth * w_depth): two products, one sum, each rounded to float32
template <int DTYPE, int VEC>
__global__ __launch_bounds__(SEF_THREADS) void k_sefuse_scale_add(
    const typename elem<DTYPE>::type* __restrict__ x_rgb, const typename elem<DTYPE>::type* __restrict__ x_depth,
    const float* __restrict__ w, typename elem<DTYPE>::type* __restrict__ y, const uint32_t HW,
    const uint32_t planes, const uint32_t nvec, const uint32_t items)
{
    typedef pack<typename elem<DTYPE>::type, VEC> P;
    for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
#pragma unroll
        for (int u = 0; u < SEF_UNROLL; ++u) {
            const uint32_t v = (item * SEF_UNROLL + u) * SEF_THREADS + threadIdx.x;
            if (v >= nvec) continue;
            const uint32_t e = v * VEC;                              // HW % VEC == 0: one plane per access
            const uint32_t plane = e / HW;
            const float wr = w[plane], wd = w[planes + plane];
            const P a = *(const P*)(x_rgb + e), b = *(const P*)(x_depth + e);
            P r;
#pragma unroll
            for (int k = 0; k < VEC; ++k)
                r.v[k] = st<DTYPE>(__fadd_rn(__fmul_rn(ld<DTYPE>(a.v[k]), wr), __fmul_rn(ld<DTYPE>(b.v[k]), wd)));
            *(P*)(y + e) = r;
        }
    }
}

// -------------------------------------------------------------------------------------- apply
// gx_m = round(gy * w_m + gs_m / float(HW)): product, IEEE division, sum, each rounded to float32;
// a NULL gx_m is not wanted
template <int DTYPE, int VEC>
__global__ __launch_bounds__(SEF_THREADS) void k_sefuse_apply(
    const typename elem<DTYPE>::type* __restrict__ gy, const float* __restrict__ w, const float* __restrict__ gs,
    typename elem<DTYPE>::type* __restrict__ gx_rgb, typename elem<DTYPE>::type* __restrict__ gx_depth,
    const uint32_t HW, const uint32_t planes, const uint32_t nvec, const uint32_t items)
{
    typedef pack<typename elem<DTYPE>::type, VEC> P;
    const float fhw = (float)HW;
    for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
#pragma unroll
        for (int u = 0; u < SEF_UNROLL; ++u) {
            const uint32_t v = (item * SEF_UNROLL + u) * SEF_THREADS + threadIdx.x;
            if (v >= nvec) continue;
            const uint32_t e = v * VEC;
            const uint32_t plane = e / HW;
            const P g = *(const P*)(gy + e);
            float f[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) f[k] = ld<DTYPE>(g.v[k]);
            if (gx_rgb) {
                const float wm = w[plane], q = __fdiv_rn(gs[plane], fhw);
                P r;
#pragma unroll
                for (int k = 0; k < VEC; ++k) r.v[k] = st<DTYPE>(__fadd_rn(__fmul_rn(f[k], wm), q));
                *(P*)(gx_rgb + e) = r;
            }
            if (gx_depth) {
                const float wm = w[planes + plane], q = __fdiv_rn(gs[planes + plane], fhw);
                P r;
#pragma unroll
                for (int k = 0; k < VEC; ++k) r.v[k] = st<DTYPE>(__fadd_rn(__fmul_rn(f[k], wm), q));
                *(P*)(gx_depth + e) = r;
            }
        }
    }
}

// ------------------------------------------------------------------------------------ host side
bool sef_f32(const void* p) { return aligned(p, 4); }
int sef_vec(int dtype) { return dtype == NMSA_F32 ? 4 : 8; }

// sizes of a map call: NMSA_OK, NMSA_ERR_ARG or NMSA_ERR_UNSUPPORTED (to be reported after the other
// argument checks)
int sef_check_map(int dtype, int B, int C, int H, int W)
{
    if (dtype != NMSA_F32 && dtype != NMSA_BF16 && dtype != NMSA_F16) return NMSA_ERR_ARG;
    if (B < 1 || C < 16 || H < 1 || W < 1) return NMSA_ERR_ARG;
    if ((int64_t)B * C * (int64_t)H * W > 0x7fffffffLL) return NMSA_ERR_UNSUPPORTED;   // 32-bit offsets
    return NMSA_OK;
}

int sef_check_vec(int act, int B, int C)
{
    if (act != NMSA_SEFUSE_ACT_RELU && act != NMSA_SEFUSE_ACT_SILU) return NMSA_ERR_ARG;
    if (B < 1 || C < 16) return NMSA_ERR_ARG;
    if (C > SEF_MAX_C || B > 0x3fffffff) return NMSA_ERR_UNSUPPORTED;
    return NMSA_OK;
}

// THE route rule of the map kernels: 16-byte accesses need whole vectors per plane and every tensor
// of the call on 16 bytes (a NULL tensor is not part of the call)
bool sef_vector(const void* t0, const void* t1, const void* t2, int dtype, int64_t HW)
{
    return HW % sef_vec(dtype) == 0 && aligned(t0, 16) && aligned(t1, 16) && aligned(t2, 16);
}

bool sef_wave_route(int64_t HW) { return HW <= NMSA_SEFUSE_WAVE_PLANE_MAX; }

}  // namespace
}  // namespace nmsa

extern "C" int nmsa_sefuse_route(const void* t0, const void* t1, const void* t2, int dtype, int H, int W)
{
    using namespace nmsa;
    const int rc = sef_check_map(dtype, 1, 16, H, W);
    if (rc == NMSA_ERR_ARG) return rc;
    if (!t0 || !elem_aligned(t0, dtype) || !elem_aligned(t1, dtype) || !elem_aligned(t2, dtype)) return NMSA_ERR_ARG;
    if (rc != NMSA_OK) return rc;
    const int64_t HW = (int64_t)H * W;
    return (sef_vector(t0, t1, t2, dtype, HW) ? NMSA_SEFUSE_ROUTE_VECTOR : NMSA_SEFUSE_ROUTE_ELEMENT) |
           (sef_wave_route(HW) ? NMSA_SEFUSE_ROUTE_WAVE : NMSA_SEFUSE_ROUTE_BLOCK);
}

// run LAUNCH(<dtype constant>, <vector route: true / false>, <lanes of a plane>) for the route of a reduction
#define SEF_DISPATCH_REDUCE(DT, LAUNCH)                       \
    do {                                                      \
        if (vector && wave) LAUNCH(DT, true, kWave);          \
        else if (vector) LAUNCH(DT, true, SEF_BLOCK_THREADS); \
        else if (wave) LAUNCH(DT, false, kWave);              \
        else LAUNCH(DT, false, SEF_BLOCK_THREADS);            \
    } while (0)

extern "C" int nmsa_sefuse_squeeze(const void* x_rgb, const void* x_depth, int dtype, int B, int C, int H, int W,
                                   float* s, nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = sef_check_map(dtype, B, C, H, W);
    if (rc == NMSA_ERR_ARG) return rc;
    if (!x_rgb || !x_depth || !s || !elem_aligned(x_rgb, dtype) || !elem_aligned(x_depth, dtype) || !sef_f32(s))
        return NMSA_ERR_ARG;
    if (rc != NMSA_OK) return rc;
    const uint32_t HW = (uint32_t)(H * W), planes = (uint32_t)(B * C);
    const bool vector = sef_vector(x_rgb, x_depth, nullptr, dtype, HW), wave = sef_wave_route(HW);
    const uint64_t items = wave ? ((uint64_t)2 * planes + SEF_WAVES - 1) / SEF_WAVES : (uint64_t)2 * planes;
    const dim3 grid(capped_grid(items, wave ? SEF_BLOCKS_PER_CU : SEF_BLOCK_ROUTE_PER_CU));
    const dim3 block(wave ? SEF_THREADS : SEF_BLOCK_THREADS);
#define SEF_SQUEEZE_ONE(DT, VECTOR, PT)                                                                     \
    hipLaunchKernelGGL((k_sefuse_squeeze<DT, VECTOR, PT>), grid, block, 0, stream,                          \
                       (const elem<DT>::type*)x_rgb, (const elem<DT>::type*)x_depth, s, HW, planes,         \
                       (uint32_t)items)
#define SEF_SQUEEZE(DT) SEF_DISPATCH_REDUCE(DT, SEF_SQUEEZE_ONE)
    NMSA_DISPATCH_DTYPE(dtype, SEF_SQUEEZE)
#undef SEF_SQUEEZE
#undef SEF_SQUEEZE_ONE
    return check_launch();
}

extern "C" int nmsa_sefuse_weight_grad(const void* gy, const void* x_rgb, const void* x_depth, int dtype, int B,
                                       int C, int H, int W, float* gw, nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = sef_check_map(dtype, B, C, H, W);
    if (rc == NMSA_ERR_ARG) return rc;
    if (!gy || !gw || !elem_aligned(gy, dtype) || !elem_aligned(x_rgb, dtype) || !elem_aligned(x_depth, dtype) ||
        !sef_f32(gw))
        return NMSA_ERR_ARG;
    if (rc != NMSA_OK) return rc;
    if (!x_rgb && !x_depth) return NMSA_OK;
    const uint32_t HW = (uint32_t)(H * W), planes = (uint32_t)(B * C);
    const bool vector = sef_vector(gy, x_rgb, x_depth, dtype, HW), wave = sef_wave_route(HW);
    const uint64_t items = wave ? ((uint64_t)planes + SEF_WAVES - 1) / SEF_WAVES : (uint64_t)planes;
    const dim3 grid(capped_grid(items, wave ? SEF_BLOCKS_PER_CU : SEF_BLOCK_ROUTE_PER_CU));
    const dim3 block(wave ? SEF_THREADS : SEF_BLOCK_THREADS);
#define SEF_WGRAD_ONE(DT, VECTOR, PT)                                                                          \
    hipLaunchKernelGGL((k_sefuse_wgrad<DT, VECTOR, PT>), grid, block, 0, stream, (const elem<DT>::type*)gy,    \
                       (const elem<DT>::type*)x_rgb, (const elem<DT>::type*)x_depth, gw, HW, planes,           \
                       (uint32_t)items)
#define SEF_WGRAD(DT) SEF_DISPATCH_REDUCE(DT, SEF_WGRAD_ONE)
    NMSA_DISPATCH_DTYPE(dtype, SEF_WGRAD)
#undef SEF_WGRAD
#undef SEF_WGRAD_ONE
    return check_launch();
}

extern "C" int nmsa_sefuse_excite(const float* s, const float* const* params, int act, int B, int C, float* w,
                                  float* z1, nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = sef_check_vec(act, B, C);
    if (rc == NMSA_ERR_ARG) return rc;
    if (!s || !params || !w || !sef_f32(s) || !sef_f32(w) || !sef_f32(z1)) return NMSA_ERR_ARG;
    for (int i = 0; i < 8; ++i)
        if (!params[i] || !sef_f32(params[i])) return NMSA_ERR_ARG;
    if (rc != NMSA_OK) return rc;
    SefParams p;
    for (int m = 0; m < 2; ++m) {
        p.W1[m] = params[4 * m]; p.b1[m] = params[4 * m + 1];
        p.W2[m] = params[4 * m + 2]; p.b2[m] = params[4 * m + 3];
    }
    const dim3 grid(2u * (unsigned)B), block(SEF_THREADS);
    if (act == NMSA_SEFUSE_ACT_RELU)
        hipLaunchKernelGGL((k_sefuse_excite<NMSA_SEFUSE_ACT_RELU>), grid, block, 0, stream, s, p, w, z1, (uint32_t)B,
                           (uint32_t)C, (uint32_t)(C / 16));
    else
        hipLaunchKernelGGL((k_sefuse_excite<NMSA_SEFUSE_ACT_SILU>), grid, block, 0, stream, s, p, w, z1, (uint32_t)B,
                           (uint32_t)C, (uint32_t)(C / 16));
    return check_launch();
}

extern "C" int nmsa_sefuse_excite_bwd(const float* gw, const float* w, const float* z1, const float* const* weights,
                                      int act, int B, int C, float* gz2, float* gz1, float* gs, float* h,
                                      nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = sef_check_vec(act, B, C);
    if (rc == NMSA_ERR_ARG) return rc;
    if (!gw || !w || !z1 || !weights || !gz2 || !gz1 || !gs || !h) return NMSA_ERR_ARG;
    if (!sef_f32(gw) || !sef_f32(w) || !sef_f32(z1) || !sef_f32(gz2) || !sef_f32(gz1) || !sef_f32(gs) || !sef_f32(h))
        return NMSA_ERR_ARG;
    for (int i = 0; i < 4; ++i)
        if (!sef_f32(weights[i])) return NMSA_ERR_ARG;
    // a modality is wanted with both of its matrices and not wanted with neither
    if (!weights[0] != !weights[1] || !weights[2] != !weights[3]) return NMSA_ERR_ARG;
    if (rc != NMSA_OK) return rc;
    if (!weights[0] && !weights[2]) return NMSA_OK;
    SefParams p;
    for (int m = 0; m < 2; ++m) {
        p.W1[m] = weights[2 * m]; p.W2[m] = weights[2 * m + 1];
        p.b1[m] = p.b2[m] = nullptr;
    }
    const dim3 grid(2u * (unsigned)B), block(SEF_THREADS);
    if (act == NMSA_SEFUSE_ACT_RELU)
        hipLaunchKernelGGL((k_sefuse_excite_bwd<NMSA_SEFUSE_ACT_RELU>), grid, block, 0, stream, gw, w, z1, p, gz2, gz1,
                           gs, h, (uint32_t)B, (uint32_t)C, (uint32_t)(C / 16));
    else
        hipLaunchKernelGGL((k_sefuse_excite_bwd<NMSA_SEFUSE_ACT_SILU>), grid, block, 0, stream, gw, w, z1, p, gz2, gz1,
                           gs, h, (uint32_t)B, (uint32_t)C, (uint32_t)(C / 16));
    return check_launch();
}

extern "C" int nmsa_sefuse_scale_add(const void* x_rgb, const void* x_depth, int dtype, const float* w, int B, int C,
                                     int H, int W, void* y, nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = sef_check_map(dtype, B, C, H, W);
    if (rc == NMSA_ERR_ARG) return rc;
    if (!x_rgb || !x_depth || !w || !y || !elem_aligned(x_rgb, dtype) || !elem_aligned(x_depth, dtype) ||
        !elem_aligned(y, dtype) || !sef_f32(w))
        return NMSA_ERR_ARG;
    if (rc != NMSA_OK) return rc;
    const uint32_t HW = (uint32_t)(H * W), planes = (uint32_t)(B * C);
    const bool vector = sef_vector(x_rgb, x_depth, y, dtype, HW);
    const uint32_t nvec = (uint32_t)((uint64_t)planes * HW / (vector ? sef_vec(dtype) : 1));
    const uint64_t per_item = (uint64_t)SEF_THREADS * SEF_UNROLL;
    const uint64_t items = (nvec + per_item - 1) / per_item;
    const dim3 grid(capped_grid(items, SEF_BLOCKS_PER_CU)), block(SEF_THREADS);
#define SEF_SCALE_ADD(DT)                                                                                      \
    do {                                                                                                       \
        typedef elem<DT>::type S;                                                                              \
        if (vector)                                                                                            \
            hipLaunchKernelGGL((k_sefuse_scale_add<DT, 16 / sizeof(S)>), grid, block, 0, stream, (const S*)x_rgb, \
                               (const S*)x_depth, w, (S*)y, HW, planes, nvec, (uint32_t)items);                \
        else                                                                                                   \
            hipLaunchKernelGGL((k_sefuse_scale_add<DT, 1>), grid, block, 0, stream, (const S*)x_rgb,            \
                               (const S*)x_depth, w, (S*)y, HW, planes, nvec, (uint32_t)items);                \
    } while (0)
    NMSA_DISPATCH_DTYPE(dtype, SEF_SCALE_ADD)
#undef SEF_SCALE_ADD
    return check_launch();
}

extern "C" int nmsa_sefuse_apply_bwd(const void* gy, int dtype, const float* w, const float* gs, int B, int C, int H,
                                     int W, void* gx_rgb, void* gx_depth, nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = sef_check_map(dtype, B, C, H, W);
    if (rc == NMSA_ERR_ARG) return rc;
    if (!gy || !w || !gs || !elem_aligned(gy, dtype) || !elem_aligned(gx_rgb, dtype) || !elem_aligned(gx_depth, dtype) ||
        !sef_f32(w) || !sef_f32(gs))
        return NMSA_ERR_ARG;
    if (rc != NMSA_OK) return rc;
    if (!gx_rgb && !gx_depth) return NMSA_OK;
    const uint32_t HW = (uint32_t)(H * W), planes = (uint32_t)(B * C);
    const bool vector = sef_vector(gy, gx_rgb, gx_depth, dtype, HW);
    const uint32_t nvec = (uint32_t)((uint64_t)planes * HW / (vector ? sef_vec(dtype) : 1));
    const uint64_t per_item = (uint64_t)SEF_THREADS * SEF_UNROLL;
    const uint64_t items = (nvec + per_item - 1) / per_item;
    const dim3 grid(capped_grid(items, SEF_BLOCKS_PER_CU)), block(SEF_THREADS);
#define SEF_APPLY(DT)                                                                                         \
    do {                                                                                                      \
        typedef elem<DT>::type S;                                                                             \
        if (vector)                                                                                           \
            hipLaunchKernelGGL((k_sefuse_apply<DT, 16 / sizeof(S)>), grid, block, 0, stream, (const S*)gy, w, gs, \
                               (S*)gx_rgb, (S*)gx_depth, HW, planes, nvec, (uint32_t)items);                  \
        else                                                                                                  \
            hipLaunchKernelGGL((k_sefuse_apply<DT, 1>), grid, block, 0, stream, (const S*)gy, w, gs, (S*)gx_rgb, \
                               (S*)gx_depth, HW, planes, nvec, (uint32_t)items);                              \
    } while (0)
    NMSA_DISPATCH_DTYPE(dtype, SEF_APPLY)
#undef SEF_APPLY
    return check_launch();
}
