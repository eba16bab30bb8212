// scene_head.hip — the scene classification decoder (model/decoder/scene.py): global average pool, flatten and
// the linear head in ONE launch forward and ONE launch backward.  The sums and their order are those of
// include/nmsa.h (nmsa_scene_head_*); testing/scene_head_ref.py restates them on the CPU.
//
//   k_sh_fwd   one workgroup of SH_FWD_THREADS lanes per image.  Phase 1, waves own groups of P consecutive
//              channels (P = 8 on the vector route, 4 on the element route) whose loads are in flight
//              together: the lanes of a wave own the plane's chunks of V consecutive elements
//              (V = 4 for f32, 8 for the halves; chunk j belongs to lane j % 64), add their elements in ascending
//              order from 0 and combine by halves (wave_reduce_sum); pooled = S / float(H W) goes to LDS (and
//              to `pooled` when wanted).  Phase 2, after one __syncthreads, waves own classes: lanes stride
//              over c with one __fmaf_rn each, combine by halves, lane 0 adds the bias and rounds once.
//              UNIT route (H W == 1): phase 1 is a copy, no division and no reduction.  VECTOR route: a chunk is
//              one aligned 16-byte load (H W % V == 0, x on 16 bytes).  ELEMENT route: the same chunks element
//              by element, the last one short.  All routes give the same bits.
//   k_sh_bwd   three kinds of independent wave items in one grid-stride kernel, SH_BWD_WAVES items per
//              workgroup trip: planes (a wave per (b, c) plane: gs by one __fmaf_rn per k, ascending, the
//              quotient rounded once and stored over the whole plane; on the UNIT route a LANE per plane),
//              gweight (a lane per element, b ascending, __fmaf_rn), gbias (a lane per element, b ascending).
//              No atomics, no workspace, no item reads what another writes.
// Addressing: 64-bit plane base, 32-bit offsets inside a plane (H W < 2^31 is checked).
#include "nmsa_common.hpp"

namespace nmsa {
namespace {

constexpr int SH_FWD_THREADS = 1024;
constexpr int SH_BWD_THREADS = 256;
constexpr int SH_BWD_WAVES = SH_BWD_THREADS / kWave;
constexpr int SH_BLOCKS_PER_CU = 8;
constexpr int SH_UNIT = 0, SH_VECTOR = 1, SH_ELEMENT = 2;      // template codes of the routes

// elements of a chunk: one 16-byte access on the vector route
template <int DTYPE> struct sh_chunk { static constexpr int n = DTYPE == NMSA_F32 ? 4 : 8; };

// element i of a [B,K] tensor whose dtype is known at run time only (wave-uniform branch)
__device__ __forceinline__ float sh_ld_rt(const void* p, size_t i, int dtype)
{
    if (dtype == NMSA_F32) return ld_at<NMSA_F32>(p, i);
    if (dtype == NMSA_BF16) return ld_at<NMSA_BF16>(p, i);
    return ld_at<NMSA_F16>(p, i);
}
__device__ __forceinline__ void sh_st_rt(void* p, size_t i, float v, int dtype)
{
    if (dtype == NMSA_F32) st_at<NMSA_F32>(p, i, v);
    else if (dtype == NMSA_BF16) st_at<NMSA_BF16>(p, i, v);
    else st_at<NMSA_F16>(p, i, v);
}

// acc = fma(a(i), b(i), acc) for i = first, first + step, .. below n, from 0, in that order.  The loads of
// SH_BATCH terms are issued together (an index past the end re-reads the last term and is not used): the chain
// waits for memory once per batch, not once per term.
constexpr uint32_t SH_BATCH = 8;
template <typename LA, typename LB>
__device__ __forceinline__ float sh_fma_chain(uint32_t first, uint32_t step, uint32_t n, LA a, LB b)
{
    float acc = 0.0f;
    if (first >= n) return acc;
    const uint32_t last = first + (n - 1 - first) / step * step;
    for (uint32_t i0 = first; i0 < n; i0 += SH_BATCH * step) {
        float av[SH_BATCH], bv[SH_BATCH];
#pragma unroll
        for (uint32_t u = 0; u < SH_BATCH; ++u) {
            const uint32_t i = min(i0 + u * step, last);
            av[u] = a(i);
            bv[u] = b(i);
        }
#pragma unroll
        for (uint32_t u = 0; u < SH_BATCH; ++u)
            if (i0 + u * step < n) acc = __fmaf_rn(av[u], bv[u], acc);
    }
    return acc;
}

template <int DTYPE, int ROUTE>
__global__ __launch_bounds__(SH_FWD_THREADS) void k_sh_fwd(
    const typename elem<DTYPE>::type* __restrict__ x, const float* __restrict__ weight,
    const float* __restrict__ bias, float* __restrict__ pooled, void* __restrict__ logits, int dtype_out,
    uint32_t C, uint32_t HW, uint32_t K)
{
    typedef typename elem<DTYPE>::type S;
    constexpr uint32_t V = sh_chunk<DTYPE>::n;
    constexpr uint32_t n_waves = SH_FWD_THREADS / kWave;
    __shared__ float s_pool[NMSA_SCENE_HEAD_MAX_CHANNELS];
    const uint32_t b = blockIdx.x;
    const uint32_t lane = (uint32_t)lane_id(), wave = threadIdx.x / kWave;
    const S* xb = x + (size_t)b * C * HW;

    if constexpr (ROUTE == SH_UNIT) {
        for (uint32_t c = threadIdx.x; c < C; c += SH_FWD_THREADS) {
            const float p = ld<DTYPE>(xb[c]);
            s_pool[c] = p;
            if (pooled) pooled[(size_t)b * C + c] = p;
        }
    } else {
        // P planes of a wave are in flight together (their loads are independent); every plane's sum keeps its
        // own order
        constexpr uint32_t P = ROUTE == SH_VECTOR ? 8 : 4;
        const uint32_t chunks = (HW + V - 1) / V;
        const float area = (float)HW;
        for (uint32_t c0 = wave * P; c0 < C; c0 += n_waves * P) {
            const S* xp = xb + (size_t)c0 * HW;
            const uint32_t np = min(P, C - c0);
            float acc[P];
#pragma unroll
            for (uint32_t p = 0; p < P; ++p) acc[p] = 0.0f;
            for (uint32_t j = lane; j < chunks; j += kWave) {
                if constexpr (ROUTE == SH_VECTOR) {
                    pack<S, V> v[P];
#pragma unroll
                    for (uint32_t p = 0; p < P; ++p)
                        if (p < np) v[p] = *(const pack<S, V>*)(xp + (size_t)p * HW + j * V);
#pragma unroll
                    for (uint32_t p = 0; p < P; ++p)
                        if (p < np) {
#pragma unroll
                            for (uint32_t e = 0; e < V; ++e) acc[p] += ld<DTYPE>(v[p].v[e]);
                        }
                } else if (j * V + V <= HW) {
                    S v[P][V];
#pragma unroll
                    for (uint32_t p = 0; p < P; ++p)
                        if (p < np) {
#pragma unroll
                            for (uint32_t e = 0; e < V; ++e) v[p][e] = xp[(size_t)p * HW + j * V + e];
                        }
#pragma unroll
                    for (uint32_t p = 0; p < P; ++p)
                        if (p < np) {
#pragma unroll
                            for (uint32_t e = 0; e < V; ++e) acc[p] += ld<DTYPE>(v[p][e]);
                        }
                } else {                                    // the plane's last, short chunk
#pragma unroll
                    for (uint32_t p = 0; p < P; ++p)
                        if (p < np)
                            for (uint32_t e = j * V; e < HW; ++e) acc[p] += ld<DTYPE>(xp[(size_t)p * HW + e]);
                }
            }
#pragma unroll
            for (uint32_t p = 0; p < P; ++p) acc[p] = wave_reduce_sum(acc[p]);
            if (lane == 0) {
#pragma unroll
                for (uint32_t p = 0; p < P; ++p)
                    if (p < np) {
                        const float q = acc[p] / area;
                        s_pool[c0 + p] = q;
                        if (pooled) pooled[(size_t)b * C + c0 + p] = q;
                    }
            }
        }
    }
    __syncthreads();

    for (uint32_t k = wave; k < K; k += n_waves) {
        const float* wk = weight + (size_t)k * C;
        float acc = sh_fma_chain(lane, kWave, C, [&](uint32_t c) { return wk[c]; },
                                 [&](uint32_t c) { return s_pool[c]; });
        acc = wave_reduce_sum(acc);
        if (lane == 0) {
            if (bias) acc += bias[k];
            sh_st_rt(logits, (size_t)b * K + k, acc, dtype_out);
        }
    }
}

struct ShBwd {
    const void* g;          // [B,K] in dtype_g
    const float* pooled;    // [B,C]
    const float* weight;    // [K,C]
    float* gweight;         // [K,C] or NULL
    float* gbias;           // [K] or NULL
    int dtype_g;
    uint32_t B, C, HW, K;
    uint32_t n_plane;       // wave items that write gx (0: gx not wanted)
    uint32_t n_gw;          // wave items that write gweight
    uint32_t n_total;       // n_plane + n_gw + wave items that write gbias
    uint32_t items;         // ceil(n_total / SH_BWD_WAVES)
};

// gs[b,c]: k ascending, one fused multiply-add each.  A lane of its own
__device__ __forceinline__ float sh_gs(const ShBwd& a, uint32_t b, uint32_t c)
{
    return sh_fma_chain(0u, 1u, a.K, [&](uint32_t k) { return sh_ld_rt(a.g, (size_t)b * a.K + k, a.dtype_g); },
                        [&](uint32_t k) { return a.weight[(size_t)k * a.C + c]; });
}

// gs[b,c] for a whole wave (b, c wave-uniform): lane l loads the terms k0 + l of a batch of 64, the chain then
// runs over the lanes' values in ascending k; every lane holds the result
__device__ __forceinline__ float sh_gs_wave(const ShBwd& a, uint32_t b, uint32_t c, uint32_t lane)
{
    float gs = 0.0f;
    for (uint32_t k0 = 0; k0 < a.K; k0 += kWave) {
        const uint32_t k = min(k0 + lane, a.K - 1);
        const float gv = sh_ld_rt(a.g, (size_t)b * a.K + k, a.dtype_g);
        const float wv = a.weight[(size_t)k * a.C + c];
        const uint32_t n = min((uint32_t)kWave, a.K - k0);
        for (uint32_t i = 0; i < n; ++i)
            gs = __fmaf_rn(__shfl(gv, (int)i), __shfl(wv, (int)i), gs);
    }
    return gs;
}

template <int DTYPE, int ROUTE>
__global__ __launch_bounds__(SH_BWD_THREADS) void k_sh_bwd(typename elem<DTYPE>::type* __restrict__ gx,
                                                           const ShBwd a)
{
    typedef typename elem<DTYPE>::type S;
    constexpr uint32_t V = sh_chunk<DTYPE>::n;
    const uint32_t lane = (uint32_t)lane_id(), wave = threadIdx.x / kWave;
    const uint32_t planes = a.B * a.C;
    for (uint32_t item = blockIdx.x; item < a.items; item += gridDim.x) {
        uint32_t wi = item * SH_BWD_WAVES + wave;
        if (wi >= a.n_total) continue;
        if (wi < a.n_plane) {
            if constexpr (ROUTE == SH_UNIT) {
                const uint32_t p = wi * kWave + lane;
                if (p < planes) gx[p] = st<DTYPE>(sh_gs(a, p / a.C, p % a.C));
            } else {
                const S val = st<DTYPE>(sh_gs_wave(a, wi / a.C, wi % a.C, lane) / (float)a.HW);
                S* xp = gx + (size_t)wi * a.HW;
                if constexpr (ROUTE == SH_VECTOR) {
                    pack<S, V> v;
#pragma unroll
                    for (uint32_t e = 0; e < V; ++e) v.v[e] = val;
                    const uint32_t chunks = a.HW / V;
                    for (uint32_t j = lane; j < chunks; j += kWave) *(pack<S, V>*)(xp + j * V) = v;
                } else {
                    for (uint32_t e = lane; e < a.HW; e += kWave) xp[e] = val;
                }
            }
            continue;
        }
        wi -= a.n_plane;
        if (wi < a.n_gw) {
            const uint32_t i = wi * kWave + lane;           // < K C + 64
            if (i < a.K * a.C) {
                const uint32_t k = i / a.C, c = i - k * a.C;
                a.gweight[i] = sh_fma_chain(
                    0u, 1u, a.B, [&](uint32_t b) { return sh_ld_rt(a.g, (size_t)b * a.K + k, a.dtype_g); },
                    [&](uint32_t b) { return a.pooled[(size_t)b * a.C + c]; });
            }
            continue;
        }
        wi -= a.n_gw;
        const uint32_t k = wi * kWave + lane;
        if (k < a.K) {
            float acc = 0.0f;
            for (uint32_t b0 = 0; b0 < a.B; b0 += SH_BATCH) {
                float gv[SH_BATCH];
#pragma unroll
                for (uint32_t u = 0; u < SH_BATCH; ++u)
                    gv[u] = sh_ld_rt(a.g, (size_t)min(b0 + u, a.B - 1) * a.K + k, a.dtype_g);
#pragma unroll
                for (uint32_t u = 0; u < SH_BATCH; ++u)
                    if (b0 + u < a.B) acc += gv[u];
            }
            a.gbias[k] = acc;
        }
    }
}

bool sh_dtype(int d) { return d == NMSA_F32 || d == NMSA_BF16 || d == NMSA_F16; }

// sizes every entry point checks; NMSA_OK, NMSA_ERR_ARG or NMSA_ERR_UNSUPPORTED
int sh_check_sizes(int dtype_x, int dtype_out, int B, int C, int H, int W, int K)
{
    if (!sh_dtype(dtype_x) || !sh_dtype(dtype_out)) return NMSA_ERR_ARG;
    if (B < 1 || C < 1 || H < 1 || W < 1 || K < 1) return NMSA_ERR_ARG;
    if (C > NMSA_SCENE_HEAD_MAX_CHANNELS || K > NMSA_SCENE_MAX_CLASSES) return NMSA_ERR_UNSUPPORTED;
    if ((int64_t)H * W > 0x7fffffffLL) return NMSA_ERR_UNSUPPORTED;         // 32-bit offsets inside a plane
    // wave items of the backward call with every output wanted: planes, gweight, gbias
    const uint64_t n = (uint64_t)B * C + ((uint64_t)K * C + kWave - 1) / kWave + ((uint64_t)K + kWave - 1) / kWave;
    if (n > 0x7fffffffull) return NMSA_ERR_UNSUPPORTED;
    return NMSA_OK;
}

// THE route rule
int sh_route(const void* x, int dtype_x, int H, int W)
{
    const int64_t hw = (int64_t)H * W;
    if (hw == 1) return SH_UNIT;
    const int v = dtype_x == NMSA_F32 ? 4 : 8;
    return (hw % v == 0 && aligned(x, 16)) ? SH_VECTOR : SH_ELEMENT;
}

}  // namespace
}  // namespace nmsa

extern "C" int nmsa_scene_head_route(const void* x_or_gx, int dtype_x, int B, int C, int H, int W, int K)
{
    using namespace nmsa;
    const int rc = sh_check_sizes(dtype_x, NMSA_F32, B, C, H, W, K);
    if (rc != NMSA_OK) return rc;
    if (!x_or_gx || !elem_aligned(x_or_gx, dtype_x)) return NMSA_ERR_ARG;
    const int r = sh_route(x_or_gx, dtype_x, H, W);
    return r == SH_UNIT ? NMSA_SH_ROUTE_UNIT : r == SH_VECTOR ? NMSA_SH_ROUTE_VECTOR : NMSA_SH_ROUTE_ELEMENT;
}

extern "C" int nmsa_scene_head_fwd(const void* x, int dtype_x, int B, int C, int H, int W, const float* weight,
                                   const float* bias, float* pooled, void* logits, int dtype_out, int K,
                                   nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = sh_check_sizes(dtype_x, dtype_out, B, C, H, W, K);
    if (rc != NMSA_OK) return rc;
    if (!x || !weight || !logits) return NMSA_ERR_ARG;
    if (!elem_aligned(x, dtype_x) || !elem_aligned(logits, dtype_out) || !aligned(weight, 4) || !aligned(bias, 4)
        || !aligned(pooled, 4))
        return NMSA_ERR_ARG;
    const int route = sh_route(x, dtype_x, H, W);
    const dim3 grid((unsigned)B), block(SH_FWD_THREADS);
    const uint32_t HW = (uint32_t)((int64_t)H * W);
#define SH_FWD_R(DT, R)                                                                                      \
    hipLaunchKernelGGL((k_sh_fwd<DT, R>), grid, block, 0, stream, (const elem<DT>::type*)x, weight, bias,    \
                       pooled, logits, dtype_out, (uint32_t)C, HW, (uint32_t)K)
#define SH_FWD(DT)                                                                                           \
    do {                                                                                                     \
        if (route == SH_UNIT) SH_FWD_R(DT, SH_UNIT);                                                         \
        else if (route == SH_VECTOR) SH_FWD_R(DT, SH_VECTOR);                                                \
        else SH_FWD_R(DT, SH_ELEMENT);                                                                       \
    } while (0)
    NMSA_DISPATCH_DTYPE(dtype_x, SH_FWD)
#undef SH_FWD
#undef SH_FWD_R
    return check_launch();
}

extern "C" int nmsa_scene_head_bwd(const void* g, int dtype_g, const float* pooled, const float* weight, int B,
                                   int C, int H, int W, int K, void* gx, int dtype_x, float* gweight, float* gbias,
                                   nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = sh_check_sizes(dtype_x, dtype_g, B, C, H, W, K);
    if (rc != NMSA_OK) return rc;
    if (!g || !pooled || !weight) return NMSA_ERR_ARG;
    if (!elem_aligned(g, dtype_g) || !elem_aligned(gx, dtype_x) || !aligned(pooled, 4) || !aligned(weight, 4)
        || !aligned(gweight, 4) || !aligned(gbias, 4))
        return NMSA_ERR_ARG;
    if (!gx && !gweight && !gbias) return NMSA_OK;                          // nothing wanted
    const int route = sh_route(gx, dtype_x, H, W);
    ShBwd a;
    a.g = g; a.pooled = pooled; a.weight = weight; a.gweight = gweight; a.gbias = gbias; a.dtype_g = dtype_g;
    a.B = (uint32_t)B; a.C = (uint32_t)C; a.HW = (uint32_t)((int64_t)H * W); a.K = (uint32_t)K;
    const uint64_t planes = (uint64_t)B * C;
    a.n_plane = !gx ? 0u : (uint32_t)(route == SH_UNIT ? (planes + kWave - 1) / kWave : planes);
    a.n_gw = gweight ? (uint32_t)(((uint64_t)K * C + kWave - 1) / kWave) : 0u;
    a.n_total = a.n_plane + a.n_gw + (gbias ? (uint32_t)((K + kWave - 1) / kWave) : 0u);   // checked: < 2^31
    a.items = (a.n_total + SH_BWD_WAVES - 1) / SH_BWD_WAVES;
    const dim3 grid(capped_grid(a.items, SH_BLOCKS_PER_CU)), block(SH_BWD_THREADS);
#define SH_BWD_R(DT, R) hipLaunchKernelGGL((k_sh_bwd<DT, R>), grid, block, 0, stream, (elem<DT>::type*)gx, a)
#define SH_BWD(DT)                                                                                           \
    do {                                                                                                     \
        if (route == SH_UNIT) SH_BWD_R(DT, SH_UNIT);                                                         \
        else if (route == SH_VECTOR) SH_BWD_R(DT, SH_VECTOR);                                                \
        else SH_BWD_R(DT, SH_ELEMENT);                                                                       \
    } while (0)
    NMSA_DISPATCH_DTYPE(dtype_x, SH_BWD)
#undef SH_BWD
#undef SH_BWD_R
    return check_launch();
}
