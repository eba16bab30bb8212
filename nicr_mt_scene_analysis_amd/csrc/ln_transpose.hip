// ln_transpose.hip — the Swin encoder-decoder fusion of the reference (model/encoder_decoder_fusion.py
// :123-148, names 'swin-ln-*'): LayerNorm over C of the encoder's NHWC skip tensor, NHWC -> NCHW, and
// optionally the addition of the decoder features, forward and backward, each in one launch (plus
// a small reducer backward).
//
//   y[b,c,p]  = ((x[b,p,c] - mean_bp) * rstd_bp) * gamma[c] + beta[c] (+ add[b,c,p])
//   gx[b,p,:] = rstd * (a - mean_c(a) - xh * mean_c(a * xh)),  a = gy * gamma, xh = (x - mean) * rstd
//   ggamma[c] = sum_bp gy * xh,   gbeta[c] = sum_bp gy
//
//   k_lnt_fwd    a tile is LNT_TP = 32 consecutive pixels of ONE image, all C channels.
//                Phase 1: a wave owns a row (pixel) and holds it in registers, a lane the channels
//                (k*64 + lane)*V .. +V of every slot k (V = 4 for a float32, 8 for a half x; at most
//                32 values).  A row of one slot (C <= 64V) is done 8 (float32) / 4 (half) rows at a
//                time, all loads issued before the first sum, with trees of V values.  Sum, mean,
//                sum of squared deviations (two passes over the registers, never E[x^2] - mean^2),
//                rstd; both sums are the lane's pairwise tree and then the halving tree over the
//                lanes.  mean / rstd go to LDS (and to global memory when asked for).
//                Phase 2, per chunk of LNT_CC = 128 channels: the tile's chunk is read AGAIN, right
//                after phase 1 (DESIGN.md 6g "Second read" says what is known about where that read
//                is served from), normalised and written into an LDS image [channel][pixel] of
//                float32; after a barrier the image is read along the pixels, `add` is added, and y
//                is stored in runs of 32 pixels.
//   k_lnt_bwd    the same tile and chunks.  gy's chunk goes through the same LDS image the other way
//                round (stored along the pixels, read by the x-side lane map).  Phase A builds the two
//                row sums of every pixel: lane values pairwise, the 16 lanes of a pixel by halves, one
//                partial per (pixel, 16V channels) in LDS, then a pairwise tree over those.  Phase B
//                reads the chunk again, writes gx and adds gy*xh, gy over the tile's pixels per
//                channel: two pixel quads in the lane, four lanes by halves, four waves in a fixed
//                order, then into the workgroup's own line [2][C] of the workspace.
//   k_lnt_reduce sums the lines of all workgroups per channel in a fixed order into ggamma, gbeta:
//                no float atomics anywhere, two calls give the same bits.
//
// Routes.  The vector route moves 16-byte vectors on both sides (V channels of x / gx, VY = 4 or 8
// pixels of y / gy / add); the element route has the SAME lane-to-channel map and the same trees, so
// it gives the same bits, but touches memory one element at a time with a guard per element: any C,
// any P, any element-aligned pointer.
// Lane map of the x side (phase 2, A, B): lane = cl*4 + pl, pixel quad q (4 pixels), pl the pixel in
// the quad, cl one of 16 channel groups of V channels: a pixel's 16 lanes read 16V contiguous
// channels (256 B).  A wave owns the quads 2*wave, 2*wave + 1 of the tile.
// LDS image: element (c, p) of a chunk at float index c*32 + (p ^ 4*((c/V) % 8)): rows of 32 floats
// with no padding, the 16-byte column slots of a row permuted by the channel group.  x side
// (ds_write_b32 / ds_read_b32, banks % 32, groups of 32 lanes): the 32 lanes of a half wave are 4
// pixels x 8 channel groups with 8 different slot permutations -> 32 different banks, conflict free.
// y side, vector route (ds_read_b128 / ds_write_b128, banks % 64): 8 lanes cover one row = one half
// of the 64 banks, the next row the other half; element route: 32 lanes read one row.
// The grid is min(tiles, 8 (fwd) / 4 (bwd) workgroups per compute unit of nmsa_device_geometry),
// grid-stride; B*P*C < 2^31 is checked, so every offset fits 32 bits (64-bit here all the same).
#include "nmsa_common.hpp"
#include <math.h>

namespace nmsa {
namespace {

constexpr int LNT_THREADS = 256;
constexpr int LNT_WAVES = LNT_THREADS / kWave;
constexpr int LNT_TP = 32;                          // pixels of a tile
constexpr int LNT_CC = 128;                         // channels of one LDS pass
constexpr int LNT_MAX_C = 2048;
constexpr int LNT_ROW_VALUES = LNT_MAX_C / kWave;   // values of a row a lane holds
constexpr int LNT_MAX_SLOTS = LNT_MAX_C / 64;       // row-sum partials of a pixel (16 lanes x V = 4)
constexpr int LNT_FWD_BLOCKS_PER_CU = 8;
constexpr int LNT_BWD_BLOCKS_PER_CU = 4;
constexpr int LNT_REDUCE_COLS = 32, LNT_REDUCE_PARTS = 8;

// elem, ld, st, pack: nmsa_common.hpp

// N elements from p.  Vector route: one 16-byte access (all N are there).  Element route: the
// first `valid` of them one by one, 0 for the rest.
template <int DTYPE, int N, bool VEC>
__device__ __forceinline__ void lnt_load(const typename elem<DTYPE>::type* p, float* out, uint32_t valid)
{
    typedef typename elem<DTYPE>::type S;
    if constexpr (VEC) {
        const pack<S, N> v = *(const pack<S, N>*)p;
#pragma unroll
        for (int j = 0; j < N; ++j) out[j] = ld<DTYPE>(v.v[j]);
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) out[j] = (uint32_t)j < valid ? ld<DTYPE>(p[j]) : 0.0f;
    }
}

template <int DTYPE, int N, bool VEC>
__device__ __forceinline__ void lnt_store(typename elem<DTYPE>::type* p, const float* in, uint32_t valid)
{
    typedef typename elem<DTYPE>::type S;
    if constexpr (VEC) {
        pack<S, N> v;
#pragma unroll
        for (int j = 0; j < N; ++j) v.v[j] = st<DTYPE>(in[j]);
        *(pack<S, N>*)p = v;
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j)
            if ((uint32_t)j < valid) p[j] = st<DTYPE>(in[j]);
    }
}

__host__ __device__ constexpr int lnt_vec(int dtype) { return dtype == NMSA_F32 ? 4 : 8; }

// how many of the V channels from c on exist (0 .. V)
template <int V>
__device__ __forceinline__ uint32_t lnt_valid(uint32_t c, uint32_t C)
{
    return c >= C ? 0u : min((uint32_t)V, C - c);
}

struct LntGeom {
    uint32_t P, C;
    uint32_t tiles_per_image, tiles;
    float eps;
};

// float index of element (c, p) of a chunk in the LDS image; V: channels of a lane's group
template <int V>
__device__ __forceinline__ uint32_t lnt_lds(uint32_t c, uint32_t p)
{
    return c * LNT_TP + (p ^ (((c / V) & 7u) << 2));
}

// the lane's pairwise tree over its own values (adjacent pairs first), destroys v
template <int N>
__device__ __forceinline__ float lnt_tree(float* v)
{
#pragma unroll
    for (int w = 1; w < N; w <<= 1)
#pragma unroll
        for (int i = 0; i < N; i += 2 * w) v[i] += v[i + w];
    return v[0];
}

// all 64 lanes by halves; every lane gets the sum
__device__ __forceinline__ float lnt_wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// y side, global -> LDS image (vector route: runs of VY pixels, element route: single elements)
template <int DY, int V, int VY, bool VEC>
__device__ __forceinline__ void lnt_image_from_global(const typename elem<DY>::type* src, float* tile,
                                                      uint32_t b, uint32_t p0, uint32_t np, uint32_t c0,
                                                      const LntGeom& g)
{
    constexpr int RPR = LNT_TP / VY;
    for (uint32_t r = threadIdx.x; r < (uint32_t)(LNT_CC * RPR); r += LNT_THREADS) {
        const uint32_t cloc = r / RPR, pr = (r % RPR) * VY, c = c0 + cloc;
        if (c >= g.C || pr >= np) continue;
        float v[VY];
        lnt_load<DY, VY, VEC>(src + ((size_t)b * g.C + c) * g.P + p0 + pr, v, VY);
        if constexpr (VY > 1) {
#pragma unroll
            for (int h = 0; h < VY; h += 4) {
                f32x4_s q = {v[h], v[h + 1], v[h + 2], v[h + 3]};
                *(f32x4_s*)&tile[lnt_lds<V>(cloc, pr + h)] = q;
            }
        } else {
            tile[lnt_lds<V>(cloc, pr)] = v[0];
        }
    }
}

// Phase 1 of the forward kernel: mean and rstd of the wave's rows (wave, wave + 4, ... of the tile).
// S: slots of a row a lane holds, S*V values; R = 32 / (S*V) rows are loaded together, so a short row
// (C <= 64V: one slot) has 8 (float32) / 4 (half) rows in flight per wave and a tree of V values only.
template <int DX, bool VEC, int S>
__device__ __forceinline__ void lnt_stats(const typename elem<DX>::type* xt, size_t row0, uint32_t np,
                                          uint32_t wave, uint32_t lane, const LntGeom& g, float* s_mean,
                                          float* s_rstd, float* __restrict__ mean_out, float* __restrict__ rstd_out)
{
    constexpr int V = lnt_vec(DX);
    static_assert(S * V <= LNT_ROW_VALUES, "a lane holds at most LNT_ROW_VALUES values of a row");
    constexpr int N = S * V, R = LNT_ROW_VALUES / N;
    const float fC = (float)g.C;
    for (uint32_t i0 = 0; i0 < (uint32_t)(LNT_TP / LNT_WAVES); i0 += R) {
        if (wave + LNT_WAVES * i0 >= np) break;
        float v[R][N], d[R][N], mean[R];
        // the lane number behind an empty asm, once per pass: otherwise the `c < C` masks of all
        // slots are hoisted out of the row loop and held in scalar register pairs across the trees
        uint32_t l1 = lane, l2 = lane;
        asm volatile("" : "+v"(l1));
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const uint32_t r = wave + LNT_WAVES * (i0 + q);
#pragma unroll
            for (int k = 0; k < S; ++k) {
                const uint32_t c = ((uint32_t)k * kWave + l1) * V;
                const uint32_t valid = r < np ? lnt_valid<V>(c, g.C) : 0u;
                if constexpr (VEC) {
                    // no branch: an absent group loads the tile's first vector and is zeroed
                    lnt_load<DX, V, VEC>(valid ? xt + (size_t)r * g.C + c : xt, v[q] + k * V, V);
#pragma unroll
                    for (int j = 0; j < V; ++j) v[q][k * V + j] = valid ? v[q][k * V + j] : 0.0f;
                } else {
                    lnt_load<DX, V, VEC>(xt + (size_t)r * g.C + c, v[q] + k * V, valid);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < R; ++q) {
#pragma unroll
            for (int i = 0; i < N; ++i) d[q][i] = v[q][i];
            mean[q] = lnt_wave_sum(lnt_tree<N>(d[q])) / fC;
        }
        asm volatile("" : "+v"(l2));
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const uint32_t r = wave + LNT_WAVES * (i0 + q);
#pragma unroll
            for (int k = 0; k < S; ++k) {
                const uint32_t valid = lnt_valid<V>(((uint32_t)k * kWave + l2) * V, g.C);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float e = v[q][k * V + j] - mean[q];
                    d[q][k * V + j] = (uint32_t)j < valid ? e * e : 0.0f;
                }
            }
            const float var = lnt_wave_sum(lnt_tree<N>(d[q])) / fC;
            const float rstd = 1.0f / sqrtf(var + g.eps);
            if (lane == 0 && r < np) {
                s_mean[r] = mean[q];
                s_rstd[r] = rstd;
                if (mean_out) {
                    mean_out[row0 + r] = mean[q];
                    rstd_out[row0 + r] = rstd;
                }
            }
        }
    }
}

template <int DX, int DY, bool VEC>
__global__ __launch_bounds__(LNT_THREADS) void k_lnt_fwd(
    const typename elem<DX>::type* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ beta, const typename elem<DY>::type* __restrict__ add,
    typename elem<DY>::type* __restrict__ y, float* __restrict__ mean_out, float* __restrict__ rstd_out,
    const LntGeom g)
{
    typedef typename elem<DX>::type SX;
    constexpr int V = lnt_vec(DX), VY = VEC ? lnt_vec(DY) : 1;
    constexpr int NCB = LNT_CC / (16 * V), RPR = LNT_TP / VY;
    __shared__ __attribute__((aligned(16))) float tile[LNT_CC * LNT_TP];
    __shared__ float s_mean[LNT_TP], s_rstd[LNT_TP];
    const uint32_t lane = (uint32_t)lane_id(), wave = threadIdx.x / kWave;
    const uint32_t pl = lane & 3u, cl = lane >> 2;
    for (uint32_t t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        const uint32_t b = t / g.tiles_per_image, p0 = (t - b * g.tiles_per_image) * LNT_TP;
        const uint32_t np = min((uint32_t)LNT_TP, g.P - p0);
        const size_t row0 = (size_t)b * g.P + p0;
        const SX* xt = x + row0 * g.C;
        // phase 1: the statistics of the tile's rows: short rows (one slot) several at a time
        if (g.C <= 1u * kWave * V)
            lnt_stats<DX, VEC, 1>(xt, row0, np, wave, lane, g, s_mean, s_rstd, mean_out, rstd_out);
        else
            lnt_stats<DX, VEC, LNT_ROW_VALUES / V>(xt, row0, np, wave, lane, g, s_mean, s_rstd, mean_out,
                                                   rstd_out);
        __syncthreads();
        // phase 2: normalise, transpose through the LDS image, add, store
        for (uint32_t c0 = 0; c0 < g.C; c0 += LNT_CC) {
#pragma unroll
            for (int qi = 0; qi < 2; ++qi) {
                const uint32_t p = (wave * 2 + qi) * 4 + pl;
                if (p >= np) continue;
                const float mean = s_mean[p], rstd = s_rstd[p];
                const SX* row = xt + (size_t)p * g.C;
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) {
                    const uint32_t cloc = ((uint32_t)cb * 16 + cl) * V, c = c0 + cloc;
                    const uint32_t valid = lnt_valid<V>(c, g.C);
                    if (!valid) continue;
                    float xv[V];
                    lnt_load<DX, V, VEC>(row + c, xv, valid);
#pragma unroll
                    for (int j = 0; j < V; ++j)
                        if ((uint32_t)j < valid)
                            tile[lnt_lds<V>(cloc + j, p)] = ((xv[j] - mean) * rstd) * gamma[c + j] + beta[c + j];
                }
            }
            __syncthreads();
            for (uint32_t r = threadIdx.x; r < (uint32_t)(LNT_CC * RPR); r += LNT_THREADS) {
                const uint32_t cloc = r / RPR, pr = (r % RPR) * VY, c = c0 + cloc;
                if (c >= g.C || pr >= np) continue;
                float o[VY];
                if constexpr (VY > 1) {
#pragma unroll
                    for (int h = 0; h < VY; h += 4) {
                        const f32x4_s q = *(const f32x4_s*)&tile[lnt_lds<V>(cloc, pr + h)];
                        o[h] = q.x; o[h + 1] = q.y; o[h + 2] = q.z; o[h + 3] = q.w;
                    }
                } else {
                    o[0] = tile[lnt_lds<V>(cloc, pr)];
                }
                const size_t off = ((size_t)b * g.C + c) * g.P + p0 + pr;
                if (add) {
                    float a[VY];
                    lnt_load<DY, VY, VEC>(add + off, a, VY);
#pragma unroll
                    for (int j = 0; j < VY; ++j) o[j] += a[j];
                }
                lnt_store<DY, VY, VEC>(y + off, o, VY);
            }
            __syncthreads();
        }
    }
}

template <int DX, int DY, bool VEC>
__global__ __launch_bounds__(LNT_THREADS) void k_lnt_bwd(
    const typename elem<DY>::type* __restrict__ gy, const typename elem<DX>::type* __restrict__ x,
    const float* __restrict__ gamma, const float* __restrict__ mean, const float* __restrict__ rstd,
    typename elem<DX>::type* __restrict__ gx, float* __restrict__ partials, const LntGeom g)
{
    typedef typename elem<DX>::type SX;
    constexpr int V = lnt_vec(DX), VY = VEC ? lnt_vec(DY) : 1;
    constexpr int NCB = LNT_CC / (16 * V);
    constexpr int TREE = LNT_MAX_SLOTS / 8;         // partials of a pixel per tree lane
    __shared__ __attribute__((aligned(16))) float tile[LNT_CC * LNT_TP];
    __shared__ float part[2][LNT_TP][LNT_MAX_SLOTS];
    __shared__ float col[LNT_WAVES][2][LNT_CC];
    __shared__ float s_mean[LNT_TP], s_rstd[LNT_TP], s_a1[LNT_TP], s_a2[LNT_TP];
    const uint32_t lane = (uint32_t)lane_id(), wave = threadIdx.x / kWave;
    const uint32_t pl = lane & 3u, cl = lane >> 2;
    const float fC = (float)g.C;
    const uint32_t slots = (g.C + LNT_CC - 1) / LNT_CC * NCB;        // written per pixel in phase A
    bool first = true;
    for (uint32_t t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        const uint32_t b = t / g.tiles_per_image, p0 = (t - b * g.tiles_per_image) * LNT_TP;
        const uint32_t np = min((uint32_t)LNT_TP, g.P - p0);
        const size_t row0 = (size_t)b * g.P + p0;
        const SX* xt = x + row0 * g.C;
        if (threadIdx.x < np) {
            s_mean[threadIdx.x] = mean[row0 + threadIdx.x];
            s_rstd[threadIdx.x] = rstd[row0 + threadIdx.x];
        }
        if (gx) {
            // phase A: mean_c(a) and mean_c(a * xh) of every pixel of the tile
            for (uint32_t c0 = 0; c0 < g.C; c0 += LNT_CC) {
                lnt_image_from_global<DY, V, VY, VEC>(gy, tile, b, p0, np, c0, g);
                __syncthreads();
#pragma unroll
                for (int qi = 0; qi < 2; ++qi) {
                    const uint32_t p = (wave * 2 + qi) * 4 + pl;
                    const bool row_in = p < np;
                    const float mu = row_in ? s_mean[p] : 0.0f, rs = row_in ? s_rstd[p] : 0.0f;
#pragma unroll
                    for (int cb = 0; cb < NCB; ++cb) {
                        const uint32_t cloc = ((uint32_t)cb * 16 + cl) * V, c = c0 + cloc;
                        const uint32_t valid = row_in ? lnt_valid<V>(c, g.C) : 0u;
                        float s1[V], s2[V];
#pragma unroll
                        for (int j = 0; j < V; ++j) s1[j] = s2[j] = 0.0f;
                        if (valid) {
                            float xv[V];
                            lnt_load<DX, V, VEC>(xt + (size_t)p * g.C + c, xv, valid);
#pragma unroll
                            for (int j = 0; j < V; ++j) {
                                if ((uint32_t)j < valid) {
                                    const float a = tile[lnt_lds<V>(cloc + j, p)] * gamma[c + j];
                                    s1[j] = a;
                                    s2[j] = a * ((xv[j] - mu) * rs);
                                }
                            }
                        }
                        float a1 = lnt_tree<V>(s1), a2 = lnt_tree<V>(s2);
#pragma unroll
                        for (int o = 4; o < kWave; o <<= 1) {       // the pixel's 16 lanes, by halves
                            a1 += __shfl_xor(a1, o);
                            a2 += __shfl_xor(a2, o);
                        }
                        if (cl == 0 && row_in) {
                            const uint32_t slot = c0 / LNT_CC * NCB + cb;
                            part[0][p][slot] = a1;
                            part[1][p][slot] = a2;
                        }
                    }
                }
                __syncthreads();
            }
            {   // 8 lanes per pixel: TREE partials pairwise in the lane, then the lanes by halves
                const uint32_t p = threadIdx.x >> 3, sub = threadIdx.x & 7u;
                float u1[TREE], u2[TREE];
#pragma unroll
                for (int i = 0; i < TREE; ++i) {
                    const uint32_t slot = sub * TREE + i;
                    const bool in = p < np && slot < slots;
                    u1[i] = in ? part[0][p][slot] : 0.0f;
                    u2[i] = in ? part[1][p][slot] : 0.0f;
                }
                float a1 = lnt_tree<TREE>(u1), a2 = lnt_tree<TREE>(u2);
#pragma unroll
                for (int o = 1; o < 8; o <<= 1) {
                    a1 += __shfl_xor(a1, o);
                    a2 += __shfl_xor(a2, o);
                }
                if (sub == 0) {
                    s_a1[p] = a1 / fC;
                    s_a2[p] = a2 / fC;
                }
            }
        }
        // phase B: gx and the per-channel sums of the tile
        for (uint32_t c0 = 0; c0 < g.C; c0 += LNT_CC) {
            lnt_image_from_global<DY, V, VY, VEC>(gy, tile, b, p0, np, c0, g);
            __syncthreads();
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                const uint32_t cloc = ((uint32_t)cb * 16 + cl) * V, c = c0 + cloc;
                const uint32_t valid = lnt_valid<V>(c, g.C);
                float sg[V], sb[V];
#pragma unroll
                for (int j = 0; j < V; ++j) sg[j] = sb[j] = 0.0f;
#pragma unroll
                for (int qi = 0; qi < 2; ++qi) {
                    const uint32_t p = (wave * 2 + qi) * 4 + pl;
                    if (p < np && valid) {
                        const float mu = s_mean[p], rs = s_rstd[p];
                        const float A1 = gx ? s_a1[p] : 0.0f, A2 = gx ? s_a2[p] : 0.0f;
                        float xv[V], out[V];
                        lnt_load<DX, V, VEC>(xt + (size_t)p * g.C + c, xv, valid);
#pragma unroll
                        for (int j = 0; j < V; ++j) {
                            out[j] = 0.0f;
                            if ((uint32_t)j < valid) {
                                const float gyv = tile[lnt_lds<V>(cloc + j, p)];
                                const float xh = (xv[j] - mu) * rs;
                                const float a = gyv * gamma[c + j];
                                out[j] = rs * ((a - A1) - xh * A2);
                                sg[j] += gyv * xh;
                                sb[j] += gyv;
                            }
                        }
                        if (gx) lnt_store<DX, V, VEC>(gx + (row0 + p) * g.C + c, out, valid);
                    }
                }
                if (partials) {                     // the same for every lane of the grid
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        sg[j] += __shfl_xor(sg[j], 1);
                        sb[j] += __shfl_xor(sb[j], 1);
                        sg[j] += __shfl_xor(sg[j], 2);
                        sb[j] += __shfl_xor(sb[j], 2);
                    }
                    if (pl == 0) {
#pragma unroll
                        for (int j = 0; j < V; ++j) {
                            col[wave][0][cloc + j] = sg[j];
                            col[wave][1][cloc + j] = sb[j];
                        }
                    }
                }
            }
            __syncthreads();
            if (partials) {
                const uint32_t s = threadIdx.x / LNT_CC, cloc = threadIdx.x % LNT_CC, c = c0 + cloc;
                if (c < g.C) {
                    const float v = (col[0][s][cloc] + col[1][s][cloc]) + (col[2][s][cloc] + col[3][s][cloc]);
                    float* dst = partials + ((size_t)blockIdx.x * 2 + s) * g.C + c;
                    *dst = first ? v : *dst + v;
                }
            }
        }
        first = false;
        __syncthreads();
    }
}

// ggamma[c], gbeta[c]: the lines of the workgroups in ascending order, LNT_REDUCE_PARTS interleaved
// running sums per channel, then those pairwise
__global__ __launch_bounds__(LNT_REDUCE_COLS * LNT_REDUCE_PARTS) void k_lnt_reduce(
    const float* __restrict__ partials, uint32_t nwg, uint32_t C, float* __restrict__ ggamma,
    float* __restrict__ gbeta)
{
    __shared__ float red[LNT_REDUCE_PARTS][LNT_REDUCE_COLS];
    const uint32_t k = threadIdx.x / LNT_REDUCE_COLS, i = threadIdx.x % LNT_REDUCE_COLS;
    const uint32_t e = blockIdx.x * LNT_REDUCE_COLS + i;            // s * C + c
    float acc = 0.0f;
    if (e < 2 * C)
        for (uint32_t w = k; w < nwg; w += LNT_REDUCE_PARTS) acc += partials[(size_t)w * 2 * C + e];
    red[k][i] = acc;
    __syncthreads();
    if (k == 0 && e < 2 * C) {
        const float v = ((red[0][i] + red[1][i]) + (red[2][i] + red[3][i])) +
                        ((red[4][i] + red[5][i]) + (red[6][i] + red[7][i]));
        if (e < C) {
            if (ggamma) ggamma[e] = v;
        } else if (gbeta) {
            gbeta[e - C] = v;
        }
    }
}

bool lnt_is_dtype(int dtype) { return dtype == NMSA_F32 || dtype == NMSA_BF16 || dtype == NMSA_F16; }

// dtypes and sizes every entry point checks; NMSA_OK, NMSA_ERR_ARG or NMSA_ERR_UNSUPPORTED
int lnt_check_sizes(int dtype_x, int dtype_y, int B, int P, int C)
{
    if (!lnt_is_dtype(dtype_x) || (dtype_y != dtype_x && dtype_y != NMSA_F32)) return NMSA_ERR_ARG;
    if (B < 1 || P < 1 || C < 1) return NMSA_ERR_ARG;
    // B * P first: B * P * C could leave int64 for B and P near 2^31
    if (C > LNT_MAX_C || (int64_t)B * P > 0x7fffffffLL / C) return NMSA_ERR_UNSUPPORTED;
    return NMSA_OK;
}

// THE route rule: the vector route needs whole 16-byte vectors along C (x side) and along P (y side)
// and every tensor of the call on 16 bytes (a NULL pointer is no tensor of the call)
bool lnt_vector(int dtype_x, int dtype_y, int P, int C, const void* a, const void* b, const void* c)
{
    return C % lnt_vec(dtype_x) == 0 && P % lnt_vec(dtype_y) == 0 && aligned(a, 16) && aligned(b, 16) &&
           aligned(c, 16);
}

LntGeom lnt_geometry(int B, int P, int C, float eps)
{
    LntGeom g;
    g.P = (uint32_t)P; g.C = (uint32_t)C; g.eps = eps;
    g.tiles_per_image = (uint32_t)((P + LNT_TP - 1) / LNT_TP);
    g.tiles = (uint32_t)B * g.tiles_per_image;                      // <= B * P < 2^31
    return g;
}

}  // namespace
}  // namespace nmsa

// CALL(DX, DY) for the five legal dtype pairs (checked before)
#define LNT_DISPATCH(dx, dy, CALL)                                          \
    do {                                                                    \
        if ((dx) == NMSA_F32) { CALL(NMSA_F32, NMSA_F32); }                 \
        else if ((dx) == NMSA_BF16 && (dy) == NMSA_F32) { CALL(NMSA_BF16, NMSA_F32); }   \
        else if ((dx) == NMSA_BF16) { CALL(NMSA_BF16, NMSA_BF16); }         \
        else if ((dy) == NMSA_F32) { CALL(NMSA_F16, NMSA_F32); }            \
        else { CALL(NMSA_F16, NMSA_F16); }                                  \
    } while (0)

extern "C" int nmsa_ln_nhwc_nchw_route(const void* x, const void* y, int dtype_x, int dtype_y,
                                       int B, int P, int C)
{
    using namespace nmsa;
    const int rc = lnt_check_sizes(dtype_x, dtype_y, B, P, C);
    if (rc != NMSA_OK) return rc;
    if (!x || !y || !aligned(x, (uintptr_t)elem_bytes(dtype_x)) ||
        !aligned(y, (uintptr_t)elem_bytes(dtype_y)))
        return NMSA_ERR_ARG;
    return lnt_vector(dtype_x, dtype_y, P, C, x, y, nullptr) ? NMSA_LNT_ROUTE_VECTOR : NMSA_LNT_ROUTE_ELEMENT;
}

extern "C" int nmsa_ln_nhwc_nchw_fwd(const void* x, int dtype_x, const float* gamma, const float* beta,
                                     float eps, const void* add, int B, int P, int C, void* y, int dtype_y,
                                     float* mean, float* rstd, nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = lnt_check_sizes(dtype_x, dtype_y, B, P, C);
    if (rc != NMSA_OK) return rc;
    const uintptr_t ex = (uintptr_t)elem_bytes(dtype_x), ey = (uintptr_t)elem_bytes(dtype_y);
    if (!x || !y || !gamma || !beta || (mean == nullptr) != (rstd == nullptr)) return NMSA_ERR_ARG;
    if (!(eps >= 0.0f) || isinf(eps)) return NMSA_ERR_ARG;
    if (!aligned(x, ex) || !aligned(y, ey) || !aligned(add, ey) || !aligned(gamma, 4) ||
        !aligned(beta, 4) || !aligned(mean, 4) || !aligned(rstd, 4))
        return NMSA_ERR_ARG;
    const bool vec = lnt_vector(dtype_x, dtype_y, P, C, x, y, add);
    const LntGeom g = lnt_geometry(B, P, C, eps);
    const dim3 grid(capped_grid(g.tiles, LNT_FWD_BLOCKS_PER_CU)), block(LNT_THREADS);
#define LNT_FWD(DX, DY)                                                                                     \
    do {                                                                                                    \
        typedef elem<DX>::type SX;                                                                          \
        typedef elem<DY>::type SY;                                                                          \
        if (vec) hipLaunchKernelGGL((k_lnt_fwd<DX, DY, true>), grid, block, 0, stream, (const SX*)x, gamma, \
                                    beta, (const SY*)add, (SY*)y, mean, rstd, g);                           \
        else hipLaunchKernelGGL((k_lnt_fwd<DX, DY, false>), grid, block, 0, stream, (const SX*)x, gamma,    \
                                beta, (const SY*)add, (SY*)y, mean, rstd, g);                               \
    } while (0)
    LNT_DISPATCH(dtype_x, dtype_y, LNT_FWD);
#undef LNT_FWD
    return check_launch();
}

extern "C" size_t nmsa_ln_nhwc_nchw_bwd_workspace_bytes(int B, int P, int C)
{
    using namespace nmsa;
    if (lnt_check_sizes(NMSA_F32, NMSA_F32, B, P, C) != NMSA_OK) return 0;
    const LntGeom g = lnt_geometry(B, P, C, 0.0f);
    return (size_t)capped_grid(g.tiles, LNT_BWD_BLOCKS_PER_CU) * 2 * (size_t)C * sizeof(float);
}

extern "C" int nmsa_ln_nhwc_nchw_bwd(const void* gy, int dtype_y, const void* x, int dtype_x,
                                     const float* gamma, const float* mean, const float* rstd,
                                     int B, int P, int C, void* gx, float* ggamma, float* gbeta,
                                     void* workspace, size_t workspace_bytes, nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = lnt_check_sizes(dtype_x, dtype_y, B, P, C);
    if (rc != NMSA_OK) return rc;
    const uintptr_t ex = (uintptr_t)elem_bytes(dtype_x), ey = (uintptr_t)elem_bytes(dtype_y);
    if (!gy || !x || !gamma || !mean || !rstd) return NMSA_ERR_ARG;
    if (!aligned(gy, ey) || !aligned(x, ex) || !aligned(gx, ex) || !aligned(gamma, 4) ||
        !aligned(mean, 4) || !aligned(rstd, 4) || !aligned(ggamma, 4) || !aligned(gbeta, 4))
        return NMSA_ERR_ARG;
    const bool reduce = ggamma || gbeta;
    const LntGeom g = lnt_geometry(B, P, C, 0.0f);
    const unsigned nwg = capped_grid(g.tiles, LNT_BWD_BLOCKS_PER_CU);
    if (reduce) {
        if (!workspace || !aligned(workspace, 16)) return NMSA_ERR_ARG;
        if (workspace_bytes < (size_t)nwg * 2 * (size_t)C * sizeof(float)) return NMSA_ERR_WORKSPACE;
    }
    if (!gx && !reduce) return NMSA_OK;
    const bool vec = lnt_vector(dtype_x, dtype_y, P, C, gy, x, gx);
    float* partials = reduce ? (float*)workspace : nullptr;
    const dim3 grid(nwg), block(LNT_THREADS);
#define LNT_BWD(DX, DY)                                                                                     \
    do {                                                                                                    \
        typedef elem<DX>::type SX;                                                                          \
        typedef elem<DY>::type SY;                                                                          \
        if (vec) hipLaunchKernelGGL((k_lnt_bwd<DX, DY, true>), grid, block, 0, stream, (const SY*)gy,       \
                                    (const SX*)x, gamma, mean, rstd, (SX*)gx, partials, g);                 \
        else hipLaunchKernelGGL((k_lnt_bwd<DX, DY, false>), grid, block, 0, stream, (const SY*)gy,          \
                                (const SX*)x, gamma, mean, rstd, (SX*)gx, partials, g);                     \
    } while (0)
    LNT_DISPATCH(dtype_x, dtype_y, LNT_BWD);
#undef LNT_BWD
    if (int l = check_launch()) return l;
    if (reduce) {
        const unsigned blocks = (unsigned)((2 * C + LNT_REDUCE_COLS - 1) / LNT_REDUCE_COLS);
        hipLaunchKernelGGL(k_lnt_reduce, dim3(blocks), dim3(LNT_REDUCE_COLS * LNT_REDUCE_PARTS), 0, stream,
                           (const float*)partials, (uint32_t)nwg, (uint32_t)C, ggamma, gbeta);
        return check_launch();
    }
    return NMSA_OK;
}
