// dve_project.hip — DenseVisualEmbeddingPostprocessing, steps 1 + 2 of the reference
// (model/postprocessing/dense_visual_embedding.py:126 and :81): L2-normalise every pixel's
// D-vector in place and project the normalised vector onto up to two sets of class embeddings.
//
// The reference runs norm, div_ and one conv2d per head (>= 16 D bytes per pixel before the
// first logit).  Here ONE pass over the embedding map accumulates the sum of squares and the raw
// dot products together; the logits are scaled by 1/norm afterwards and the map is read once more
// only for the in-place write-back (12 D bytes per pixel + the logits).
//
// Tuned kernel (D % 4 == 0, H*W % 4 == 0, C <= 256 per head): the dot products are a
// [classes x D] x [D x pixels] product on v_mfma_f32_16x16x4_f32 (f32 operands and accumulation,
// bitwise an fmaf chain).  One wave owns 16*PT consecutive pixels of one image and NT tiles of 16
// classes, all accumulators in registers; no LDS.  Lane (r = lane & 15, kk = lane >> 4):
//   A operand  w[class 16 t + r][d0 + 4 kk + j]            one float4 per 16 channels and tile
//   B operand  x[d0 + 4 kk + j][p0 + 64 v + 4 r + c]       float4 over c: four pixel tiles
//   result     acc[t][4 v + c][i] = dot(class 16 t + 4 kk + i, pixel p0 + 64 v + 4 r + c)
// so a float4 over c is four consecutive pixels of one class row: 256 contiguous bytes per 16
// lanes on both the loads and the logit stores.  More class tiles than NT: further passes over the
// same pixels (the in-place write comes after the last one).
//
// Everything else (any D >= 1, any C >= 1, odd H*W, unaligned pointers) takes k_dve_generic: one
// lane per pixel, plain fmaf.  Both routes compute dot(x, w) * (1 / sqrt(sum x^2)) and
// x * (1 / sqrt(sum x^2)): a zero vector gives NaN everywhere (0 * inf), inf / NaN propagate.
// (The factor form needs the sum of squares to be a normal float32: see include/nmsa.h.)
// Which kernel runs is decided by dve_route alone; nmsa_dve_project_route exports its answer.
#include "nmsa_common.hpp"

namespace nmsa {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct DveHeads {
    const float* w[2];   // [C, D] or nullptr
    float* out[2];       // [B, C, H*W]
    int C[2];
    int tiles[2];        // ceil(C / 16), 0 for a disabled head
};

template <int PT, int NT>
__global__ __launch_bounds__(256) void k_dve_project(float* __restrict__ emb, const DveHeads h,
                                                     const int D, const int HW,
                                                     const int tiles_per_img, const int n_tiles)
{
    static_assert(PT % 4 == 0, "pixel tiles come in float4 groups");
    constexpr int NV = PT / 4;
    const int wave_tile = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (wave_tile >= n_tiles) return;                       // wave-uniform
    const int b = wave_tile / tiles_per_img;
    const int p0 = (wave_tile - b * tiles_per_img) * (16 * PT);
    const int lane = lane_id();
    const int r = lane & 15, kk = lane >> 4;

    float* const img = emb + (size_t)b * (size_t)D * (size_t)HW;
    int px[NV];
    bool pv[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        px[v] = p0 + 64 * v + 4 * r;
        pv[v] = px[v] < HW;                                 // HW % 4 == 0: all four or none
    }

    const int T = h.tiles[0] + h.tiles[1];
    float inv[PT];
    int t0 = 0;
    do {                                                    // T >= 1 on this route
        // this pass's class tiles: weight row of this lane (A operand), clamped when padded
        const float* wrow[NT];
        bool wv_ok[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int t = t0 + n;
            const int hd = t < h.tiles[0] ? 0 : 1;
            const int cl = 16 * (t - (hd ? h.tiles[0] : 0)) + r;
            wv_ok[n] = t < T && cl < h.C[hd];
            wrow[n] = wv_ok[n] ? h.w[hd] + (size_t)cl * (size_t)D : nullptr;
        }

        f32x4 acc[NT][PT];
        float ss[PT];
#pragma unroll
        for (int q = 0; q < PT; ++q) {
            ss[q] = 0.0f;
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[n][q] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }

        for (int d0 = 0; d0 < D; d0 += 16) {
            const int d = d0 + 4 * kk;
            const bool dv = d < D;                          // D % 4 == 0: all four channels or none
            f32x4 wv[NT];
#pragma unroll
            for (int n = 0; n < NT; ++n)
                wv[n] = (dv && wv_ok[n]) ? *reinterpret_cast<const f32x4*>(wrow[n] + d)
                                         : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            f32x4 xv[4][NV];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int v = 0; v < NV; ++v)
                    xv[j][v] = (dv && pv[v])
                        ? *reinterpret_cast<const f32x4*>(img + (size_t)(d + j) * (size_t)HW + px[v])
                        : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int v = 0; v < NV; ++v)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float x = xv[j][v][c];
                        ss[4 * v + c] = __fmaf_rn(x, x, ss[4 * v + c]);
#pragma unroll
                        for (int n = 0; n < NT; ++n)
                            acc[n][4 * v + c] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                                wv[n][j], x, acc[n][4 * v + c], 0, 0, 0);
                    }
        }

        // sum of squares: the four channel groups kk sit 16 lanes apart; every pass adds in the
        // same order, so the norm does not depend on the number of heads
#pragma unroll
        for (int q = 0; q < PT; ++q) {
            float s = ss[q];
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            inv[q] = 1.0f / sqrtf(s);
        }

#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int t = t0 + n;
            if (t >= T) break;                              // wave-uniform
            const int hd = t < h.tiles[0] ? 0 : 1;
            const int C = h.C[hd];
            const int c_base = 16 * (t - (hd ? h.tiles[0] : 0)) + 4 * kk;
            float* const out = h.out[hd] + (size_t)b * (size_t)C * (size_t)HW;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (c_base + i >= C) continue;
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    if (!pv[v]) continue;
                    f32x4 o;
#pragma unroll
                    for (int c = 0; c < 4; ++c) o[c] = acc[n][4 * v + c][i] * inv[4 * v + c];
                    *reinterpret_cast<f32x4*>(out + (size_t)(c_base + i) * (size_t)HW + px[v]) = o;
                }
            }
        }
        t0 += NT;
    } while (t0 < T);

    // in-place write-back: lane (r, kk) takes the channels d = kk (mod 4) of its own pixels
#pragma unroll 4
    for (int d = kk; d < D; d += 4) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            if (!pv[v]) continue;
            f32x4* const p = reinterpret_cast<f32x4*>(img + (size_t)d * (size_t)HW + px[v]);
            f32x4 x = *p;
#pragma unroll
            for (int c = 0; c < 4; ++c) x[c] *= inv[4 * v + c];
            *p = x;
        }
    }
}

// Any shape: one lane per pixel, the channels walked with stride H*W (coalesced across lanes),
// eight classes per walk, four partial sums per accumulator (channel index mod 4).
constexpr int GEN_CB = 8;

__global__ __launch_bounds__(256) void k_dve_generic(float* __restrict__ emb, const DveHeads h,
                                                     const int D, const int HW, const size_t total)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= total) return;
    const size_t b = p / (size_t)HW;
    const size_t q = p - b * (size_t)HW;
    float* const x = emb + b * (size_t)D * (size_t)HW + q;

    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int d = 0; d < D; ++d) {
        const float v = x[(size_t)d * (size_t)HW];
        s[d & 3] = __fmaf_rn(v, v, s[d & 3]);
    }
    const float inv = 1.0f / sqrtf((s[0] + s[1]) + (s[2] + s[3]));

    for (int hd = 0; hd < 2; ++hd) {
        const float* const w = h.w[hd];
        if (w == nullptr) continue;
        const int C = h.C[hd];
        float* const out = h.out[hd] + b * (size_t)C * (size_t)HW + q;
        for (int c0 = 0; c0 < C; c0 += GEN_CB) {
            float a[GEN_CB][4];
            const float* wr[GEN_CB];
#pragma unroll
            for (int k = 0; k < GEN_CB; ++k) {
                const int c = c0 + k < C ? c0 + k : C - 1;  // padded rows repeat the last class
                wr[k] = w + (size_t)c * (size_t)D;
                a[k][0] = a[k][1] = a[k][2] = a[k][3] = 0.0f;
            }
            int d = 0;
            for (; d + 3 < D; d += 4) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v = x[(size_t)(d + j) * (size_t)HW];
#pragma unroll
                    for (int k = 0; k < GEN_CB; ++k) a[k][j] = __fmaf_rn(v, wr[k][d + j], a[k][j]);
                }
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) {                   // D % 4 trailing channels
                if (d + j >= D) break;
                const float v = x[(size_t)(d + j) * (size_t)HW];
#pragma unroll
                for (int k = 0; k < GEN_CB; ++k) a[k][j] = __fmaf_rn(v, wr[k][d + j], a[k][j]);
            }
#pragma unroll
            for (int k = 0; k < GEN_CB; ++k)
                if (c0 + k < C)
                    out[(size_t)(c0 + k) * (size_t)HW] = ((a[k][0] + a[k][1]) + (a[k][2] + a[k][3])) * inv;
        }
    }

    for (int d = 0; d < D; ++d) x[(size_t)d * (size_t)HW] *= inv;
}

template <int PT, int NT>
int launch_tuned(float* emb, const DveHeads& h, int B, int D, int HW, hipStream_t stream)
{
    const int tiles_per_img = (HW + 16 * PT - 1) / (16 * PT);
    const long long n_tiles = (long long)B * tiles_per_img;                 // dve_route: fits an int
    const unsigned blocks = (unsigned)((n_tiles + 3) / 4);
    hipLaunchKernelGGL((k_dve_project<PT, NT>), dim3(blocks), dim3(256), 0, stream, emb, h, D, HW,
                       tiles_per_img, (int)n_tiles);
    return check_launch();
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

constexpr int tuned_route(int PT, int NT) { return PT * 16 + NT; }

// THE route rule: validates the arguments, fills `h` and answers NMSA_DVE_KERNEL_GENERIC (0),
// PT * 16 + NT of the k_dve_project instantiation, or the NMSA_ERR_* the call returns.  Launches
// nothing; nmsa_dve_project switches on the answer and on nothing else.
int dve_route(const float* emb, int B, int D, int H, int W,
              const float* weight_a, int Ca, const float* logits_a,
              const float* weight_b, int Cb, const float* logits_b, int route, DveHeads& h)
{
    if (!emb || B < 1 || D < 1 || H < 1 || W < 1) return NMSA_ERR_ARG;
    if (weight_a && (Ca < 1 || !logits_a)) return NMSA_ERR_ARG;
    if (weight_b && (Cb < 1 || !logits_b)) return NMSA_ERR_ARG;
    if (route != NMSA_DVE_ROUTE_AUTO && route != NMSA_DVE_ROUTE_GENERIC) return NMSA_ERR_ARG;
    if ((long long)H * W > 0x7fffffffLL) return NMSA_ERR_ARG;
    const int HW = H * W;

    h.w[0] = weight_a; h.out[0] = const_cast<float*>(logits_a); h.C[0] = weight_a ? Ca : 0;
    h.w[1] = weight_b; h.out[1] = const_cast<float*>(logits_b); h.C[1] = weight_b ? Cb : 0;
    h.tiles[0] = (h.C[0] + 15) / 16;
    h.tiles[1] = (h.C[1] + 15) / 16;
    const int T = h.tiles[0] + h.tiles[1];

    const bool tuned = route == NMSA_DVE_ROUTE_AUTO && T > 0 && D % 4 == 0 && D <= 1024 && HW % 4 == 0 &&
        h.C[0] <= 256 && h.C[1] <= 256 && aligned16(emb) &&
        (!weight_a || (aligned16(weight_a) && aligned16(logits_a))) &&
        (!weight_b || (aligned16(weight_b) && aligned16(logits_b)));
    if (!tuned) {
        const size_t blocks = ((size_t)B * (size_t)HW + 255) / 256;
        return blocks > 0x7fffffffull ? NMSA_ERR_ARG : NMSA_DVE_KERNEL_GENERIC;
    }
    // up to 48 classes in one pass: 128 pixels per wave while that still gives every SIMD of the
    // device two waves, 64 pixels on small maps; more classes: 64 pixels x 96 classes per pass
    int PT = 4;
    if (T <= 3) {
        const DeviceGeometry g = device_geometry();
        const long long waves128 = (long long)B * ((HW + 127) / 128);
        if (waves128 >= (long long)g.cus * 4 * 2) PT = 8;
    }
    const long long n_tiles = (long long)B * ((HW + 16 * PT - 1) / (16 * PT));
    if (n_tiles > 0x7fffffffLL - 4) return NMSA_ERR_ARG;
    return tuned_route(PT, T <= 3 ? 3 : 6);
}

}  // namespace
}  // namespace nmsa

using namespace nmsa;

extern "C" int nmsa_dve_project_route(const float* emb, int B, int D, int H, int W,
                                      const float* weight_a, int Ca, const float* logits_a,
                                      const float* weight_b, int Cb, const float* logits_b, int route)
{
    DveHeads h;
    return dve_route(emb, B, D, H, W, weight_a, Ca, logits_a, weight_b, Cb, logits_b, route, h);
}

extern "C" int nmsa_dve_project(float* emb, int B, int D, int H, int W,
                                const float* weight_a, int Ca, float* logits_a,
                                const float* weight_b, int Cb, float* logits_b,
                                int route, nmsa_stream_t stream_)
{
    DveHeads h;
    const int kernel = dve_route(emb, B, D, H, W, weight_a, Ca, logits_a, weight_b, Cb, logits_b, route, h);
    hipStream_t stream = (hipStream_t)stream_;
    const int HW = H * W;
    switch (kernel) {
    case NMSA_DVE_KERNEL_GENERIC: {
        const size_t total = (size_t)B * (size_t)HW;
        hipLaunchKernelGGL(k_dve_generic, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                           emb, h, D, HW, total);
        return check_launch();
    }
    case tuned_route(8, 3): return launch_tuned<8, 3>(emb, h, B, D, HW, stream);
    case tuned_route(4, 3): return launch_tuned<4, 3>(emb, h, B, D, HW, stream);
    case tuned_route(4, 6): return launch_tuned<4, 6>(emb, h, B, D, HW, stream);
    default: return kernel < 0 ? kernel : NMSA_ERR_ARG;    // an error of the rule
    }
}
