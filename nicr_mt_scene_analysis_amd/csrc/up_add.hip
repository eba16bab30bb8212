// up_add.hip — the end of every dense decoder module of the reference (model/decoder/dense_base.py):
// `Upsampling` (x2) and the `add` of the encoder skip that follows it (model/encoder_decoder_fusion.py),
// in ONE pass: x and skip are read once, y is written once.
//
//   y[n,c,Y,X] = u[n,c,Y,X] + skip[n,c,Y,X],   u = up(x)
//   nearest            u = x[n,c,Y>>1,X>>1]
//   bilinear           bilinear_src(0.5, ., .) per output row and column and bilerp of crop_resize.hpp: ATen's
//                      align_corners = False rule.  Output row 2r takes input rows r-1 and r (0.25 / 0.75),
//                      row 2r+1 rows r and min(r+1, h-1) (0.75 / 0.25); row 0 takes rows 0 and min(1, h-1)
//                      with 1 / 0 — the zero weight is multiplied, an infinity there gives ATen's NaN.
//                      Columns alike.
//   learned (+zeropad) the formula, halo rules and operation order of k_up_fwd (upsampling.hip): pre-added
//                      weight pairs, bias + 4 fused multiply-adds
// The sum is one float32 addition; a half output is rounded once, after it.
//
// Work split: k_up_fwd's.  A work item is (plane n*C+c, chunk); a plane's lane units — row
// tile of UA_TILE_H input rows x run of NP consecutive input pixels — are numbered row tile major and a
// chunk is UA_THREADS consecutive units, one per lane.  The channel is the same for the whole workgroup.
// A lane walks its tile's rows top down with a rolling three-row window in registers (nearest keeps one
// row) and per input row writes two output rows of 2 NP pixels.  NP = 2 (f32) or 4 (half): the lane's
// run of skip and y per output row is one aligned 16-byte vector.  Odd widths (w % NP != 0) and pointers
// off 16 bytes take NP = 1 with element-wise accesses.  The grid is min(items, 8 workgroups per compute
// unit of nmsa_device_geometry), grid-stride.  64-bit plane base, 32-bit offsets inside a plane (4hw <
// 2^31 is checked).
#include "crop_resize.hpp"

namespace nmsa {
namespace {

constexpr int UA_THREADS = 256;
constexpr int UA_TILE_H = 8;             // input rows a lane walks
constexpr int UA_BLOCKS_PER_CU = 8;

// what a kernel computes for u; the two learned modes differ in the halo values only (UaGeom::zeropad)
constexpr int UA_NEAREST = 0, UA_BILINEAR = 1, UA_LEARNED = 2;

// elem, ld, st, pack: nmsa_common.hpp; bilinear_src, bilerp: crop_resize.hpp

// N elements from p: one vector access on the vector route, element-wise on the one-pixel route
template <int DTYPE, int N, bool VEC>
__device__ __forceinline__ void ua_load(const typename elem<DTYPE>::type* p, float* out)
{
    typedef typename elem<DTYPE>::type S;
    if constexpr (VEC) {
        const pack<S, N> v = *(const pack<S, N>*)p;
#pragma unroll
        for (int j = 0; j < N; ++j) out[j] = ld<DTYPE>(v.v[j]);
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) out[j] = ld<DTYPE>(p[j]);
    }
}

template <int DTYPE, int N, bool VEC>
__device__ __forceinline__ void ua_store(typename elem<DTYPE>::type* p, const float* in)
{
    typedef typename elem<DTYPE>::type S;
    if constexpr (VEC) {
        pack<S, N> v;
#pragma unroll
        for (int j = 0; j < N; ++j) v.v[j] = st<DTYPE>(in[j]);
        *(pack<S, N>*)p = v;
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) p[j] = st<DTYPE>(in[j]);
    }
}

struct UaGeom {
    uint32_t C, h, w;
    uint32_t G;          // lane groups per row: w / NP
    uint32_t units;      // per plane: row tiles * G
    uint32_t chunks;     // per plane: ceil(units / UA_THREADS)
    uint32_t items;      // planes * chunks
    int zeropad;         // learned-zeropad: the halo is 0; every other mode: the border pixel
};

// input row `r` of a plane (r may be -1 or h), columns s0-1 .. s0+NP into a[0 .. NP+1]; the halo repeats
// the border pixel or, with zeropad, is 0.  HALO false (nearest): columns s0 .. s0+NP-1 only, r inside.
template <int DTYPE, int NP, bool HALO>
__device__ __forceinline__ void ua_x_row(const typename elem<DTYPE>::type* xp, int r, const UaGeom& g,
                                         uint32_t s0, float* a)
{
    if constexpr (!HALO) {
        ua_load<DTYPE, NP, (NP > 1)>(xp + (uint32_t)r * g.w + s0, a + 1);
    } else {
        const bool outside = r < 0 || r >= (int)g.h;
        if (outside && g.zeropad) {
#pragma unroll
            for (int j = 0; j < NP + 2; ++j) a[j] = 0.0f;
            return;
        }
        const uint32_t rc = r < 0 ? 0u : (r >= (int)g.h ? g.h - 1 : (uint32_t)r);
        const typename elem<DTYPE>::type* p = xp + rc * g.w + s0;
        ua_load<DTYPE, NP, (NP > 1)>(p, a + 1);
        a[0] = s0 > 0 ? ld<DTYPE>(p[-1]) : (g.zeropad ? 0.0f : a[1]);
        a[NP + 1] = s0 + NP < g.w ? ld<DTYPE>(p[NP]) : (g.zeropad ? 0.0f : a[NP]);
    }
}

template <int DTYPE, int NP, int KIND>
__global__ __launch_bounds__(UA_THREADS) void k_up_add(
    const typename elem<DTYPE>::type* __restrict__ x, const float* __restrict__ weight,
    const float* __restrict__ bias, const typename elem<DTYPE>::type* __restrict__ skip,
    typename elem<DTYPE>::type* __restrict__ y, const UaGeom g)
{
    typedef typename elem<DTYPE>::type S;
    constexpr bool HALO = KIND != UA_NEAREST;
    for (uint32_t item = blockIdx.x; item < g.items; item += gridDim.x) {
        const uint32_t plane = item / g.chunks, chunk = item - plane * g.chunks;
        const uint32_t unit = chunk * UA_THREADS + threadIdx.x;
        if (unit >= g.units) continue;
        const uint32_t tile = unit / g.G, s0 = (unit - tile * g.G) * NP;
        const uint32_t r0 = tile * UA_TILE_H, r1 = min(g.h, r0 + UA_TILE_H);
        const S* xp = x + (size_t)plane * g.h * g.w;
        const S* sp = skip + (size_t)plane * g.h * g.w * 4;
        S* yp = y + (size_t)plane * g.h * g.w * 4;

        // learned: K[dy][dx][k][l], output parity (dy, dx), k-th of its two input rows, l-th of its two columns
        float K[2][2][2][2] = {};
        float b = 0.0f;
        if constexpr (KIND == UA_LEARNED) {
            const uint32_t c = plane % g.C;
            const float* W = weight + (size_t)c * 9;
            b = bias ? bias[c] : 0.0f;
            float R[2][2][3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                R[0][0][j] = W[j];
                R[0][1][j] = W[3 + j] + W[6 + j];
                R[1][0][j] = W[j] + W[3 + j];
                R[1][1][j] = W[6 + j];
            }
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    K[dy][0][k][0] = R[dy][k][0];
                    K[dy][0][k][1] = R[dy][k][1] + R[dy][k][2];
                    K[dy][1][k][0] = R[dy][k][0] + R[dy][k][1];
                    K[dy][1][k][1] = R[dy][k][2];
                }
        }
        // bilinear: the weights of the lane's 2 NP output columns; only column 0 starts at its own pixel
        float wx0[2 * NP] = {}, wx1[2 * NP] = {};
        bool left = false;
        if constexpr (KIND == UA_BILINEAR) {
#pragma unroll
            for (int q = 0; q < 2 * NP; ++q) {
                int ix0, ix1;
                bilinear_src(0.5f, (int)(2 * s0) + q, (int)g.w, ix0, ix1, wx0[q], wx1[q]);
                if (q == 0) left = ix0 == (int)s0;
            }
        }

        float a[3][NP + 2];                 // rows r-1, r, r+1 (nearest: a[1] alone)
        if constexpr (HALO) {
            ua_x_row<DTYPE, NP, true>(xp, (int)r0 - 1, g, s0, a[0]);
            ua_x_row<DTYPE, NP, true>(xp, (int)r0, g, s0, a[1]);
        }
        for (uint32_t r = r0; r < r1; ++r) {
            if constexpr (HALO) ua_x_row<DTYPE, NP, true>(xp, (int)r + 1, g, s0, a[2]);
            else ua_x_row<DTYPE, NP, false>(xp, (int)r, g, s0, a[1]);
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                const uint32_t off = (2 * r + dy) * (2 * g.w) + 2 * s0;
                float out[2 * NP], sk[2 * NP];
                ua_load<DTYPE, 2 * NP, (NP > 1)>(sp + off, sk);
                if constexpr (KIND == UA_NEAREST) {
#pragma unroll
                    for (int q = 0; q < 2 * NP; ++q) out[q] = a[1][q / 2 + 1];
                } else if constexpr (KIND == UA_BILINEAR) {
                    int iy0, iy1;
                    float wy0, wy1;
                    bilinear_src(0.5f, (int)(2 * r) + dy, (int)g.h, iy0, iy1, wy0, wy1);
                    // the two source rows: r-1 and r for an even output row, but 0 and min(1, h-1) for row 0;
                    // r and min(r+1, h-1) for an odd one
                    const bool top = dy == 0 && iy0 == (int)r;
                    float t0[NP + 2], t1[NP + 2];
#pragma unroll
                    for (int j = 0; j < NP + 2; ++j) {
                        t0[j] = (dy == 1 || top) ? a[1][j] : a[0][j];
                        t1[j] = (dy == 1 || top) ? a[2][j] : a[1][j];
                    }
#pragma unroll
                    for (int p = 0; p < NP; ++p) {
                        // even column: pixels s-1 and s, but 0 and min(1, w-1) for column 0; odd: s and min(s+1, w-1)
                        const bool lf = p == 0 && left;
                        const int e0 = p, e1 = p + 1, e2 = p + 2;           // a[.][p + 1] is pixel p
                        out[2 * p] = bilerp(lf ? t0[e1] : t0[e0], lf ? t0[e2] : t0[e1],
                                            lf ? t1[e1] : t1[e0], lf ? t1[e2] : t1[e1],
                                            wx0[2 * p], wx1[2 * p], wy0, wy1);
                        out[2 * p + 1] = bilerp(t0[e1], t0[e2], t1[e1], t1[e2],
                                                wx0[2 * p + 1], wx1[2 * p + 1], wy0, wy1);
                    }
                } else {
#pragma unroll
                    for (int p = 0; p < NP; ++p)
#pragma unroll
                        for (int dx = 0; dx < 2; ++dx) {
                            const int i0 = p + dx;
                            float acc = b;
                            acc = __fmaf_rn(K[dy][dx][0][0], a[dy][i0], acc);
                            acc = __fmaf_rn(K[dy][dx][0][1], a[dy][i0 + 1], acc);
                            acc = __fmaf_rn(K[dy][dx][1][0], a[dy + 1][i0], acc);
                            acc = __fmaf_rn(K[dy][dx][1][1], a[dy + 1][i0 + 1], acc);
                            out[2 * p + dx] = acc;
                        }
                }
#pragma unroll
                for (int q = 0; q < 2 * NP; ++q) out[q] = __fadd_rn(out[q], sk[q]);
                ua_store<DTYPE, 2 * NP, (NP > 1)>(yp + off, out);
            }
            if constexpr (HALO) {
#pragma unroll
                for (int j = 0; j < NP + 2; ++j) { a[0][j] = a[1][j]; a[1][j] = a[2][j]; }
            }
        }
    }
}

int ua_run(int dtype) { return dtype == NMSA_F32 ? 2 : 4; }

// THE route rule: the vector route needs the lane run to divide the width and every tensor on 16 bytes
bool ua_vector(int dtype, int w, const void* x, const void* skip, const void* y)
{
    return w % ua_run(dtype) == 0 && aligned(x, 16) && aligned(skip, 16) && aligned(y, 16);
}

bool ua_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes)
{
    const uint64_t a0 = (uint64_t)(uintptr_t)a, b0 = (uint64_t)(uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// what both entry points check of the tensors; NMSA_OK, NMSA_ERR_ARG or NMSA_ERR_UNSUPPORTED
int ua_check(const void* x, const void* skip, const void* y, int dtype, int B, int C, int h, int w)
{
    if (dtype != NMSA_F32 && dtype != NMSA_BF16 && dtype != NMSA_F16) return NMSA_ERR_ARG;
    if (B < 1 || C < 1 || h < 1 || w < 1) return NMSA_ERR_ARG;
    if (!x || !skip || !y) return NMSA_ERR_ARG;
    if (!elem_aligned(x, dtype) || !elem_aligned(skip, dtype) || !elem_aligned(y, dtype)) return NMSA_ERR_ARG;
    if ((int64_t)h * w * 4 > 0x7fffffffLL) return NMSA_ERR_UNSUPPORTED;     // 32-bit offsets inside a plane
    if ((int64_t)B * C > 0x7fffffffLL) return NMSA_ERR_UNSUPPORTED;
    // below 2^31 planes of below 2^31 elements of at most 4 bytes: the byte counts fit 64 bits
    const uint64_t in_bytes = (uint64_t)B * C * h * w * elem_bytes(dtype), out_bytes = in_bytes * 4;
    if (ua_overlap(y, out_bytes, x, in_bytes) || ua_overlap(y, out_bytes, skip, out_bytes)) return NMSA_ERR_ARG;
    return NMSA_OK;
}

// work items of a call with NP pixels per lane; false when there are 2^31 or more
bool ua_geometry(int B, int C, int h, int w, int NP, int zeropad, UaGeom& g)
{
    g.C = (uint32_t)C; g.h = (uint32_t)h; g.w = (uint32_t)w; g.zeropad = zeropad;
    g.G = (uint32_t)(w / NP);
    const uint64_t tiles = ((uint64_t)h + UA_TILE_H - 1) / UA_TILE_H;
    const uint64_t units = tiles * g.G;                               // <= h * w < 2^29
    const uint64_t chunks = (units + UA_THREADS - 1) / UA_THREADS;
    const uint64_t items = (uint64_t)B * C * chunks;
    if (items > 0x7fffffffull) return false;                  // item + gridDim.x stays below 2^32
    g.units = (uint32_t)units; g.chunks = (uint32_t)chunks; g.items = (uint32_t)items;
    return true;
}

template <int DTYPE, int KIND>
void ua_launch(bool vec, dim3 grid, hipStream_t stream, const void* x, const float* weight, const float* bias,
               const void* skip, void* y, const UaGeom& g)
{
    typedef typename elem<DTYPE>::type S;
    const dim3 block(UA_THREADS);
    if (vec) hipLaunchKernelGGL((k_up_add<DTYPE, (DTYPE == NMSA_F32 ? 2 : 4), KIND>), grid, block, 0, stream,
                                (const S*)x, weight, bias, (const S*)skip, (S*)y, g);
    else hipLaunchKernelGGL((k_up_add<DTYPE, 1, KIND>), grid, block, 0, stream, (const S*)x, weight, bias,
                            (const S*)skip, (S*)y, g);
}

}  // namespace
}  // namespace nmsa

extern "C" int nmsa_up2x_add_route(const void* x, const void* skip, const void* y, int dtype,
                                   int B, int C, int h, int w)
{
    using namespace nmsa;
    const int rc = ua_check(x, skip, y, dtype, B, C, h, w);
    if (rc != NMSA_OK) return rc;
    const bool vec = ua_vector(dtype, w, x, skip, y);
    UaGeom g;
    if (!ua_geometry(B, C, h, w, vec ? ua_run(dtype) : 1, 0, g)) return NMSA_ERR_UNSUPPORTED;
    return vec ? NMSA_UPADD_ROUTE_VECTOR : NMSA_UPADD_ROUTE_PIXEL;
}

extern "C" int nmsa_up2x_add_fwd(const void* x, int dtype, int mode, const float* weight, const float* bias,
                                 const void* skip, int B, int C, int h, int w, void* y, nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    if (mode != NMSA_UPADD_NEAREST && mode != NMSA_UPADD_BILINEAR && mode != NMSA_UPADD_LEARNED &&
        mode != NMSA_UPADD_LEARNED_ZEROPAD)
        return NMSA_ERR_ARG;
    const bool learned = mode == NMSA_UPADD_LEARNED || mode == NMSA_UPADD_LEARNED_ZEROPAD;
    if (learned && (!weight || !aligned(weight, 4) || !aligned(bias, 4))) return NMSA_ERR_ARG;
    const int rc = ua_check(x, skip, y, dtype, B, C, h, w);
    if (rc != NMSA_OK) return rc;
    if (!learned) weight = bias = nullptr;                    // ignored in the other two modes
    const bool vec = ua_vector(dtype, w, x, skip, y);
    UaGeom g;
    if (!ua_geometry(B, C, h, w, vec ? ua_run(dtype) : 1, mode == NMSA_UPADD_LEARNED_ZEROPAD, g))
        return NMSA_ERR_UNSUPPORTED;
    const dim3 grid(capped_grid(g.items, UA_BLOCKS_PER_CU));
#define UA_FWD(DT)                                                                                         \
    do {                                                                                                   \
        if (mode == NMSA_UPADD_NEAREST) ua_launch<DT, UA_NEAREST>(vec, grid, stream, x, weight, bias, skip, y, g);   \
        else if (mode == NMSA_UPADD_BILINEAR)                                                              \
            ua_launch<DT, UA_BILINEAR>(vec, grid, stream, x, weight, bias, skip, y, g);                    \
        else ua_launch<DT, UA_LEARNED>(vec, grid, stream, x, weight, bias, skip, y, g);                    \
    } while (0)
    NMSA_DISPATCH_DTYPE(dtype, UA_FWD)
#undef UA_FWD
    return check_launch();
}
