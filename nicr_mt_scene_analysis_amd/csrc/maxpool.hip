// maxpool.hip — the stem max pool of the ResNet backbones (model/backbone/resnet.py: nn.MaxPool2d(3, 2, 1) at
// the head of stage 1): kernel 3x3, stride 2, padding 1, dilation 1, floor mode, forward and backward, each in
// ONE pass over its tensors.  Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1.
//
//   k_mp_fwd   x read once, y written once and, for training, a ONE-BYTE code per output pixel in place of
//              ATen's int64 index: code = 3 * (r - (2 oy - 1)) + (c - (2 ox - 1)), the window position 0..8 of
//              the input pixel (r, c) ATen's index names.  Selection is ATen's rule with explicit comparisons:
//              the valid (non-padded) window positions in row-major order, starting at the first, replaced
//              when `val > max || isnan(val)`: ties (signed zeros included) keep the first position, a window
//              with NaNs selects its last NaN, an all -inf window its first position.  y carries the selected
//              element's BITS.  The rule is separable: scanning each window row by it and then the three row
//              winners by it selects the same element (no NaN: the first row holding the maximum and the first
//              position in it; NaNs: the last row holding one and the last NaN in it), so the scan of input
//              row 2 oy + 1 serves output rows oy and oy + 1.
//   k_mp_bwd   gather form: gx[r, c] = sum of gy[oy, ox] over the at most four windows that cover (r, c) and
//              whose code points at it, oy ascending, then ox ascending, added in float32 from 0 and rounded
//              once for a half output.  Every gx element is written; no atomics, no memset: two calls give the
//              same bits.  Row r = 2 oy is covered by window row oy alone (window row 1), row 2 oy + 1 by
//              window rows oy (row 2) and oy + 1 (row 0); columns alike.
//
// Work split (both kernels).  A unit is a row tile of MP_TILE_H OUTPUT rows x a group of NO consecutive output
// pixels; the units of all planes are numbered plane major, row tile major, and a work item is MP_THREADS
// consecutive units, one per lane.  A lane walks its tile's rows top down and keeps the row it shares with the
// next output row in registers.  VECTOR route: NO = 2 (f32) / 4 (half), the lane's 2 NO input (gx) elements of
// a row are one aligned 16-byte vector, its y (gy) run is 8 bytes, its codes 2 / 4 bytes; the one halo element
// of a row comes as an aligned dword for the halves (never a 2-byte load).  Taken when W % (2 NO) == 0 and
// every tensor of the call starts on 16 bytes.  PIXEL route: NO = 1, element-wise accesses, any width and any
// element-aligned pointer.  Both routes give the same bits.
// The grid is min(items, 8 workgroups per compute unit of nmsa_device_geometry), grid-stride.
// Addressing: 64-bit plane base, 32-bit offsets inside a plane (H W < 2^31 is checked).
#include "nmsa_common.hpp"

namespace nmsa {
namespace {

constexpr int MP_THREADS = 256;
constexpr int MP_TILE_H = 8;             // output rows a lane walks
constexpr int MP_BLOCKS_PER_CU = 8;
constexpr uint32_t MP_NO_CODE = 255u;    // a window outside the map: matches no position

// elem, ld, st, pack: nmsa_common.hpp

// the element p[0].  VEC: p is 4-byte aligned and p[1] lies inside the row, a half comes as the low part of
// one dword
template <int DTYPE, bool VEC>
__device__ __forceinline__ typename elem<DTYPE>::type mp_first(const typename elem<DTYPE>::type* p)
{
    if constexpr (VEC && DTYPE != NMSA_F32) return (uint16_t)(*(const uint32_t*)p & 0xffffu);
    else return p[0];
}

// the element p[-1].  VEC: p is 4-byte aligned and p[-2] lies inside the row, a half comes as the high part
// of one dword
template <int DTYPE, bool VEC>
__device__ __forceinline__ typename elem<DTYPE>::type mp_before(const typename elem<DTYPE>::type* p)
{
    if constexpr (VEC && DTYPE != NMSA_F32) return (uint16_t)(*(const uint32_t*)(p - 2) >> 16);
    else return p[-1];
}

struct MpGeom {
    uint32_t H, W, Ho, Wo;
    uint32_t G;          // lane groups per output row: Wo / NO
    uint32_t units;      // per plane: row tiles * G
    uint32_t total;      // planes * units
    uint32_t items;      // ceil(total / MP_THREADS)
};

// the current choice of a scan: the value compared, the element's bits, its position
template <typename S>
struct mp_sel {
    float v;
    S b;
    uint32_t k;
};

// ATen's replacement rule
template <typename S>
__device__ __forceinline__ void mp_take(mp_sel<S>& m, float v, S b, uint32_t k)
{
    const bool t = v > m.v || v != v;
    m.v = t ? v : m.v;
    m.b = t ? b : m.b;
    m.k = t ? k : m.k;
}

// input row r (inside the map) scanned for the NO output pixels from ox0: the winner of the columns
// 2 ox - 1, 2 ox, 2 ox + 1 that lie inside the map, k = its column position 0..2
template <int DTYPE, int NO, bool VEC>
__device__ __forceinline__ void mp_scan_row(const typename elem<DTYPE>::type* xp, uint32_t r, const MpGeom& g,
                                            uint32_t ox0, mp_sel<typename elem<DTYPE>::type>* out)
{
    typedef typename elem<DTYPE>::type S;
    const S* p = xp + r * g.W + 2 * ox0;
    S a[2 * NO + 1];                         // a[0]: column 2 ox0 - 1
    const bool left = ox0 > 0;
    if constexpr (VEC) {
        const pack<S, 2 * NO> v = *(const pack<S, 2 * NO>*)p;
#pragma unroll
        for (int j = 0; j < 2 * NO; ++j) a[j + 1] = v.v[j];
        a[0] = left ? mp_before<DTYPE, true>(p) : a[1];
    } else {
        a[1] = p[0];
        a[0] = left ? p[-1] : a[1];
        a[2] = 2 * ox0 + 1 < g.W ? p[1] : a[1];
    }
    const bool right = VEC || 2 * ox0 + 1 < g.W;         // NO == 1 off the vector route
#pragma unroll
    for (int j = 0; j < NO; ++j) {
        mp_sel<S> m;
        if (j == 0 && !left) {
            m.v = ld<DTYPE>(a[1]); m.b = a[1]; m.k = 1u;
        } else {
            m.v = ld<DTYPE>(a[2 * j]); m.b = a[2 * j]; m.k = 0u;
            mp_take(m, ld<DTYPE>(a[2 * j + 1]), a[2 * j + 1], 1u);
        }
        if (right) mp_take(m, ld<DTYPE>(a[2 * j + 2]), a[2 * j + 2], 2u);
        out[j] = m;
    }
}

template <int DTYPE, int NO>
__global__ __launch_bounds__(MP_THREADS) void k_mp_fwd(
    const typename elem<DTYPE>::type* __restrict__ x, typename elem<DTYPE>::type* __restrict__ y,
    uint8_t* __restrict__ code, const MpGeom g)
{
    typedef typename elem<DTYPE>::type S;
    constexpr bool VEC = NO > 1;
    for (uint32_t item = blockIdx.x; item < g.items; item += gridDim.x) {
        const uint32_t gu = item * MP_THREADS + threadIdx.x;
        if (gu >= g.total) continue;
        const uint32_t plane = gu / g.units, u = gu - plane * g.units;
        const uint32_t tile = u / g.G, ox0 = (u - tile * g.G) * NO;
        const uint32_t oy0 = tile * MP_TILE_H, oy1 = min(g.Ho, oy0 + MP_TILE_H);
        const S* xp = x + (size_t)plane * g.H * g.W;
        const size_t obase = (size_t)plane * g.Ho * g.Wo;
        mp_sel<S> prev[NO], mid[NO], next[NO];
#pragma unroll
        for (int j = 0; j < NO; ++j) {
            prev[j].v = 0.0f; prev[j].b = S(0); prev[j].k = 0u;
            next[j] = prev[j];
        }
        if (oy0 > 0) mp_scan_row<DTYPE, NO, VEC>(xp, 2 * oy0 - 1, g, ox0, prev);
        for (uint32_t oy = oy0; oy < oy1; ++oy) {
            mp_scan_row<DTYPE, NO, VEC>(xp, 2 * oy, g, ox0, mid);
            const bool below = 2 * oy + 1 < g.H;
            if (below) mp_scan_row<DTYPE, NO, VEC>(xp, 2 * oy + 1, g, ox0, next);
            pack<S, NO> yv;
            pack<uint8_t, NO> kv;
#pragma unroll
            for (int j = 0; j < NO; ++j) {
                mp_sel<S> m;
                if (oy > 0) {
                    m = prev[j];
                    mp_take(m, mid[j].v, mid[j].b, 3u + mid[j].k);
                } else {
                    m = mid[j];
                    m.k += 3u;
                }
                if (below) mp_take(m, next[j].v, next[j].b, 6u + next[j].k);
                yv.v[j] = m.b;
                kv.v[j] = (uint8_t)m.k;
            }
            const uint32_t o = oy * g.Wo + ox0;
            *(pack<S, NO>*)(y + obase + o) = yv;
            if (code) *(pack<uint8_t, NO>*)(code + obase + o) = kv;
#pragma unroll
            for (int j = 0; j < NO; ++j) prev[j] = next[j];
        }
    }
}

// window row oy for the outputs ox0 .. ox0 + NO (the last one: the right neighbour's first): gy and code;
// MP_NO_CODE where the window lies outside the map
template <int DTYPE, int NO, bool VEC>
__device__ __forceinline__ void mp_gy_row(const typename elem<DTYPE>::type* gp, const uint8_t* cp, uint32_t oy,
                                          const MpGeom& g, uint32_t ox0, float* gv, uint32_t* cd)
{
    typedef typename elem<DTYPE>::type S;
    if (oy >= g.Ho) {
#pragma unroll
        for (int j = 0; j <= NO; ++j) { gv[j] = 0.0f; cd[j] = MP_NO_CODE; }
        return;
    }
    const uint32_t o = oy * g.Wo + ox0;
    const pack<S, NO> gvec = *(const pack<S, NO>*)(gp + o);
    const pack<uint8_t, NO> cvec = *(const pack<uint8_t, NO>*)(cp + o);
#pragma unroll
    for (int j = 0; j < NO; ++j) { gv[j] = ld<DTYPE>(gvec.v[j]); cd[j] = cvec.v[j]; }
    if (ox0 + NO < g.Wo) {
        gv[NO] = ld<DTYPE>(mp_first<DTYPE, VEC>(gp + o + NO));
        // Wo is a multiple of NO on the vector route: the pair (quad) behind the lane's codes lies inside the row
        if constexpr (VEC) cd[NO] = (uint32_t)(*(const pack<uint8_t, NO>*)(cp + o + NO)).v[0];
        else cd[NO] = cp[o + NO];
    } else {
        gv[NO] = 0.0f; cd[NO] = MP_NO_CODE;
    }
}

// the share of one window row in the gx elements 2 ox0 .. 2 ox0 + 2 NO - 1 of an input row that is the
// window's row `dr`; ox ascending
template <int NO>
__device__ __forceinline__ void mp_gather(float* acc, const float* gv, const uint32_t* cd, uint32_t dr)
{
#pragma unroll
    for (int j = 0; j < NO; ++j) {
        if (cd[j] == 3u * dr + 1u) acc[2 * j] += gv[j];
        if (cd[j] == 3u * dr + 2u) acc[2 * j + 1] += gv[j];
        if (cd[j + 1] == 3u * dr) acc[2 * j + 1] += gv[j + 1];
    }
}

template <int DTYPE, int NO>
__device__ __forceinline__ void mp_gx_store(typename elem<DTYPE>::type* p, const float* acc, bool second)
{
    typedef typename elem<DTYPE>::type S;
    if constexpr (NO > 1) {
        pack<S, 2 * NO> v;
#pragma unroll
        for (int j = 0; j < 2 * NO; ++j) v.v[j] = st<DTYPE>(acc[j]);
        *(pack<S, 2 * NO>*)p = v;
    } else {
        p[0] = st<DTYPE>(acc[0]);
        if (second) p[1] = st<DTYPE>(acc[1]);
    }
}

template <int DTYPE, int NO>
__global__ __launch_bounds__(MP_THREADS) void k_mp_bwd(
    const typename elem<DTYPE>::type* __restrict__ gy, const uint8_t* __restrict__ code,
    typename elem<DTYPE>::type* __restrict__ gx, const MpGeom g)
{
    typedef typename elem<DTYPE>::type S;
    constexpr bool VEC = NO > 1;
    for (uint32_t item = blockIdx.x; item < g.items; item += gridDim.x) {
        const uint32_t gu = item * MP_THREADS + threadIdx.x;
        if (gu >= g.total) continue;
        const uint32_t plane = gu / g.units, u = gu - plane * g.units;
        const uint32_t tile = u / g.G, ox0 = (u - tile * g.G) * NO;
        const uint32_t oy0 = tile * MP_TILE_H, oy1 = min(g.Ho, oy0 + MP_TILE_H);
        const size_t obase = (size_t)plane * g.Ho * g.Wo;
        const S* gp = gy + obase;
        const uint8_t* cp = code + obase;
        S* xp = gx + (size_t)plane * g.H * g.W;
        const bool second = VEC || 2 * ox0 + 1 < g.W;     // column 2 ox0 + 1 of the one-pixel route
        float gc[NO + 1], gn[NO + 1];
        uint32_t cc[NO + 1], cn[NO + 1];
        mp_gy_row<DTYPE, NO, VEC>(gp, cp, oy0, g, ox0, gc, cc);
        for (uint32_t oy = oy0; oy < oy1; ++oy) {
            mp_gy_row<DTYPE, NO, VEC>(gp, cp, oy + 1, g, ox0, gn, cn);
            float acc[2 * NO];
#pragma unroll
            for (int j = 0; j < 2 * NO; ++j) acc[j] = 0.0f;
            mp_gather<NO>(acc, gc, cc, 1u);
            mp_gx_store<DTYPE, NO>(xp + (2 * oy) * g.W + 2 * ox0, acc, second);
            if (2 * oy + 1 < g.H) {
#pragma unroll
                for (int j = 0; j < 2 * NO; ++j) acc[j] = 0.0f;
                mp_gather<NO>(acc, gc, cc, 2u);
                mp_gather<NO>(acc, gn, cn, 0u);
                mp_gx_store<DTYPE, NO>(xp + (2 * oy + 1) * g.W + 2 * ox0, acc, second);
            }
#pragma unroll
            for (int j = 0; j <= NO; ++j) { gc[j] = gn[j]; cc[j] = cn[j]; }
        }
    }
}

int mp_run(int dtype) { return dtype == NMSA_F32 ? 2 : 4; }          // output pixels of a lane, vector route

// sizes every entry point checks; NMSA_OK, NMSA_ERR_ARG or NMSA_ERR_UNSUPPORTED
int mp_check_sizes(int dtype, int B, int C, int H, int W)
{
    if (dtype != NMSA_F32 && dtype != NMSA_BF16 && dtype != NMSA_F16) return NMSA_ERR_ARG;
    if (B < 1 || C < 1 || H < 1 || W < 1) return NMSA_ERR_ARG;
    if ((int64_t)H * W > 0x7fffffffLL) return NMSA_ERR_UNSUPPORTED;         // 32-bit offsets inside a plane
    if ((int64_t)B * C > 0x7fffffffLL) return NMSA_ERR_UNSUPPORTED;
    return NMSA_OK;
}

// units of a call with NO output pixels per lane; false when there are 2^31 or more
bool mp_geometry(int B, int C, int H, int W, int NO, MpGeom& g)
{
    g.H = (uint32_t)H; g.W = (uint32_t)W;
    g.Ho = (uint32_t)((H - 1) / 2 + 1); g.Wo = (uint32_t)((W - 1) / 2 + 1);
    g.G = g.Wo / (uint32_t)NO;
    const uint64_t tiles = ((uint64_t)g.Ho + MP_TILE_H - 1) / MP_TILE_H;
    const uint64_t units = tiles * g.G;                               // <= Ho * Wo < 2^31
    const uint64_t total = (uint64_t)B * C * units;
    if (total > 0x7fffffffull) return false;              // item * MP_THREADS + lane stays below 2^32
    g.units = (uint32_t)units; g.total = (uint32_t)total;
    g.items = (uint32_t)((total + MP_THREADS - 1) / MP_THREADS);
    return true;
}

// THE route rule: the vector route needs the lane's input run to divide the width and every tensor of the
// call on 16 bytes
bool mp_vector(int dtype, int W, const void* a, const void* b, const void* c)
{
    return W % (2 * mp_run(dtype)) == 0 && aligned(a, 16) && aligned(b, 16) && aligned(c, 16);
}

}  // namespace
}  // namespace nmsa

extern "C" int nmsa_maxpool3x3s2_route(const void* x, const void* y_or_gx, int dtype, int B, int C, int H, int W)
{
    using namespace nmsa;
    const int rc = mp_check_sizes(dtype, B, C, H, W);
    if (rc != NMSA_OK) return rc;
    const uintptr_t e = (uintptr_t)elem_bytes(dtype);
    if (!x || !y_or_gx || !aligned(x, e) || !aligned(y_or_gx, e)) return NMSA_ERR_ARG;
    return mp_vector(dtype, W, x, y_or_gx, nullptr) ? NMSA_MP_ROUTE_VECTOR : NMSA_MP_ROUTE_PIXEL;
}

extern "C" int nmsa_maxpool3x3s2_fwd(const void* x, int dtype, int B, int C, int H, int W, void* y,
                                     uint8_t* code, nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = mp_check_sizes(dtype, B, C, H, W);
    if (rc != NMSA_OK) return rc;
    const uintptr_t e = (uintptr_t)elem_bytes(dtype);
    if (!x || !y || !aligned(x, e) || !aligned(y, e)) return NMSA_ERR_ARG;
    const bool vec = mp_vector(dtype, W, x, y, code);
    MpGeom g;
    if (!mp_geometry(B, C, H, W, vec ? mp_run(dtype) : 1, g)) return NMSA_ERR_UNSUPPORTED;
    const dim3 grid(capped_grid(g.items, MP_BLOCKS_PER_CU)), block(MP_THREADS);
#define MP_FWD(DT)                                                                                          \
    do {                                                                                                    \
        typedef elem<DT>::type S;                                                                           \
        if (vec) hipLaunchKernelGGL((k_mp_fwd<DT, (DT == NMSA_F32 ? 2 : 4)>), grid, block, 0, stream,       \
                                    (const S*)x, (S*)y, code, g);                                           \
        else hipLaunchKernelGGL((k_mp_fwd<DT, 1>), grid, block, 0, stream, (const S*)x, (S*)y, code, g);    \
    } while (0)
    NMSA_DISPATCH_DTYPE(dtype, MP_FWD)
#undef MP_FWD
    return check_launch();
}

extern "C" int nmsa_maxpool3x3s2_bwd(const void* gy, const uint8_t* code, int dtype, int B, int C, int H, int W,
                                     void* gx, nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = mp_check_sizes(dtype, B, C, H, W);
    if (rc != NMSA_OK) return rc;
    const uintptr_t e = (uintptr_t)elem_bytes(dtype);
    if (!gy || !code || !gx || !aligned(gy, e) || !aligned(gx, e)) return NMSA_ERR_ARG;
    const bool vec = mp_vector(dtype, W, gy, code, gx);
    MpGeom g;
    if (!mp_geometry(B, C, H, W, vec ? mp_run(dtype) : 1, g)) return NMSA_ERR_UNSUPPORTED;
    const dim3 grid(capped_grid(g.items, MP_BLOCKS_PER_CU)), block(MP_THREADS);
#define MP_BWD(DT)                                                                                          \
    do {                                                                                                    \
        typedef elem<DT>::type S;                                                                           \
        if (vec) hipLaunchKernelGGL((k_mp_bwd<DT, (DT == NMSA_F32 ? 2 : 4)>), grid, block, 0, stream,       \
                                    (const S*)gy, code, (S*)gx, g);                                         \
        else hipLaunchKernelGGL((k_mp_bwd<DT, 1>), grid, block, 0, stream, (const S*)gy, code, (S*)gx, g);  \
    } while (0)
    NMSA_DISPATCH_DTYPE(dtype, MP_BWD)
#undef MP_BWD
    return check_launch();
}
