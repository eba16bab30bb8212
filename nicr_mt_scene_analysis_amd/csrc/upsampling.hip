// upsampling.hip — the learned x2 head upsampling of the reference (model/upsampling.py:39-96,
// modes 'learned-3x3' and 'learned-3x3-zeropad'): nearest x2, replication or zero pad, depthwise
// 3x3 convolution, forward and backward, each in ONE pass over its tensors.
//
//   y[n,c,Y,X] = b[c] + sum_{i,j in 0..2} W[c,0,i,j] * U(Y+i-1, X+j-1)
//   U(p,q)     = x[n,c,p>>1,q>>1] for 0 <= p < 2h, 0 <= q < 2w
//   replicate: p, q clamped to that range first;   zeropad: 0 outside it
//
//   k_up_fwd     x read once, y written once.  The three weight rows (and columns) collapse per
//                output parity: the even output row 2r takes W[0] on input row r-1 and W[1]+W[2] on
//                row r, the odd row 2r+1 takes W[0]+W[1] on r and W[2] on r+1; an output pixel is
//                bias + 4 fused multiply-adds.  Both pad modes are a rule for the HALO values only
//                (row r-1 at r = 0, column s-1 at s = 0, ...): replicate repeats the border pixel,
//                zero pad puts 0 there — the collapsed weights are the same everywhere.
//   k_up_bwd     gy and x read once; gx written, and per workgroup ten partial sums (gW 3x3, gb)
//                into the workspace.  Input pixel (r,s) owns the 4x4 window gy[2r-1..2r+2,
//                2s-1..2s+2] (0 outside the map).  With the membership sets
//                    rows of tap i:  i=0 {2,3}  i=1 {1,2}  i=2 {0,1}      (window row a = Y-2r+1)
//                    replicate only: i=0 gains row 1 at r = 0, i=2 gains row 2 at r = h-1
//                (columns alike) P[i][j] = sum of the window over rows(i) x columns(j), and
//                    gx[r,s] = sum_ij W[i][j] * P[i][j],  gW[i][j] += x[r,s] * P[i][j],
//                    gb += the four gy of the pixel itself.   No atomics: gx is a gather.
//   k_up_reduce  one wave per channel sums that channel's partials in a fixed order into gW, gb:
//                no float atomics anywhere, two calls give the same bits.
//
// Work split (both kernels).  A work item is (plane n*C+c, chunk): the plane's lane units — row
// tile of UP_TILE_H input rows x group of NP consecutive input pixels — are numbered row tile
// major, and a chunk is UP_THREADS consecutive units, one per lane.  The channel is the same for
// the whole workgroup (weights in scalar registers, one partial per item); a lane walks its tile's
// rows top down with a rolling window, so every input row is fetched by ~(UP_TILE_H+2)/UP_TILE_H
// lanes and each gy row by one.  NP = 2 (f32) or 4 (half): the lane's output run per row is one
// aligned 16-byte vector and consecutive lanes store consecutive vectors.  Odd widths (w % NP != 0)
// and pointers off 16 bytes take NP = 1 with element-wise accesses (no alignment assumed).
// The grid is min(items, 8 workgroups per compute unit of nmsa_device_geometry), grid-stride.
// Addressing: 64-bit plane base, 32-bit offsets inside a plane (4hw < 2^31 is checked).
#include "nmsa_common.hpp"

namespace nmsa {
namespace {

constexpr int UP_THREADS = 256;
constexpr int UP_TILE_H = 8;             // input rows a lane walks
constexpr int UP_BLOCKS_PER_CU = 8;
constexpr int UP_PARTIAL = 10;           // gW[3][3], gb
constexpr int UP_REDUCE_THREADS = 64;

// elem, ld, st, pack: nmsa_common.hpp

// N elements from p: one vector access on the vector route, element-wise on the one-pixel route
template <int DTYPE, int N, bool VEC>
__device__ __forceinline__ void up_load(const typename elem<DTYPE>::type* p, float* out)
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
__device__ __forceinline__ void up_store(typename elem<DTYPE>::type* p, const float* in)
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

struct UpGeom {
    uint32_t C, h, w;
    uint32_t G;          // lane groups per row: w / NP
    uint32_t units;      // per plane: row tiles * G
    uint32_t chunks;     // per plane: ceil(units / UP_THREADS)
    uint32_t items;      // planes * chunks
    int zeropad;
};

// input row `r` of a plane (r may be -1 or h), columns s0-1 .. s0+NP, halo by the pad mode
template <int DTYPE, int NP>
__device__ __forceinline__ void up_x_row(const typename elem<DTYPE>::type* xp, int r, const UpGeom& g,
                                         uint32_t s0, float* a)
{
    const bool outside = r < 0 || r >= (int)g.h;
    if (outside && g.zeropad) {
#pragma unroll
        for (int j = 0; j < NP + 2; ++j) a[j] = 0.0f;
        return;
    }
    const uint32_t rc = r < 0 ? 0u : (r >= (int)g.h ? g.h - 1 : (uint32_t)r);
    const typename elem<DTYPE>::type* p = xp + rc * g.w + s0;
    up_load<DTYPE, NP, (NP > 1)>(p, a + 1);
    a[0] = s0 > 0 ? ld<DTYPE>(p[-1]) : (g.zeropad ? 0.0f : a[1]);
    a[NP + 1] = s0 + NP < g.w ? ld<DTYPE>(p[NP]) : (g.zeropad ? 0.0f : a[NP]);
}

template <int DTYPE, int NP>
__global__ __launch_bounds__(UP_THREADS) void k_up_fwd(
    const typename elem<DTYPE>::type* __restrict__ x, const float* __restrict__ weight,
    const float* __restrict__ bias, typename elem<DTYPE>::type* __restrict__ y, const UpGeom g)
{
    typedef typename elem<DTYPE>::type S;
    for (uint32_t item = blockIdx.x; item < g.items; item += gridDim.x) {
        const uint32_t plane = item / g.chunks, chunk = item - plane * g.chunks;
        const uint32_t unit = chunk * UP_THREADS + threadIdx.x;
        if (unit >= g.units) continue;
        const uint32_t c = plane % g.C;
        const float* W = weight + (size_t)c * 9;
        const float b = bias ? bias[c] : 0.0f;
        // K[dy][dx][k][l]: output parity (dy, dx), k-th of its two input rows, l-th of its two columns
        float R[2][2][3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            R[0][0][j] = W[j];
            R[0][1][j] = W[3 + j] + W[6 + j];
            R[1][0][j] = W[j] + W[3 + j];
            R[1][1][j] = W[6 + j];
        }
        float K[2][2][2][2];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                K[dy][0][k][0] = R[dy][k][0];
                K[dy][0][k][1] = R[dy][k][1] + R[dy][k][2];
                K[dy][1][k][0] = R[dy][k][0] + R[dy][k][1];
                K[dy][1][k][1] = R[dy][k][2];
            }
        const uint32_t tile = unit / g.G, s0 = (unit - tile * g.G) * NP;
        const uint32_t r0 = tile * UP_TILE_H, r1 = min(g.h, r0 + UP_TILE_H);
        const S* xp = x + (size_t)plane * g.h * g.w;
        S* yp = y + (size_t)plane * g.h * g.w * 4;
        float a[3][NP + 2];                 // rows r-1, r, r+1
        up_x_row<DTYPE, NP>(xp, (int)r0 - 1, g, s0, a[0]);
        up_x_row<DTYPE, NP>(xp, (int)r0, g, s0, a[1]);
        for (uint32_t r = r0; r < r1; ++r) {
            up_x_row<DTYPE, NP>(xp, (int)r + 1, g, s0, a[2]);
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                float out[2 * NP];
#pragma unroll
                for (int p = 0; p < NP; ++p)
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx) {
                        const int i0 = p + dx;          // a[.][p + 1] is pixel p
                        float acc = b;
                        acc = __fmaf_rn(K[dy][dx][0][0], a[dy][i0], acc);
                        acc = __fmaf_rn(K[dy][dx][0][1], a[dy][i0 + 1], acc);
                        acc = __fmaf_rn(K[dy][dx][1][0], a[dy + 1][i0], acc);
                        acc = __fmaf_rn(K[dy][dx][1][1], a[dy + 1][i0 + 1], acc);
                        out[2 * p + dx] = acc;
                    }
                up_store<DTYPE, 2 * NP, (NP > 1)>(yp + (2 * r + dy) * (2 * g.w) + 2 * s0, out);
            }
#pragma unroll
            for (int j = 0; j < NP + 2; ++j) { a[0][j] = a[1][j]; a[1][j] = a[2][j]; }
        }
    }
}

// gy row Y of a plane (0 outside 0 .. 2h-1), columns 2*s0-1 .. 2*s0+2*NP (0 outside 0 .. 2w-1)
template <int DTYPE, int NP>
__device__ __forceinline__ void up_gy_row(const typename elem<DTYPE>::type* gp, int Y, const UpGeom& g,
                                          uint32_t s0, float* a)
{
    if (Y < 0 || Y >= (int)(2 * g.h)) {
#pragma unroll
        for (int j = 0; j < 2 * NP + 2; ++j) a[j] = 0.0f;
        return;
    }
    const typename elem<DTYPE>::type* p = gp + (uint32_t)Y * (2 * g.w) + 2 * s0;
    up_load<DTYPE, 2 * NP, (NP > 1)>(p, a + 1);
    a[0] = s0 > 0 ? ld<DTYPE>(p[-1]) : 0.0f;
    a[2 * NP + 1] = s0 + NP < g.w ? ld<DTYPE>(p[2 * NP]) : 0.0f;
}

template <int DTYPE, int NP>
__global__ __launch_bounds__(UP_THREADS) void k_up_bwd(
    const typename elem<DTYPE>::type* __restrict__ gy, const typename elem<DTYPE>::type* __restrict__ x,
    const float* __restrict__ weight, typename elem<DTYPE>::type* __restrict__ gx,
    float* __restrict__ partials, const UpGeom g)
{
    typedef typename elem<DTYPE>::type S;
    __shared__ float red[UP_THREADS / kWave][UP_PARTIAL];
    const bool rep = !g.zeropad;
    for (uint32_t item = blockIdx.x; item < g.items; item += gridDim.x) {
        const uint32_t plane = item / g.chunks, chunk = item - plane * g.chunks;
        const uint32_t unit = chunk * UP_THREADS + threadIdx.x;
        const uint32_t c = plane % g.C;
        float W[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) W[k] = weight[(size_t)c * 9 + k];
        float acc[UP_PARTIAL];
#pragma unroll
        for (int k = 0; k < UP_PARTIAL; ++k) acc[k] = 0.0f;
        if (unit < g.units) {
            const uint32_t tile = unit / g.G, s0 = (unit - tile * g.G) * NP;
            const uint32_t r0 = tile * UP_TILE_H, r1 = min(g.h, r0 + UP_TILE_H);
            const size_t base = (size_t)plane * g.h * g.w;
            const S* gp = gy + base * 4;
            float win[4][2 * NP + 2];       // gy rows 2r-1 .. 2r+2
            up_gy_row<DTYPE, NP>(gp, 2 * (int)r0 - 1, g, s0, win[0]);
            up_gy_row<DTYPE, NP>(gp, 2 * (int)r0, g, s0, win[1]);
            for (uint32_t r = r0; r < r1; ++r) {
                up_gy_row<DTYPE, NP>(gp, 2 * (int)r + 1, g, s0, win[2]);
                up_gy_row<DTYPE, NP>(gp, 2 * (int)r + 2, g, s0, win[3]);
                float xv[NP] = {}, out[NP];
                if (partials) up_load<DTYPE, NP, (NP > 1)>(x + base + r * g.w + s0, xv);
                const bool top = rep && r == 0, bottom = rep && r == g.h - 1;
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    // w % NP == 0 on the vector route: only the lane's first pixel can be column 0 and
                    // only its last one column w-1
                    const bool left = p == 0 && rep && s0 == 0, right = p == NP - 1 && rep && s0 + NP == g.w;
                    const int b0 = 2 * p;   // window column of gy column 2s-1
                    float cs[4][3];         // per window row: the column sets of taps j = 0, 1, 2
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        cs[a][0] = win[a][b0 + 2] + win[a][b0 + 3] + (left ? win[a][b0 + 1] : 0.0f);
                        cs[a][1] = win[a][b0 + 1] + win[a][b0 + 2];
                        cs[a][2] = win[a][b0] + win[a][b0 + 1] + (right ? win[a][b0 + 2] : 0.0f);
                    }
                    float gxv = 0.0f;
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const float P0 = cs[2][j] + cs[3][j] + (top ? cs[1][j] : 0.0f);
                        const float P1 = cs[1][j] + cs[2][j];
                        const float P2 = cs[0][j] + cs[1][j] + (bottom ? cs[2][j] : 0.0f);
                        gxv = __fmaf_rn(W[j], P0, gxv);
                        gxv = __fmaf_rn(W[3 + j], P1, gxv);
                        gxv = __fmaf_rn(W[6 + j], P2, gxv);
                        if (partials) {
                            acc[j] = __fmaf_rn(xv[p], P0, acc[j]);
                            acc[3 + j] = __fmaf_rn(xv[p], P1, acc[3 + j]);
                            acc[6 + j] = __fmaf_rn(xv[p], P2, acc[6 + j]);
                        }
                    }
                    if (partials && g.zeropad) {
                        // the zero-padded convolution multiplies the gy of an edge row / column by the padded
                        // zeros: nothing for a finite gy, NaN for a NaN or an infinity, as in torch's gweight.
                        // Every gy is multiplied on its own: a sum of large finite values first could overflow
                        const bool zt = r == 0, zb = r == g.h - 1, zl = s0 + p == 0, zr = s0 + p == g.w - 1;
                        if (zt || zb || zl || zr) {
                            const float z11 = __fmul_rn(0.0f, win[1][b0 + 1]), z12 = __fmul_rn(0.0f, win[1][b0 + 2]);
                            const float z21 = __fmul_rn(0.0f, win[2][b0 + 1]), z22 = __fmul_rn(0.0f, win[2][b0 + 2]);
                            float rowz[3] = {0.0f, 0.0f, 0.0f}, colz[3] = {0.0f, 0.0f, 0.0f};
                            if (zt) rowz[0] = z11 + z12;        // gy row 0 under the taps i = 0
                            if (zb) rowz[2] = z21 + z22;        // gy row 2h-1 under i = 2
                            if (zl) colz[0] = z11 + z21;        // gy column 0 under j = 0
                            if (zr) colz[2] = z12 + z22;        // gy column 2w-1 under j = 2
#pragma unroll
                            for (int i = 0; i < 3; ++i)
#pragma unroll
                                for (int j = 0; j < 3; ++j) acc[3 * i + j] += rowz[i] + colz[j];
                        }
                    }
                    out[p] = gxv;
                    acc[9] += (win[1][b0 + 1] + win[1][b0 + 2]) + (win[2][b0 + 1] + win[2][b0 + 2]);
                }
                if (gx) up_store<DTYPE, NP, (NP > 1)>(gx + base + r * g.w + s0, out);
#pragma unroll
                for (int j = 0; j < 2 * NP + 2; ++j) { win[0][j] = win[2][j]; win[1][j] = win[3][j]; }
            }
        }
        if (partials) {                     // the same for every lane of the grid
#pragma unroll
            for (int k = 0; k < UP_PARTIAL; ++k) acc[k] = wave_reduce_sum(acc[k]);
            if (lane_id() == 0) {
#pragma unroll
                for (int k = 0; k < UP_PARTIAL; ++k) red[threadIdx.x / kWave][k] = acc[k];
            }
            __syncthreads();
            if (threadIdx.x < UP_PARTIAL) {
                float s = red[0][threadIdx.x];
#pragma unroll
                for (int v = 1; v < UP_THREADS / kWave; ++v) s += red[v][threadIdx.x];
                partials[(size_t)item * UP_PARTIAL + threadIdx.x] = s;
            }
            __syncthreads();
        }
    }
}

// one wave per channel: entries (n, chunk) of the channel in ascending order, lane-strided, then
// the fixed shuffle tree
__global__ __launch_bounds__(UP_REDUCE_THREADS) void k_up_reduce(
    const float* __restrict__ partials, uint32_t B, uint32_t C, uint32_t chunks,
    float* __restrict__ gweight, float* __restrict__ gbias)
{
    const uint32_t c = blockIdx.x;
    float acc[UP_PARTIAL];
#pragma unroll
    for (int k = 0; k < UP_PARTIAL; ++k) acc[k] = 0.0f;
    const uint32_t entries = B * chunks;                           // <= items < 2^31
    for (uint32_t e = threadIdx.x; e < entries; e += UP_REDUCE_THREADS) {
        const uint32_t n = e / chunks, k2 = e - n * chunks;
        const float* p = partials + ((size_t)(n * C + c) * chunks + k2) * UP_PARTIAL;
#pragma unroll
        for (int k = 0; k < UP_PARTIAL; ++k) acc[k] += p[k];
    }
#pragma unroll
    for (int k = 0; k < UP_PARTIAL; ++k) acc[k] = wave_reduce_sum(acc[k]);
    if (threadIdx.x == 0) {
        if (gweight) {
#pragma unroll
            for (int k = 0; k < 9; ++k) gweight[(size_t)c * 9 + k] = acc[k];
        }
        if (gbias) gbias[c] = acc[9];
    }
}

int up_run(int dtype) { return dtype == NMSA_F32 ? 2 : 4; }

// sizes every entry point checks; NMSA_OK, NMSA_ERR_ARG or NMSA_ERR_UNSUPPORTED
int up_check_sizes(int dtype, int B, int C, int h, int w)
{
    if (dtype != NMSA_F32 && dtype != NMSA_BF16 && dtype != NMSA_F16) return NMSA_ERR_ARG;
    if (B < 1 || C < 1 || h < 1 || w < 1) return NMSA_ERR_ARG;
    if ((int64_t)h * w * 4 > 0x7fffffffLL) return NMSA_ERR_UNSUPPORTED;     // 32-bit offsets inside a plane
    if ((int64_t)B * C > 0x7fffffffLL) return NMSA_ERR_UNSUPPORTED;
    return NMSA_OK;
}

// work items of a call with NP pixels per lane; false when there are 2^31 or more
bool up_geometry(int B, int C, int h, int w, int NP, int zeropad, UpGeom& g)
{
    g.C = (uint32_t)C; g.h = (uint32_t)h; g.w = (uint32_t)w; g.zeropad = zeropad;
    g.G = (uint32_t)(w / NP);
    const uint64_t tiles = ((uint64_t)h + UP_TILE_H - 1) / UP_TILE_H;
    const uint64_t units = tiles * g.G;                               // <= h * w < 2^29
    const uint64_t chunks = (units + UP_THREADS - 1) / UP_THREADS;
    const uint64_t items = (uint64_t)B * C * chunks;
    if (items > 0x7fffffffull) return false;                  // item + gridDim.x stays below 2^32
    g.units = (uint32_t)units; g.chunks = (uint32_t)chunks; g.items = (uint32_t)items;
    return true;
}

// THE route rule: the vector route needs the lane run to divide the width and every tensor of
// the call on 16 bytes
bool up_vector(int dtype, int w, const void* a, const void* b, const void* c)
{
    return w % up_run(dtype) == 0 && aligned(a, 16) && aligned(b, 16) && aligned(c, 16);
}

}  // namespace
}  // namespace nmsa

extern "C" int nmsa_upsample2x_dw3x3_route(const void* x, const void* y_or_gx, int dtype,
                                           int B, int C, int h, int w)
{
    using namespace nmsa;
    const int rc = up_check_sizes(dtype, B, C, h, w);
    if (rc != NMSA_OK) return rc == NMSA_ERR_UNSUPPORTED ? rc : NMSA_ERR_ARG;
    const uintptr_t e = (uintptr_t)elem_bytes(dtype);
    if (!x || !y_or_gx || !aligned(x, e) || !aligned(y_or_gx, e)) return NMSA_ERR_ARG;
    return up_vector(dtype, w, x, y_or_gx, nullptr) ? NMSA_UP_ROUTE_VECTOR : NMSA_UP_ROUTE_PIXEL;
}

extern "C" int nmsa_upsample2x_dw3x3_fwd(const void* x, int dtype, const float* weight, const float* bias,
                                         int B, int C, int h, int w, int zeropad, void* y,
                                         nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = up_check_sizes(dtype, B, C, h, w);
    if (rc != NMSA_OK) return rc;
    const uintptr_t e = (uintptr_t)elem_bytes(dtype);
    if (!x || !weight || !y || (zeropad != 0 && zeropad != 1)) return NMSA_ERR_ARG;
    if (!aligned(x, e) || !aligned(y, e) || !aligned(weight, 4) || !aligned(bias, 4))
        return NMSA_ERR_ARG;
    const bool vec = up_vector(dtype, w, x, y, nullptr);
    UpGeom g;
    if (!up_geometry(B, C, h, w, vec ? up_run(dtype) : 1, zeropad, g)) return NMSA_ERR_UNSUPPORTED;
    const dim3 grid(capped_grid(g.items, UP_BLOCKS_PER_CU)), block(UP_THREADS);
#define UP_FWD(DT)                                                                                          \
    do {                                                                                                    \
        typedef elem<DT>::type S;                                                                           \
        if (vec) hipLaunchKernelGGL((k_up_fwd<DT, (DT == NMSA_F32 ? 2 : 4)>), grid, block, 0, stream,       \
                                    (const S*)x, weight, bias, (S*)y, g);                                   \
        else hipLaunchKernelGGL((k_up_fwd<DT, 1>), grid, block, 0, stream, (const S*)x, weight, bias,       \
                                (S*)y, g);                                                                  \
    } while (0)
    NMSA_DISPATCH_DTYPE(dtype, UP_FWD)
#undef UP_FWD
    return check_launch();
}

extern "C" size_t nmsa_upsample2x_dw3x3_bwd_workspace_bytes(int B, int C, int h, int w)
{
    using namespace nmsa;
    if (B < 1 || C < 1 || h < 1 || w < 1) return 0;
    // the one-pixel route has the most work items: one lane unit per pixel of a row tile
    const uint64_t tiles = ((uint64_t)h + UP_TILE_H - 1) / UP_TILE_H;
    const uint64_t chunks = (tiles * (uint64_t)w + UP_THREADS - 1) / UP_THREADS;
    return (size_t)((uint64_t)B * C * chunks * UP_PARTIAL * sizeof(float));
}

extern "C" int nmsa_upsample2x_dw3x3_bwd(const void* gy, const void* x, int dtype, const float* weight,
                                         int B, int C, int h, int w, int zeropad,
                                         void* gx, float* gweight, float* gbias,
                                         void* workspace, size_t workspace_bytes, nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = up_check_sizes(dtype, B, C, h, w);
    if (rc != NMSA_OK) return rc;
    const uintptr_t e = (uintptr_t)elem_bytes(dtype);
    if (!gy || !x || !weight || (zeropad != 0 && zeropad != 1)) return NMSA_ERR_ARG;
    if (!aligned(gy, e) || !aligned(x, e) || !aligned(gx, e) || !aligned(weight, 4) ||
        !aligned(gweight, 4) || !aligned(gbias, 4))
        return NMSA_ERR_ARG;
    const bool reduce = gweight || gbias;
    const bool vec = up_vector(dtype, w, gy, x, gx);
    UpGeom g;
    if (!up_geometry(B, C, h, w, vec ? up_run(dtype) : 1, zeropad, g)) return NMSA_ERR_UNSUPPORTED;
    if (reduce) {
        if (!workspace || !aligned(workspace, 16)) return NMSA_ERR_ARG;
        if (workspace_bytes < (size_t)g.items * UP_PARTIAL * sizeof(float)) return NMSA_ERR_WORKSPACE;
    }
    if (!gx && !reduce) return NMSA_OK;
    float* partials = reduce ? (float*)workspace : nullptr;
    const dim3 grid(capped_grid(g.items, UP_BLOCKS_PER_CU)), block(UP_THREADS);
#define UP_BWD(DT)                                                                                          \
    do {                                                                                                    \
        typedef elem<DT>::type S;                                                                           \
        if (vec) hipLaunchKernelGGL((k_up_bwd<DT, (DT == NMSA_F32 ? 2 : 4)>), grid, block, 0, stream,       \
                                    (const S*)gy, (const S*)x, weight, (S*)gx, partials, g);                \
        else hipLaunchKernelGGL((k_up_bwd<DT, 1>), grid, block, 0, stream, (const S*)gy, (const S*)x,       \
                                weight, (S*)gx, partials, g);                                               \
    } while (0)
    NMSA_DISPATCH_DTYPE(dtype, UP_BWD)
#undef UP_BWD
    if (int l = check_launch()) return l;
    if (reduce) {
        hipLaunchKernelGGL(k_up_reduce, dim3((unsigned)C), dim3(UP_REDUCE_THREADS), 0, stream,
                           (const float*)partials, (uint32_t)B, (uint32_t)C, g.chunks, gweight, gbias);
        return check_launch();
    }
    return NMSA_OK;
}
