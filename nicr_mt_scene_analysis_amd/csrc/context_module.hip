// context_module.hip — the hot path of the reference's context module (model/context_module/ppm.py,
// appm.py): all adaptive average pools of x in ONE launch, and the resize of every branch output
// together with the copy of x straight into the concatenated tensor in ONE launch; one launch each
// backward.  Up to NMSA_PPM_MAX_BINS branches per call; their sizes, channel counts and pointers
// are host arrays read at call time and carried in the kernel arguments (PpmDesc, by value).
//
//   pool_i[n,c,i,j] = ( sum_{h in rows(i)} ( sum_{w in cols(j)} x[n,c,h,w] ) ) / float(|rows| |cols|)
//                     rows(i) = floor(i H / ph) .. ceil((i+1) H / ph) - 1, cols(j) alike (ATen's windows)
//   gx[n,c,h,w]     = sum_i sum_{(a,b): h in rows(a), w in cols(b)} gp_i[n,c,a,b] / float(area(a,b))
//   out[n, 0..C)    = x;   out[n, C + off_i + c] = resize(y_i[n,c], H x W), nearest or bilinear
//                     (align_corners = False), ATen's float index arithmetic (nearest_src,
//                     bilinear_src and bilerp of crop_resize.hpp, shared with resize.hip)
//   gy_i[n,c,p,q]   = sum_{h reads p} wy(h,p) * ( sum_{w reads q} wx(w,q) * g_out[n, C+off_i+c, h, w] )
//
// Summation orders (fixed; no atomics; the same bits on every call and on both routes):
//   pool_fwd    a row's segment left to right (from 0), the row sums top to bottom (from 0), one division
//   pool_bwd    bins in order, cells row-major, one division per cell, added to a sum that starts at 0
//   upcat_bwd   a row's contributions left to right as fused multiply-adds from 0, the weighted row
//               sums top to bottom as fused multiply-adds from 0
//
// Work split.  The maps are small (15x20 .. 32x64) and there are B*C planes in the thousands:
//   k_ppm_pool_fwd, k_ppm_upcat_bwd   both reduce a plane to a few cells.  A WAVE owns a plane,
//       PPM_WAVES = 4 planes per workgroup.  LDS route: the wave stages its plane in LDS as float32
//       with coalesced loads (x / g_out are read from memory exactly once), then per branch the
//       lanes share the H * pw row segments (stage 1, into LDS) and then the ph * pw cells
//       (stage 2): the longest serial chain is one row or one column of the map, not a window.
//       GLOBAL route (a plane above PPM_LDS_PLANE elements or H * pw above PPM_LDS_ROWS): a lane
//       owns a cell and walks its window in memory in the same order — any size, the same bits.
//   k_ppm_pool_bwd   a lane owns a column of a plane and walks the rows (the row's cell range is
//       wave-uniform); for W < 64 a wave carries floor(64 / W) planes side by side.
//   k_ppm_upcat_fwd  the output is a flat stream: an item is 1024 consecutive pixels of one output
//       plane (a copy of x, or a branch), consecutive lanes store consecutive elements.
// Grids: min(items, PPM_BLOCKS_PER_CU workgroups per compute unit of nmsa_device_geometry), grid-stride;
// k_ppm_pool_bwd launches one item per wave instead (a grid-stride loop on top of its per-branch
// scalars does not fit the scalar registers, and an item is a walk over all H rows).
// Addressing: 64-bit plane bases, 32-bit offsets inside a plane (H, W, ph, pw <= 32768 is checked).
#include "crop_resize.hpp"

namespace nmsa {
namespace {

constexpr int PPM_THREADS = 256;
constexpr int PPM_WAVES = PPM_THREADS / kWave;
constexpr int PPM_BLOCKS_PER_CU = 8;
constexpr int PPM_LDS_PLANE = 2048;      // elements of a plane a wave stages (32 x 64)
constexpr int PPM_LDS_ROWS = 512;        // H * pw row sums of one branch
constexpr int PPM_CAT_RUN = 4;           // pixels per lane and item of k_ppm_upcat_fwd
constexpr int PPM_MAX_DIM = 32768;

// elem, ld, st: nmsa_common.hpp; nearest_src, bilinear_src, bilerp: crop_resize.hpp

struct PpmDesc {
    uint32_t C, H, W, HW;
    uint32_t n;                          // branches
    uint32_t planes;                     // planes the kernel walks
    uint32_t sum_cr, c_total;            // upcat: sum of cr, C + sum_cr
    int mode;
    int ph[NMSA_PPM_MAX_BINS], pw[NMSA_PPM_MAX_BINS], cr[NMSA_PPM_MAX_BINS];
    void* p[NMSA_PPM_MAX_BINS];
};

// branch `b` of the descriptor (b is uniform: three scalar selects, no indexed access to the arguments)
__device__ __forceinline__ void ppm_pick(const PpmDesc& d, int b, int& ph, int& pw, void*& p)
{
    ph = d.ph[0]; pw = d.pw[0]; p = d.p[0];
#pragma unroll
    for (int k = 1; k < NMSA_PPM_MAX_BINS; ++k)
        if (b == k) { ph = d.ph[k]; pw = d.pw[k]; p = d.p[k]; }
}

// first / one-past-last index of ATen's adaptive window `i` of `out` over `in`
__device__ __forceinline__ int ppm_win_lo(int i, int in, int out) { return (i * in) / out; }
__device__ __forceinline__ int ppm_win_hi(int i, int in, int out) { return ((i + 1) * in + out - 1) / out; }

// the weight with which output index `dst` reads source cell `cell` (false: it does not read it)
__device__ __forceinline__ bool ppm_reads(int mode, float scale, int dst, int in, int cell, float& wgt)
{
    if (mode == NMSA_PPM_NEAREST) {
        wgt = 1.0f;
        return nearest_src(scale, dst, in) == cell;
    }
    int i0, i1;
    float w0, w1;
    bilinear_src(scale, dst, in, i0, i1, w0, w1);
    wgt = __fadd_rn(i0 == cell ? w0 : 0.0f, i1 == cell ? w1 : 0.0f);
    return i0 == cell || i1 == cell;
}

// a range of output indices that holds every one that reads `cell` (members are tested exactly)
__device__ __forceinline__ void ppm_readers(int mode, float scale, int out, int cell, int& lo, int& hi)
{
    const float inv = 1.0f / scale;
    float a, b;
    if (mode == NMSA_PPM_NEAREST) {
        a = (float)cell * inv;
        b = (float)(cell + 1) * inv;
    } else {
        a = ((float)cell - 0.5f) * inv - 0.5f;
        b = ((float)cell + 1.5f) * inv - 0.5f;
    }
    a = fminf(fmaxf(a - 2.0f, 0.0f), (float)(out - 1));
    b = fminf(fmaxf(b + 2.0f, 0.0f), (float)(out - 1));
    lo = (int)floorf(a);
    hi = (int)ceilf(b);
}

// ---------------------------------------------------------------------------------- pool forward
template <int DTYPE, bool LDS>
__global__ __launch_bounds__(PPM_THREADS) void k_ppm_pool_fwd(
    const typename elem<DTYPE>::type* __restrict__ x, const PpmDesc d)
{
    typedef typename elem<DTYPE>::type S;
    __shared__ float s_plane[LDS ? PPM_WAVES * PPM_LDS_PLANE : 1];
    __shared__ float s_rows[LDS ? PPM_WAVES * PPM_LDS_ROWS : 1];
    const int wave = threadIdx.x / kWave, lane = lane_id();
    const int H = (int)d.H, W = (int)d.W;
    const uint32_t stride = gridDim.x * PPM_WAVES;
    const uint32_t iters = (d.planes + stride - 1) / stride;
    for (uint32_t it = 0; it < iters; ++it) {
        const uint32_t plane = it * stride + blockIdx.x * PPM_WAVES + wave;
        const bool valid = plane < d.planes;
        const S* xp = x + (size_t)plane * d.HW;
        if constexpr (LDS) {
            float* pl = s_plane + wave * PPM_LDS_PLANE;
            if (valid)
                for (uint32_t i = lane; i < d.HW; i += kWave) pl[i] = ld<DTYPE>(xp[i]);
            __syncthreads();
        }
#pragma nounroll
        for (int b = 0; b < (int)d.n; ++b) {
            int ph, pw;
            void* base;
            ppm_pick(d, b, ph, pw, base);
            S* op = (S*)base + (size_t)plane * (uint32_t)(ph * pw);
            if constexpr (LDS) {
                const float* pl = s_plane + wave * PPM_LDS_PLANE;
                float* rows = s_rows + wave * PPM_LDS_ROWS;
                if (valid)
                    for (int idx = lane; idx < H * pw; idx += kWave) {
                        const int h = idx / pw, j = idx - h * pw;
                        const int w0 = ppm_win_lo(j, W, pw), w1 = ppm_win_hi(j, W, pw);
                        float r = 0.0f;
                        for (int w = w0; w < w1; ++w) r = __fadd_rn(r, pl[h * W + w]);
                        rows[idx] = r;
                    }
                __syncthreads();
                if (valid)
                    for (int cell = lane; cell < ph * pw; cell += kWave) {
                        const int i = cell / pw, j = cell - i * pw;
                        const int h0 = ppm_win_lo(i, H, ph), h1 = ppm_win_hi(i, H, ph);
                        const int kw = ppm_win_hi(j, W, pw) - ppm_win_lo(j, W, pw);
                        float s = 0.0f;
                        for (int h = h0; h < h1; ++h) s = __fadd_rn(s, rows[h * pw + j]);
                        op[cell] = st<DTYPE>(__fdiv_rn(s, (float)((h1 - h0) * kw)));
                    }
                __syncthreads();
            } else {
                if (valid)
                    for (int cell = lane; cell < ph * pw; cell += kWave) {
                        const int i = cell / pw, j = cell - i * pw;
                        const int h0 = ppm_win_lo(i, H, ph), h1 = ppm_win_hi(i, H, ph);
                        const int w0 = ppm_win_lo(j, W, pw), w1 = ppm_win_hi(j, W, pw);
                        float s = 0.0f;
                        for (int h = h0; h < h1; ++h) {
                            float r = 0.0f;
                            for (int w = w0; w < w1; ++w) r = __fadd_rn(r, ld<DTYPE>(xp[h * W + w]));
                            s = __fadd_rn(s, r);
                        }
                        op[cell] = st<DTYPE>(__fdiv_rn(s, (float)((h1 - h0) * (w1 - w0))));
                    }
            }
        }
    }
}

// --------------------------------------------------------------------------------- pool backward
template <int DTYPE>
__global__ __launch_bounds__(PPM_THREADS) void k_ppm_pool_bwd(
    typename elem<DTYPE>::type* __restrict__ gx, const PpmDesc d, const uint32_t side,
    const uint32_t chunks, const uint32_t items)
{
    typedef typename elem<DTYPE>::type S;
    __shared__ int s_j0[NMSA_PPM_MAX_BINS][PPM_THREADS], s_j1[NMSA_PPM_MAX_BINS][PPM_THREADS];
    __shared__ int s_kw0[NMSA_PPM_MAX_BINS][PPM_THREADS], s_kw1[NMSA_PPM_MAX_BINS][PPM_THREADS];
    const int wave = threadIdx.x / kWave, lane = lane_id();
    const int H = (int)d.H, W = (int)d.W;
    const uint32_t cols = min(d.W, (uint32_t)kWave);       // lanes a plane's row takes
    const uint32_t sub = (uint32_t)lane / cols, wl = (uint32_t)lane - sub * cols;
    // one item per wave: the walk over H rows is long enough, and a grid-stride loop on top of the
    // per-branch scalars does not fit the scalar registers
    {
        const uint32_t item = blockIdx.x * PPM_WAVES + wave;
        const uint32_t group = item / chunks, chunk = item - group * chunks;
        const uint32_t plane = group * side + sub;
        const int w = (int)(chunk * kWave + wl);
        if (item >= items || sub >= side || plane >= d.planes || w >= W) return;
        // first / last column cell over w and their window lengths, per branch: the lane's own slots
        // (nobody else reads them)
#pragma nounroll
        for (int b = 0; b < (int)d.n; ++b) {
            int ph, pw;
            void* base;
            ppm_pick(d, b, ph, pw, base);
            const int j0 = (w * pw) / W, j1 = ((w + 1) * pw - 1) / W;
            s_j0[b][threadIdx.x] = j0;
            s_j1[b][threadIdx.x] = base ? j1 : -1;
            s_kw0[b][threadIdx.x] = ppm_win_hi(j0, W, pw) - ppm_win_lo(j0, W, pw);
            s_kw1[b][threadIdx.x] = ppm_win_hi(j1, W, pw) - ppm_win_lo(j1, W, pw);
        }
        S* gp = gx + (size_t)plane * d.HW;
        for (int h = 0; h < H; ++h) {
            float acc = 0.0f;
#pragma nounroll
            for (int b = 0; b < (int)d.n; ++b) {
                int ph, pw;
                void* base;
                ppm_pick(d, b, ph, pw, base);
                const int j0 = s_j0[b][threadIdx.x], j1 = s_j1[b][threadIdx.x];
                const int kw0 = s_kw0[b][threadIdx.x], kw1 = s_kw1[b][threadIdx.x];
                const S* src = (const S*)base + (size_t)plane * (uint32_t)(ph * pw);
                const int i0 = (h * ph) / H, i1 = ((h + 1) * ph - 1) / H;
                for (int i = i0; i <= i1; ++i) {
                    const int kh = ppm_win_hi(i, H, ph) - ppm_win_lo(i, H, ph);
                    for (int j = j0; j <= j1; ++j) {
                        const int kw = j == j0 ? kw0 : (j == j1 ? kw1 : ppm_win_hi(j, W, pw) - ppm_win_lo(j, W, pw));
                        acc = __fadd_rn(acc, __fdiv_rn(ld<DTYPE>(src[i * pw + j]), (float)(kh * kw)));
                    }
                }
            }
            gp[h * W + w] = st<DTYPE>(acc);
        }
    }
}

// ------------------------------------------------------------------- upsample + concat forward
template <int DTYPE>
__global__ __launch_bounds__(PPM_THREADS) void k_ppm_upcat_fwd(
    const typename elem<DTYPE>::type* __restrict__ x, typename elem<DTYPE>::type* __restrict__ out,
    const PpmDesc d, const uint32_t chunks, const uint32_t items)
{
    typedef typename elem<DTYPE>::type S;
    const int H = (int)d.H, W = (int)d.W;
    for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t plane = item / chunks, chunk = item - plane * chunks;
        const uint32_t n = plane / d.c_total, ch = plane - n * d.c_total;
        S* op = out + (size_t)plane * d.HW;
        const uint32_t base = chunk * (PPM_THREADS * PPM_CAT_RUN) + threadIdx.x;
        if (ch < d.C) {                                     // the copy of x: the elements as they are
            const S* xp = x + ((size_t)n * d.C + ch) * d.HW;
#pragma unroll
            for (int k = 0; k < PPM_CAT_RUN; ++k) {
                const uint32_t i = base + k * PPM_THREADS;
                if (i < d.HW) op[i] = xp[i];
            }
            continue;
        }
        uint32_t c = ch - d.C;
        int ph = 1, pw = 1;
        const S* src = nullptr;
        bool found = false;
#pragma unroll
        for (int b = 0; b < NMSA_PPM_MAX_BINS; ++b) {
            if (b < (int)d.n && !found) {
                if (c < (uint32_t)d.cr[b]) {
                    ph = d.ph[b]; pw = d.pw[b];
                    src = (const S*)d.p[b] + ((size_t)n * (uint32_t)d.cr[b] + c) * (uint32_t)(ph * pw);
                    found = true;
                } else {
                    c -= (uint32_t)d.cr[b];
                }
            }
        }
        const float sy = (float)ph / (float)H, sx = (float)pw / (float)W;   // ATen compute_scales_value
#pragma unroll
        for (int k = 0; k < PPM_CAT_RUN; ++k) {
            const uint32_t i = base + k * PPM_THREADS;
            if (i >= d.HW) continue;
            const int h = (int)(i / d.W), w = (int)(i - (uint32_t)h * d.W);
            float v;
            if (d.mode == NMSA_PPM_NEAREST) {
                v = ld<DTYPE>(src[nearest_src(sy, h, ph) * pw + nearest_src(sx, w, pw)]);
            } else {
                int iy0, iy1, ix0, ix1;
                float wy0, wy1, wx0, wx1;
                bilinear_src(sy, h, ph, iy0, iy1, wy0, wy1);
                bilinear_src(sx, w, pw, ix0, ix1, wx0, wx1);
                v = bilerp(ld<DTYPE>(src[iy0 * pw + ix0]), ld<DTYPE>(src[iy0 * pw + ix1]),
                           ld<DTYPE>(src[iy1 * pw + ix0]), ld<DTYPE>(src[iy1 * pw + ix1]),
                           wx0, wx1, wy0, wy1);
            }
            op[i] = st<DTYPE>(v);
        }
    }
}

// ------------------------------------------------------------------ upsample + concat backward
template <int DTYPE, bool LDS>
__global__ __launch_bounds__(PPM_THREADS) void k_ppm_upcat_bwd(
    const typename elem<DTYPE>::type* __restrict__ g_out, const PpmDesc d)
{
    typedef typename elem<DTYPE>::type S;
    __shared__ float s_plane[LDS ? PPM_WAVES * PPM_LDS_PLANE : 1];
    __shared__ float s_rows[LDS ? PPM_WAVES * PPM_LDS_ROWS : 1];
    const int wave = threadIdx.x / kWave, lane = lane_id();
    const int H = (int)d.H, W = (int)d.W;
    const uint32_t stride = gridDim.x * PPM_WAVES;
    const uint32_t iters = (d.planes + stride - 1) / stride;
    for (uint32_t it = 0; it < iters; ++it) {
        const uint32_t plane = it * stride + blockIdx.x * PPM_WAVES + wave;     // over B * sum_cr
        const uint32_t n = plane / d.sum_cr;
        uint32_t c = plane - n * d.sum_cr;
        int ph = 1, pw = 1;
        S* dst = nullptr;
        bool found = false;
#pragma unroll
        for (int b = 0; b < NMSA_PPM_MAX_BINS; ++b) {
            if (b < (int)d.n && !found) {
                if (c < (uint32_t)d.cr[b]) {
                    ph = d.ph[b]; pw = d.pw[b];
                    if (d.p[b]) dst = (S*)d.p[b] + ((size_t)n * (uint32_t)d.cr[b] + c) * (uint32_t)(ph * pw);
                    found = true;
                } else {
                    c -= (uint32_t)d.cr[b];
                }
            }
        }
        const bool valid = plane < d.planes && dst != nullptr;
        const S* gp = g_out + ((size_t)n * d.c_total + d.C + (plane - n * d.sum_cr)) * d.HW;
        const float sy = (float)ph / (float)H, sx = (float)pw / (float)W;
        if constexpr (LDS) {
            float* pl = s_plane + wave * PPM_LDS_PLANE;
            float* rows = s_rows + wave * PPM_LDS_ROWS;
            if (valid)
                for (uint32_t i = lane; i < d.HW; i += kWave) pl[i] = ld<DTYPE>(gp[i]);
            __syncthreads();
            if (valid)
                for (int idx = lane; idx < H * pw; idx += kWave) {
                    const int h = idx / pw, q = idx - h * pw;
                    int w0, w1;
                    ppm_readers(d.mode, sx, W, q, w0, w1);
                    float r = 0.0f;
                    for (int w = w0; w <= w1; ++w) {
                        float wx;
                        if (ppm_reads(d.mode, sx, w, pw, q, wx)) r = __fmaf_rn(pl[h * W + w], wx, r);
                    }
                    rows[idx] = r;
                }
            __syncthreads();
            if (valid)
                for (int cell = lane; cell < ph * pw; cell += kWave) {
                    const int p = cell / pw, q = cell - p * pw;
                    int h0, h1;
                    ppm_readers(d.mode, sy, H, p, h0, h1);
                    float s = 0.0f;
                    for (int h = h0; h <= h1; ++h) {
                        float wy;
                        if (ppm_reads(d.mode, sy, h, ph, p, wy)) s = __fmaf_rn(rows[h * pw + q], wy, s);
                    }
                    dst[cell] = st<DTYPE>(s);
                }
            __syncthreads();
        } else {
            if (valid)
                for (int cell = lane; cell < ph * pw; cell += kWave) {
                    const int p = cell / pw, q = cell - p * pw;
                    int h0, h1, w0, w1;
                    ppm_readers(d.mode, sy, H, p, h0, h1);
                    ppm_readers(d.mode, sx, W, q, w0, w1);
                    float s = 0.0f;
                    for (int h = h0; h <= h1; ++h) {
                        float wy;
                        if (!ppm_reads(d.mode, sy, h, ph, p, wy)) continue;
                        float r = 0.0f;
                        for (int w = w0; w <= w1; ++w) {
                            float wx;
                            if (ppm_reads(d.mode, sx, w, pw, q, wx))
                                r = __fmaf_rn(ld<DTYPE>(gp[h * W + w]), wx, r);
                        }
                        s = __fmaf_rn(r, wy, s);
                    }
                    dst[cell] = st<DTYPE>(s);
                }
        }
    }
}

// ------------------------------------------------------------------------------------ host side
// sizes every entry point checks; NMSA_OK, NMSA_ERR_ARG or NMSA_ERR_UNSUPPORTED
int ppm_check_sizes(int dtype, int B, int C, int H, int W, int n_bins, const int* ph, const int* pw)
{
    if (dtype != NMSA_F32 && dtype != NMSA_BF16 && dtype != NMSA_F16) return NMSA_ERR_ARG;
    if (B < 1 || C < 1 || H < 1 || W < 1) return NMSA_ERR_ARG;
    if (n_bins < 1 || n_bins > NMSA_PPM_MAX_BINS || !ph || !pw) return NMSA_ERR_ARG;
    for (int i = 0; i < n_bins; ++i)
        if (ph[i] < 1 || pw[i] < 1) return NMSA_ERR_ARG;
    if (H > PPM_MAX_DIM || W > PPM_MAX_DIM) return NMSA_ERR_UNSUPPORTED;    // 32-bit offsets and index products
    for (int i = 0; i < n_bins; ++i)
        if (ph[i] > PPM_MAX_DIM || pw[i] > PPM_MAX_DIM) return NMSA_ERR_UNSUPPORTED;
    if ((int64_t)B * C > 0x7fffffffLL) return NMSA_ERR_UNSUPPORTED;
    return NMSA_OK;
}

// THE route rule of the two plane-reducing kernels
bool ppm_lds(int H, int W, int n_bins, const int* pw)
{
    if ((int64_t)H * W > PPM_LDS_PLANE) return false;
    for (int i = 0; i < n_bins; ++i)
        if ((int64_t)H * pw[i] > PPM_LDS_ROWS) return false;
    return true;
}

void ppm_desc(PpmDesc& d, int C, int H, int W, int n_bins, const int* ph, const int* pw, const int* cr,
              void* const* p, int mode)
{
    d.C = (uint32_t)C; d.H = (uint32_t)H; d.W = (uint32_t)W; d.HW = (uint32_t)(H * W);
    d.n = (uint32_t)n_bins; d.planes = 0; d.sum_cr = 0; d.c_total = 0; d.mode = mode;
    for (int i = 0; i < NMSA_PPM_MAX_BINS; ++i) {
        const bool on = i < n_bins;
        d.ph[i] = on ? ph[i] : 1; d.pw[i] = on ? pw[i] : 1; d.cr[i] = on && cr ? cr[i] : 0;
        d.p[i] = on ? p[i] : nullptr;
    }
}

// channel counts of an upcat call: NMSA_OK with the sum in `sum_cr`, or the error
int ppm_check_channels(int B, int C, int n_bins, const int* cr, int64_t& sum_cr)
{
    if (!cr) return NMSA_ERR_ARG;
    sum_cr = 0;
    for (int i = 0; i < n_bins; ++i) {
        if (cr[i] < 1) return NMSA_ERR_ARG;
        sum_cr += cr[i];
    }
    if ((int64_t)B * (C + sum_cr) > 0x7fffffffLL) return NMSA_ERR_UNSUPPORTED;
    return NMSA_OK;
}

}  // namespace
}  // namespace nmsa

extern "C" int nmsa_ppm_route(int H, int W, int n_bins, const int* ph, const int* pw)
{
    using namespace nmsa;
    const int rc = ppm_check_sizes(NMSA_F32, 1, 1, H, W, n_bins, ph, pw);
    if (rc != NMSA_OK) return rc;
    return ppm_lds(H, W, n_bins, pw) ? NMSA_PPM_ROUTE_LDS : NMSA_PPM_ROUTE_GLOBAL;
}

extern "C" int nmsa_ppm_pool_fwd(const void* x, int dtype, int B, int C, int H, int W, int n_bins,
                                 const int* ph, const int* pw, void* const* pooled, nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = ppm_check_sizes(dtype, B, C, H, W, n_bins, ph, pw);
    if (rc != NMSA_OK) return rc;
    if (!x || !pooled || !elem_aligned(x, dtype)) return NMSA_ERR_ARG;
    for (int i = 0; i < n_bins; ++i)
        if (!pooled[i] || !elem_aligned(pooled[i], dtype)) return NMSA_ERR_ARG;
    PpmDesc d;
    ppm_desc(d, C, H, W, n_bins, ph, pw, nullptr, pooled, 0);
    d.planes = (uint32_t)(B * C);
    const bool lds = ppm_lds(H, W, n_bins, pw);
    const dim3 grid(capped_grid(((uint64_t)d.planes + PPM_WAVES - 1) / PPM_WAVES, PPM_BLOCKS_PER_CU)), block(PPM_THREADS);
#define PPM_POOL_FWD(DT)                                                                                    \
    do {                                                                                                    \
        typedef elem<DT>::type S;                                                                           \
        if (lds) hipLaunchKernelGGL((k_ppm_pool_fwd<DT, true>), grid, block, 0, stream, (const S*)x, d);    \
        else hipLaunchKernelGGL((k_ppm_pool_fwd<DT, false>), grid, block, 0, stream, (const S*)x, d);       \
    } while (0)
    NMSA_DISPATCH_DTYPE(dtype, PPM_POOL_FWD)
#undef PPM_POOL_FWD
    return check_launch();
}

extern "C" int nmsa_ppm_pool_bwd(const void* const* gp, int dtype, int B, int C, int H, int W, int n_bins,
                                 const int* ph, const int* pw, void* gx, nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = ppm_check_sizes(dtype, B, C, H, W, n_bins, ph, pw);
    if (rc != NMSA_OK) return rc;
    if (!gp || !gx || !elem_aligned(gx, dtype)) return NMSA_ERR_ARG;
    for (int i = 0; i < n_bins; ++i)
        if (!elem_aligned(gp[i], dtype)) return NMSA_ERR_ARG;      // NULL: that branch adds nothing
    PpmDesc d;
    ppm_desc(d, C, H, W, n_bins, ph, pw, nullptr, (void* const*)gp, 0);
    d.planes = (uint32_t)(B * C);
    const uint32_t side = W < kWave ? (uint32_t)(kWave / W) : 1u;          // planes a wave carries
    const uint32_t chunks = (uint32_t)((W + kWave - 1) / kWave);
    const uint64_t items = ((uint64_t)d.planes + side - 1) / side * chunks;
    if (items > 0x7fffffffull) return NMSA_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((items + PPM_WAVES - 1) / PPM_WAVES)), block(PPM_THREADS);
#define PPM_POOL_BWD(DT)                                                                                    \
    hipLaunchKernelGGL((k_ppm_pool_bwd<DT>), grid, block, 0, stream, (elem<DT>::type*)gx, d, side,          \
                       chunks, (uint32_t)items)
    NMSA_DISPATCH_DTYPE(dtype, PPM_POOL_BWD)
#undef PPM_POOL_BWD
    return check_launch();
}

extern "C" int nmsa_ppm_upcat_fwd(const void* x, const void* const* ys, int dtype, int B, int C, int H, int W,
                                  int n_bins, const int* cr, const int* ph, const int* pw, int mode,
                                  void* out, nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = ppm_check_sizes(dtype, B, C, H, W, n_bins, ph, pw);
    if (rc != NMSA_OK) return rc;
    if (mode != NMSA_PPM_NEAREST && mode != NMSA_PPM_BILINEAR) return NMSA_ERR_ARG;
    int64_t sum_cr = 0;
    if (int e = ppm_check_channels(B, C, n_bins, cr, sum_cr)) return e;
    if (!x || !ys || !out || !elem_aligned(x, dtype) || !elem_aligned(out, dtype)) return NMSA_ERR_ARG;
    for (int i = 0; i < n_bins; ++i)
        if (!ys[i] || !elem_aligned(ys[i], dtype)) return NMSA_ERR_ARG;
    PpmDesc d;
    ppm_desc(d, C, H, W, n_bins, ph, pw, cr, (void* const*)ys, mode);
    d.sum_cr = (uint32_t)sum_cr; d.c_total = (uint32_t)(C + sum_cr);
    d.planes = (uint32_t)(B * (C + sum_cr));
    const uint32_t run = PPM_THREADS * PPM_CAT_RUN;
    const uint32_t chunks = (d.HW + run - 1) / run;
    const uint64_t items = (uint64_t)d.planes * chunks;
    if (items > 0x7fffffffull) return NMSA_ERR_UNSUPPORTED;
    const dim3 grid(capped_grid(items, PPM_BLOCKS_PER_CU)), block(PPM_THREADS);
#define PPM_UPCAT_FWD(DT)                                                                                   \
    hipLaunchKernelGGL((k_ppm_upcat_fwd<DT>), grid, block, 0, stream, (const elem<DT>::type*)x,             \
                       (elem<DT>::type*)out, d, chunks, (uint32_t)items)
    NMSA_DISPATCH_DTYPE(dtype, PPM_UPCAT_FWD)
#undef PPM_UPCAT_FWD
    return check_launch();
}

extern "C" int nmsa_ppm_upcat_bwd(const void* g_out, int dtype, int B, int C, int H, int W, int n_bins,
                                  const int* cr, const int* ph, const int* pw, int mode, void* const* gys,
                                  nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = ppm_check_sizes(dtype, B, C, H, W, n_bins, ph, pw);
    if (rc != NMSA_OK) return rc;
    if (mode != NMSA_PPM_NEAREST && mode != NMSA_PPM_BILINEAR) return NMSA_ERR_ARG;
    int64_t sum_cr = 0;
    if (int e = ppm_check_channels(B, C, n_bins, cr, sum_cr)) return e;
    if (!g_out || !gys || !elem_aligned(g_out, dtype)) return NMSA_ERR_ARG;
    bool any = false;
    for (int i = 0; i < n_bins; ++i) {
        if (!elem_aligned(gys[i], dtype)) return NMSA_ERR_ARG;    // NULL: that gradient is not wanted
        any = any || gys[i];
    }
    if (!any) return NMSA_OK;
    PpmDesc d;
    ppm_desc(d, C, H, W, n_bins, ph, pw, cr, gys, mode);
    d.sum_cr = (uint32_t)sum_cr; d.c_total = (uint32_t)(C + sum_cr);
    d.planes = (uint32_t)(B * sum_cr);
    const bool lds = ppm_lds(H, W, n_bins, pw);
    const dim3 grid(capped_grid(((uint64_t)d.planes + PPM_WAVES - 1) / PPM_WAVES, PPM_BLOCKS_PER_CU)), block(PPM_THREADS);
#define PPM_UPCAT_BWD(DT)                                                                                   \
    do {                                                                                                    \
        typedef elem<DT>::type S;                                                                           \
        if (lds) hipLaunchKernelGGL((k_ppm_upcat_bwd<DT, true>), grid, block, 0, stream, (const S*)g_out, d); \
        else hipLaunchKernelGGL((k_ppm_upcat_bwd<DT, false>), grid, block, 0, stream, (const S*)g_out, d);  \
    } while (0)
    NMSA_DISPATCH_DTYPE(dtype, PPM_UPCAT_BWD)
#undef PPM_UPCAT_BWD
    return check_launch();
}
