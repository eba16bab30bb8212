// mlp_decoder.hip — the hot step of the reference's MLP decoders (model/decoder/mlp_base.py): every
// embedded branch map resized to the 1/4-resolution grid and written straight into the concatenated
// tensor in front of the `fuse` convolution in ONE launch; ONE launch backward.  Up to
// NMSA_MLPDEC_MAX_BRANCHES branches per call; their channel counts, shifts and pointers are host
// arrays read at call time and carried in the kernel arguments (MldDesc, by value).
//
//   out[b, off_i + c, Y, X] = resize(y_i[b, c], H x W)     off_i = c_0 + ... + c_(i-1)
//   y_i [B, c_i, H >> s_i, W >> s_i], factor f_i = 1 << s_i; nearest or bilinear (align_corners = False)
//   gy_i[b, c, p, q] = sum_{Y reads p} wy(Y, p) * ( sum_{X reads q} wx(X, q) * g_out[b, off_i + c, Y, X] )
//
// The arithmetic is that of nmsa_ppm_upcat_fwd / _bwd (context_module.hip), through the same
// nearest_src, bilinear_src and bilerp of crop_resize.hpp: ATen's float index arithmetic with
// scale = float(h) / float(H) (1 / f, exact), the blend
// (a*wx0 + b*wx1)*wy0 + (c*wx0 + d*wx1)*wy1 with one fused multiply-add per sum; backward a row's
// contributions left to right as fused multiply-adds from 0, the weighted row sums top to bottom as
// fused multiply-adds from 0.  A branch with s_i == 0 is copied element for element.  No atomics, no
// workspace: every call and both forward routes give the same bits.
//
// Work split.  The maps are large (120x160 and up) and the kernel is bound by its stores:
//   k_mlpdec_upcat_fwd   the output is a flat stream.  An item is MLD_THREADS * VEC consecutive pixels
//       of one output plane; a lane produces VEC consecutive pixels of one row and stores them at once.
//       VECTOR route (VEC = 4 float32 / 8 half): 16 bytes per lane; needs W % VEC == 0 and every
//       tensor on 16 bytes, so no vector crosses a row and every plane starts on 16 bytes.  The
//       s_i == 0 branch moves 16-byte vectors both ways.  ELEMENT route (VEC = 1): any width, any
//       element-aligned pointer.  Source reads are element-wise on both routes and repeat out of the
//       cache (a source pixel is read by up to 2f x 2f outputs).
//   k_mlpdec_upcat_bwd   gather form.  A lane owns one source pixel and walks its footprint in g_out
//       (at most 2f x 2f pixels bilinear, f x f nearest); an item is MLD_THREADS consecutive source
//       pixels of one branch's flat [B * c_i * h_i * w_i] array, the branches in order (the largest
//       factor, whose lanes walk longest, first).  The up-to-four reads of every g_out element come
//       out of the cache; there is no LDS staging.  A branch with a NULL gy_i has no items.
// Grids: min(items, MLD_BLOCKS_PER_CU workgroups per compute unit of nmsa_device_geometry), grid-stride.
// Addressing: 64-bit plane bases, 32-bit offsets inside a plane (H, W <= 32768 is checked).
#include "crop_resize.hpp"

namespace nmsa {
namespace {

constexpr int MLD_THREADS = 256;
constexpr int MLD_BLOCKS_PER_CU = 8;
constexpr int MLD_MAX_DIM = 32768;
constexpr int MLD_MAX_SHIFT = 4;

// elem, ld, st, pack: nmsa_common.hpp; nearest_src, bilinear_src, bilerp: crop_resize.hpp

struct MldDesc {
    uint32_t B, H, W, HW;
    uint32_t n;                                  // branches
    uint32_t c_total;                            // sum of c
    int mode;
    uint32_t c[NMSA_MLPDEC_MAX_BRANCHES], s[NMSA_MLPDEC_MAX_BRANCHES];
    uint32_t off[NMSA_MLPDEC_MAX_BRANCHES];      // first output channel of the branch
    uint32_t first[NMSA_MLPDEC_MAX_BRANCHES];    // bwd: first item of the branch
    void* p[NMSA_MLPDEC_MAX_BRANCHES];
};

// the weight with which output index `dst` reads source cell `cell` (false: it does not read it)
__device__ __forceinline__ bool mld_reads(int mode, float scale, int dst, int in, int cell, float& wgt)
{
    if (mode == NMSA_MLPDEC_NEAREST) {
        wgt = 1.0f;
        return nearest_src(scale, dst, in) == cell;
    }
    int i0, i1;
    float w0, w1;
    bilinear_src(scale, dst, in, i0, i1, w0, w1);
    wgt = __fadd_rn(i0 == cell ? w0 : 0.0f, i1 == cell ? w1 : 0.0f);
    return i0 == cell || i1 == cell;
}

// a range of output indices that holds every one that reads `cell` at factor f = 1 << sh (members are
// tested exactly): nearest f*cell .. f*cell + f - 1; bilinear i0 == cell for f*cell + f/2 ..
// f*cell + 3f/2 - 1 and i1 == cell for the f indices below; cell 1 is also the i1 of the f/2 indices at the border
// whose source clamps to 0 (weight 0: nothing for a finite gradient, NaN for a NaN or an infinity, as ATen's
// backward gives); the border clamps stay inside [0, out)
__device__ __forceinline__ void mld_readers(int mode, int sh, int out, int cell, int& lo, int& hi)
{
    const int f = 1 << sh, a = cell << sh;
    if (mode == NMSA_MLPDEC_NEAREST) {
        lo = a;
        hi = a + f - 1;
    } else {
        lo = cell == 1 ? 0 : max(a - (f >> 1), 0);
        hi = min(a + f + (f >> 1) - 1, out - 1);
    }
}

// ------------------------------------------------------------------- upsample + concat forward
template <int DTYPE, int VEC>
__global__ __launch_bounds__(MLD_THREADS) void k_mlpdec_upcat_fwd(
    typename elem<DTYPE>::type* __restrict__ out, const MldDesc d, const uint32_t chunks, const uint32_t items)
{
    typedef typename elem<DTYPE>::type S;
    typedef pack<S, VEC> P;
    const int H = (int)d.H, W = (int)d.W;
    for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t plane = item / chunks, chunk = item - plane * chunks;
        const uint32_t n = plane / d.c_total;
        uint32_t c = plane - n * d.c_total;
        uint32_t cb = 1, sh = 0;
        const S* base = nullptr;
        bool found = false;
#pragma unroll
        for (int b = 0; b < NMSA_MLPDEC_MAX_BRANCHES; ++b) {
            if (b < (int)d.n && !found) {
                if (c < d.c[b]) {
                    cb = d.c[b]; sh = d.s[b]; base = (const S*)d.p[b];
                    found = true;
                } else {
                    c -= d.c[b];
                }
            }
        }
        const uint32_t i = (chunk * MLD_THREADS + threadIdx.x) * VEC;     // HW % VEC == 0 on the vector route
        if (i >= d.HW) continue;
        const int ph = H >> sh, pw = W >> sh;
        const S* src = base + ((size_t)n * cb + c) * (uint32_t)(ph * pw);
        S* op = out + (size_t)plane * d.HW + i;
        if (sh == 0) {                                      // the copy: the elements as they are
            *(P*)op = *(const P*)(src + i);
            continue;
        }
        const int h = (int)(i / d.W), w = (int)(i - (uint32_t)h * d.W);
        const float sy = (float)ph / (float)H, sx = (float)pw / (float)W;   // ATen compute_scales_value
        P r;
        if (d.mode == NMSA_MLPDEC_NEAREST) {
            const S* row = src + nearest_src(sy, h, ph) * pw;
#pragma unroll
            for (int k = 0; k < VEC; ++k) r.v[k] = row[nearest_src(sx, w + k, pw)];
        } else {
            int iy0, iy1;
            float wy0, wy1;
            bilinear_src(sy, h, ph, iy0, iy1, wy0, wy1);
            const S* r0 = src + iy0 * pw;
            const S* r1 = src + iy1 * pw;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                int ix0, ix1;
                float wx0, wx1;
                bilinear_src(sx, w + k, pw, ix0, ix1, wx0, wx1);
                r.v[k] = st<DTYPE>(bilerp(ld<DTYPE>(r0[ix0]), ld<DTYPE>(r0[ix1]),
                                          ld<DTYPE>(r1[ix0]), ld<DTYPE>(r1[ix1]),
                                          wx0, wx1, wy0, wy1));
            }
        }
        *(P*)op = r;
    }
}

// ------------------------------------------------------------------ upsample + concat backward
template <int DTYPE>
__global__ __launch_bounds__(MLD_THREADS) void k_mlpdec_upcat_bwd(
    const typename elem<DTYPE>::type* __restrict__ g_out, const MldDesc d, const uint32_t items)
{
    typedef typename elem<DTYPE>::type S;
    const int H = (int)d.H, W = (int)d.W;
    for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
        // the last branch whose first item is not behind `item` (a branch without items shares its
        // first item with the next one)
        uint32_t cb = d.c[0], sh = d.s[0], off = d.off[0], first = d.first[0];
        S* dst = (S*)d.p[0];
#pragma unroll
        for (int b = 1; b < NMSA_MLPDEC_MAX_BRANCHES; ++b)
            if (b < (int)d.n && item >= d.first[b]) {
                cb = d.c[b]; sh = d.s[b]; off = d.off[b]; first = d.first[b]; dst = (S*)d.p[b];
            }
        const int ph = H >> sh, pw = W >> sh;
        const uint32_t hw = (uint32_t)(ph * pw);
        const uint64_t idx0 = (uint64_t)(item - first) * MLD_THREADS;      // first source pixel of the item
        const uint64_t plane0 = idx0 / hw;
        const uint32_t r = (uint32_t)(idx0 - plane0 * hw) + threadIdx.x;
        const uint32_t dp = r / hw, pix = r - dp * hw;
        const uint64_t plane = plane0 + dp;
        if (plane >= (uint64_t)d.B * cb) continue;
        const int p = (int)(pix / (uint32_t)pw), q = (int)(pix - (uint32_t)p * (uint32_t)pw);
        const uint32_t n = (uint32_t)(plane / cb), c = (uint32_t)(plane - (uint64_t)n * cb);
        const S* gp = g_out + ((size_t)n * d.c_total + off + c) * d.HW;
        const float sy = (float)ph / (float)H, sx = (float)pw / (float)W;
        int h0, h1, w0, w1;
        mld_readers(d.mode, (int)sh, H, p, h0, h1);
        mld_readers(d.mode, (int)sh, W, q, w0, w1);
        float s = 0.0f;
        for (int h = h0; h <= h1; ++h) {
            float wy;
            if (!mld_reads(d.mode, sy, h, ph, p, wy)) continue;
            const S* row = gp + h * W;
            float acc = 0.0f;
            for (int w = w0; w <= w1; ++w) {
                float wx;
                if (mld_reads(d.mode, sx, w, pw, q, wx)) acc = __fmaf_rn(ld<DTYPE>(row[w]), wx, acc);
            }
            s = __fmaf_rn(acc, wy, s);
        }
        dst[plane * hw + pix] = st<DTYPE>(s);
    }
}

// ------------------------------------------------------------------------------------ host side
int mld_vec(int dtype) { return dtype == NMSA_F32 ? 4 : 8; }

// what every entry point checks of the sizes; NMSA_OK, NMSA_ERR_ARG or NMSA_ERR_UNSUPPORTED.  `c` may
// be NULL for the route query, which does not look at channels.
int mld_check_sizes(int dtype, int mode, int B, int H, int W, int n, const int* c, bool need_c, const int* s,
                    int64_t& c_total)
{
    if (dtype != NMSA_F32 && dtype != NMSA_BF16 && dtype != NMSA_F16) return NMSA_ERR_ARG;
    if (mode != NMSA_MLPDEC_NEAREST && mode != NMSA_MLPDEC_BILINEAR) return NMSA_ERR_ARG;
    if (B < 1 || H < 1 || W < 1) return NMSA_ERR_ARG;
    if (n < 1 || n > NMSA_MLPDEC_MAX_BRANCHES || !s || (need_c && !c)) return NMSA_ERR_ARG;
    c_total = 0;
    for (int i = 0; i < n; ++i) {
        if (s[i] < 0 || s[i] > MLD_MAX_SHIFT) return NMSA_ERR_ARG;
        if (H % (1 << s[i]) || W % (1 << s[i])) return NMSA_ERR_ARG;
        if (need_c) {
            if (c[i] < 1) return NMSA_ERR_ARG;
            c_total += c[i];
        }
    }
    if (H > MLD_MAX_DIM || W > MLD_MAX_DIM) return NMSA_ERR_UNSUPPORTED;    // 32-bit offsets inside a plane
    if ((int64_t)B * c_total > 0x7fffffffLL) return NMSA_ERR_UNSUPPORTED;
    return NMSA_OK;
}

// THE route rule of the forward kernel
bool mld_vector(const void* const* ys, const void* out, int dtype, int W, int n)
{
    if (W % mld_vec(dtype) || !aligned(out, 16)) return false;
    for (int i = 0; i < n; ++i)
        if (!aligned(ys[i], 16)) return false;
    return true;
}

void mld_desc(MldDesc& d, int B, int H, int W, int n, const int* c, const int* s, void* const* p, int mode,
              int64_t c_total)
{
    d.B = (uint32_t)B; d.H = (uint32_t)H; d.W = (uint32_t)W; d.HW = (uint32_t)(H * W);
    d.n = (uint32_t)n; d.c_total = (uint32_t)c_total; d.mode = mode;
    uint32_t off = 0;
    for (int i = 0; i < NMSA_MLPDEC_MAX_BRANCHES; ++i) {
        const bool on = i < n;
        d.c[i] = on ? (uint32_t)c[i] : 0u; d.s[i] = on ? (uint32_t)s[i] : 0u;
        d.off[i] = off; d.first[i] = 0; d.p[i] = on ? p[i] : nullptr;
        off += d.c[i];
    }
}

}  // namespace
}  // namespace nmsa

extern "C" int nmsa_mlpdec_route(const void* const* ys, const void* out, int dtype, int H, int W, int n,
                                 const int* s)
{
    using namespace nmsa;
    int64_t c_total = 0;
    const int rc = mld_check_sizes(dtype, NMSA_MLPDEC_NEAREST, 1, H, W, n, nullptr, false, s, c_total);
    if (rc == NMSA_ERR_ARG) return rc;
    if (!ys || !out || !elem_aligned(out, dtype)) return NMSA_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (!ys[i] || !elem_aligned(ys[i], dtype)) return NMSA_ERR_ARG;
    if (rc != NMSA_OK) return rc;
    return mld_vector(ys, out, dtype, W, n) ? NMSA_MLPDEC_ROUTE_VECTOR : NMSA_MLPDEC_ROUTE_ELEMENT;
}

extern "C" int nmsa_mlpdec_upcat_fwd(const void* const* ys, int dtype, int B, int H, int W, int n, const int* c,
                                     const int* s, int mode, void* out, nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    int64_t c_total = 0;
    const int rc = mld_check_sizes(dtype, mode, B, H, W, n, c, true, s, c_total);
    if (rc == NMSA_ERR_ARG) return rc;
    if (!ys || !out || !elem_aligned(out, dtype)) return NMSA_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (!ys[i] || !elem_aligned(ys[i], dtype)) return NMSA_ERR_ARG;
    if (rc != NMSA_OK) return rc;
    const bool vector = mld_vector(ys, out, dtype, W, n);
    const uint64_t run = (uint64_t)MLD_THREADS * (vector ? mld_vec(dtype) : 1);
    const uint64_t chunks = ((uint64_t)H * W + run - 1) / run;
    const uint64_t items = (uint64_t)B * c_total * chunks;
    if (items > 0x7fffffffull) return NMSA_ERR_UNSUPPORTED;
    MldDesc d;
    mld_desc(d, B, H, W, n, c, s, (void* const*)ys, mode, c_total);
    const dim3 grid(capped_grid(items, MLD_BLOCKS_PER_CU)), block(MLD_THREADS);
#define MLD_UPCAT_FWD(DT)                                                                                   \
    do {                                                                                                    \
        typedef elem<DT>::type S;                                                                           \
        if (vector)                                                                                         \
            hipLaunchKernelGGL((k_mlpdec_upcat_fwd<DT, 16 / sizeof(S)>), grid, block, 0, stream, (S*)out, d, \
                               (uint32_t)chunks, (uint32_t)items);                                          \
        else                                                                                                \
            hipLaunchKernelGGL((k_mlpdec_upcat_fwd<DT, 1>), grid, block, 0, stream, (S*)out, d,             \
                               (uint32_t)chunks, (uint32_t)items);                                          \
    } while (0)
    NMSA_DISPATCH_DTYPE(dtype, MLD_UPCAT_FWD)
#undef MLD_UPCAT_FWD
    return check_launch();
}

extern "C" int nmsa_mlpdec_upcat_bwd(const void* g_out, int dtype, int B, int H, int W, int n, const int* c,
                                     const int* s, int mode, void* const* gys, nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    int64_t c_total = 0;
    const int rc = mld_check_sizes(dtype, mode, B, H, W, n, c, true, s, c_total);
    if (rc == NMSA_ERR_ARG) return rc;
    if (!g_out || !gys || !elem_aligned(g_out, dtype)) return NMSA_ERR_ARG;
    bool any = false;
    for (int i = 0; i < n; ++i) {
        if (!elem_aligned(gys[i], dtype)) return NMSA_ERR_ARG;    // NULL: that gradient is not wanted
        any = any || gys[i];
    }
    if (rc != NMSA_OK) return rc;
    MldDesc d;
    mld_desc(d, B, H, W, n, c, s, gys, mode, c_total);
    // (the gradient of a branch with s_i == 0 is the view g_out[:, off_i : off_i + c_i]: a caller passes
    // NULL for it; a pointer gets the copy, one pixel per lane)
    uint64_t items = 0;
    for (int i = 0; i < n; ++i) {
        if (items > 0x7fffffffull) return NMSA_ERR_UNSUPPORTED;
        d.first[i] = (uint32_t)items;
        if (!gys[i]) continue;
        const uint64_t pixels = (uint64_t)B * c[i] * (uint64_t)(H >> s[i]) * (uint64_t)(W >> s[i]);
        items += (pixels + MLD_THREADS - 1) / MLD_THREADS;
    }
    if (items > 0x7fffffffull) return NMSA_ERR_UNSUPPORTED;
    if (!any || items == 0) return NMSA_OK;
    const dim3 grid(capped_grid(items, MLD_BLOCKS_PER_CU)), block(MLD_THREADS);
#define MLD_UPCAT_BWD(DT)                                                                                   \
    hipLaunchKernelGGL((k_mlpdec_upcat_bwd<DT>), grid, block, 0, stream, (const elem<DT>::type*)g_out, d,   \
                       (uint32_t)items)
    NMSA_DISPATCH_DTYPE(dtype, MLD_UPCAT_BWD)
#undef MLD_UPCAT_BWD
    return check_launch();
}
