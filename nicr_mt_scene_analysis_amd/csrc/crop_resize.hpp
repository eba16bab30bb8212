// crop_resize.hpp — geometry of "crop to the valid region, resize to the dataset resolution"
// (reference model/postprocessing/dense_base.py:15-58), shared by every kernel that reads a
// network-resolution map at full-resolution coordinates (resize.hip, normal.hip), and ATen's source
// index and blend arithmetic for every kernel that resamples (context_module.hip, mlp_decoder.hip too).
#pragma once
#include "nmsa_common.hpp"

namespace nmsa {

struct CropResize {
    int Hs, Ws;        // source plane size
    int y0, x0, h, w;  // valid region inside the source plane
    int Ho, Wo;        // output plane size
    float sy, sx;      // float(h)/float(Ho), float(w)/float(Wo)
};

// ATen's nearest source index (F.interpolate(mode='nearest'), pinned by
// tests/golden/fullres_cases.npz): src = min(int(floorf(dst * scale)), in - 1)
__device__ __forceinline__ int nearest_src(float scale, int dst, int in)
{
    return min((int)floorf(__fmul_rn((float)dst, scale)), in - 1);
}

// ATen's bilinear source (area_pixel_compute_source_index, align_corners = False): the two source
// indices of `dst` and their weights
__device__ __forceinline__ void bilinear_src(float scale, int dst, int in,
                                             int& i0, int& i1, float& w0, float& w1)
{
    float s = __fmaf_rn(scale, __fadd_rn((float)dst, 0.5f), -0.5f);
    s = (s < 0.f) ? 0.f : s;
    i0 = min((int)s, in - 1);
    i1 = min(i0 + 1, in - 1);
    w1 = fminf(fmaxf(__fsub_rn(s, (float)i0), 0.f), 1.f);
    w0 = __fsub_rn(1.0f, w1);
}

// the blend (a*wx0 + b*wx1)*wy0 + (c*wx0 + d*wx1)*wy1 with one fused multiply-add per sum
__device__ __forceinline__ float bilerp(float a, float b, float c, float d,
                                        float wx0, float wx1, float wy0, float wy1)
{
    const float t0 = __fmaf_rn(a, wx0, __fmul_rn(b, wx1));
    const float t1 = __fmaf_rn(c, wx0, __fmul_rn(d, wx1));
    return __fmaf_rn(t0, wy0, __fmul_rn(t1, wy1));
}

inline bool bad_geometry(int planes, int Hs, int Ws, int y0, int x0, int h, int w, int Ho, int Wo)
{
    if (planes <= 0 || Hs <= 0 || Ws <= 0 || h <= 0 || w <= 0 || Ho <= 0 || Wo <= 0) return true;
    if (y0 < 0 || x0 < 0 || (int64_t)y0 + h > Hs || (int64_t)x0 + w > Ws) return true;
    if ((int64_t)Hs * Ws > ((int64_t)1 << 30) || (int64_t)Ho * Wo > ((int64_t)1 << 30)) return true;
    return false;
}

inline CropResize make_geometry(int Hs, int Ws, int y0, int x0, int h, int w, int Ho, int Wo)
{
    CropResize g;
    g.Hs = Hs; g.Ws = Ws; g.y0 = y0; g.x0 = x0; g.h = h; g.w = w; g.Ho = Ho; g.Wo = Wo;
    g.sy = (float)h / (float)Ho;      // ATen compute_scales_value<float>
    g.sx = (float)w / (float)Wo;
    return g;
}

}  // namespace nmsa
