// multiscale.hip — side-output targets: every key of a batch at every downscale in ONE launch.
//
// Replaces, behind the C ABI of include/nmsa.h, the per-key, per-scale nearest resizes of
//   MultiscaleSupervisionGenerator._preprocess  (data/preprocessing/multiscale_supervision.py:41-67)
//   -> resize(), cv2.INTER_NEAREST branch        (data/preprocessing/resize.py:95-161)
//
//   k_multiscale_nearest   one descriptor per (key, scale): dst[p, y, x] = src[p, rows[y], cols[x]]
//                          over the leading planes p = B * C, elements moved as raw bits of 1, 2,
//                          4 or 8 bytes (no float conversion: NaN payloads and -0.0 survive)
//
// The index maps `rows` / `cols` come from the host, which evaluates OpenCV's rule in double
// arithmetic once per shape; nothing of the rule is evaluated here.  The outputs are small
// (downscales 8 / 16 / 32 are under 2 % of the input), so the cost of the torch formulation is its
// launches, one or two per key and scale: here a workgroup finds its descriptor from the block
// prefix in the table (wave-uniform loads) and each lane moves one output element, consecutive
// lanes consecutive elements of an output row, so the stores coalesce; the loads are a strided
// gather by nature.
//
// The table and the maps travel in one pinned staging buffer: the entry point checks every field
// on the host copy (shapes, element sizes, map offsets, every map entry against its source side)
// BEFORE anything is enqueued, fills in the block prefix, then enqueues one asynchronous copy and
// the launch.  No host synchronisation; capturable in a hipGraph (the copy node re-reads the
// pinned buffer at replay: a captured call needs a staging buffer of its own).
#include "nmsa_common.hpp"

#include <string.h>

namespace nmsa {
namespace {

constexpr int MS_THREADS = 256;

static_assert(sizeof(nmsa_multiscale_desc) == 64, "the staging layout is 16 words per descriptor");

template <typename T>
__device__ __forceinline__ void move_one(const nmsa_multiscale_desc& d, size_t s, size_t e)
{
    ((T*)d.dst)[e] = ((const T*)d.src)[s];
}

__global__ __launch_bounds__(MS_THREADS) void k_multiscale_nearest(
    const nmsa_multiscale_desc* __restrict__ table, int n_desc, const int32_t* __restrict__ maps)
{
    // table[i].block_begin <= blockIdx.x < table[i + 1].block_begin; the same for every lane
    int lo = 0, hi = n_desc;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((uint32_t)table[mid].block_begin <= blockIdx.x) lo = mid; else hi = mid;
    }
    const nmsa_multiscale_desc d = table[lo];
    const uint32_t total = (uint32_t)d.planes * (uint32_t)d.h * (uint32_t)d.w;    // < 2^31, checked
    const uint32_t e = (blockIdx.x - (uint32_t)d.block_begin) * MS_THREADS + threadIdx.x;
    if (e >= total) return;
    const uint32_t x = e % (uint32_t)d.w;
    const uint32_t t = e / (uint32_t)d.w;
    const uint32_t y = t % (uint32_t)d.h;
    const uint32_t p = t / (uint32_t)d.h;
    const size_t s = ((size_t)p * d.H + (size_t)maps[d.row_map + y]) * d.W + (size_t)maps[d.col_map + x];
    switch (d.log2_size) {
        case 0: move_one<uint8_t>(d, s, e); break;
        case 1: move_one<uint16_t>(d, s, e); break;
        case 2: move_one<uint32_t>(d, s, e); break;
        default: move_one<uint64_t>(d, s, e); break;
    }
}

}  // namespace
}  // namespace nmsa

extern "C" int nmsa_multiscale_nearest(void* staging_host, void* staging_device, int n_desc,
                                       int n_words, nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    if (!staging_host || !staging_device || n_desc <= 0 || n_desc > NMSA_MULTISCALE_MAX_DESC ||
        (uintptr_t)staging_host % 8 != 0 || (uintptr_t)staging_device % 8 != 0)
        return NMSA_ERR_ARG;
    const int64_t table_words = (int64_t)n_desc * 16;
    if ((int64_t)n_words < table_words) return NMSA_ERR_ARG;
    const int64_t map_words = (int64_t)n_words - table_words;
    nmsa_multiscale_desc* table = (nmsa_multiscale_desc*)staging_host;
    const int32_t* maps = (const int32_t*)staging_host + table_words;
    int64_t blocks = 0;
    for (int i = 0; i < n_desc; ++i) {
        nmsa_multiscale_desc& d = table[i];
        if (!d.src || !d.dst || d.planes <= 0 || d.H <= 0 || d.W <= 0 || d.h <= 0 || d.w <= 0 ||
            d.log2_size < 0 || d.log2_size > 3)
            return NMSA_ERR_ARG;
        if (d.src % ((uint64_t)1 << d.log2_size) != 0 || d.dst % ((uint64_t)1 << d.log2_size) != 0)
            return NMSA_ERR_ARG;
        if ((int64_t)d.planes * d.h * d.w > 0x7fffffffLL) return NMSA_ERR_ARG;
        if (d.row_map < 0 || d.col_map < 0 || (int64_t)d.row_map + d.h > map_words ||
            (int64_t)d.col_map + d.w > map_words)
            return NMSA_ERR_ARG;
        for (int y = 0; y < d.h; ++y)
            if (maps[d.row_map + y] < 0 || maps[d.row_map + y] >= d.H) return NMSA_ERR_ARG;
        for (int x = 0; x < d.w; ++x)
            if (maps[d.col_map + x] < 0 || maps[d.col_map + x] >= d.W) return NMSA_ERR_ARG;
        d.block_begin = (int32_t)blocks;
        blocks += ((int64_t)d.planes * d.h * d.w + MS_THREADS - 1) / MS_THREADS;
        if (blocks > 0x7fffffffLL) return NMSA_ERR_ARG;
    }
    if (check_hip(hipMemcpyAsync(staging_device, staging_host, (size_t)n_words * 4,
                                 hipMemcpyHostToDevice, stream)))
        return NMSA_ERR_LAUNCH;
    hipLaunchKernelGGL(k_multiscale_nearest, dim3((unsigned)blocks), dim3(MS_THREADS), 0, stream,
                       (const nmsa_multiscale_desc*)staging_device, n_desc,
                       (const int32_t*)staging_device + table_words);
    return check_launch();
}
