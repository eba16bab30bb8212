// maae.hip — orientation MAE on device tables (gfx950).
//
// Replaces, behind the C ABI of include/nmsa.h, the host loops of
//   MeanAbsoluteAngularError.update                       (metric/mae.py:40-64)
//   PanopticQualityWithOrientationMAE.update_mae          (metric/mae.py:129-162)
//
//   k_maae_keyed     every valid key of the prediction table is looked up in the target table of
//                    the same image; |angle error| and the pair count go into the metric's states
//   k_maae_matched   the match table of nmsa_pq_update joined with two id tables and two
//                    orientation tables: target id -> target instance -> target angle, then
//                    pred id -> pred instance -> pred angle; a pair counts when all four hit
//
// The work is at most a few thousand pairs per batch and latency-bound, so ONE workgroup walks the
// images in order.  Lane l takes entries l, l + 256, ... of every image: the assignment of pairs to
// lanes, the lane -> wave -> workgroup reduction and the single read-modify-write of the states are
// all fixed, so two runs on the same input give bit-identical states (no atomic whose order varies).
//
// The error is the float32 chain of abs_angle_error_rad (`%` of torch on float32 tensors is fmod
// plus the divisor where the result is non-zero and negative), every step IEEE-rounded: exact
// fmodf, no contraction (-ffp-contract=off), no fast-math.  Each error is widened to f64 before
// it is added.
#include <math.h>
#include "nmsa_common.hpp"

namespace nmsa {
namespace {

constexpr int MAAE_THREADS = 256;

struct OrientationTable {
    const int32_t* keys;        // [B,K] ascending in [0, n[b]); NULL: dense, key = column
    const float* angle;         // [B,K]
    const uint8_t* valid;       // [B,K]
    const int32_t* n;           // [B]; may be NULL for a dense table
    const int32_t* status;      // [1] status word of the kernel that made the table, or NULL
    int K;
};

struct IdTable {
    const int64_t* pan;         // [B,K]
    const int64_t* ins;         // [B,K]
    const int32_t* n;           // [B]
    int K;
    int ascending;              // pan rows ascend: binary search; otherwise a linear walk
};

__device__ __forceinline__ int row_length(const int32_t* n, int b, int K)
{
    const int v = n[b];
    return v < 0 ? 0 : (v > K ? K : v);
}

__device__ __forceinline__ bool orientation_lookup(const OrientationTable& t, int b, long long key,
                                                   float& angle)
{
    int at;
    if (!t.keys) {
        if (key < 0 || key >= t.K) return false;
        at = (int)key;
    } else {
        const int32_t* row = t.keys + (size_t)b * t.K;
        int lo = 0, hi = row_length(t.n, b, t.K);
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((long long)row[mid] < key) lo = mid + 1; else hi = mid;
        }
        if (lo >= row_length(t.n, b, t.K) || (long long)row[lo] != key) return false;
        at = lo;
    }
    const size_t i = (size_t)b * t.K + at;
    if (!t.valid[i]) return false;
    angle = t.angle[i];
    return true;
}

__device__ __forceinline__ bool id_lookup(const IdTable& t, int b, long long pan, long long& ins)
{
    const int64_t* row = t.pan + (size_t)b * t.K;
    const int n = row_length(t.n, b, t.K);
    int at = -1;
    if (t.ascending) {
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((long long)row[mid] < pan) lo = mid + 1; else hi = mid;
        }
        if (lo < n && (long long)row[lo] == pan) at = lo;
    } else {
        for (int i = 0; i < n; ++i)
            if ((long long)row[i] == pan) { at = i; break; }
    }
    if (at < 0) return false;
    ins = (long long)t.ins[(size_t)b * t.K + at];
    return true;
}

// torch's `x % m` for float32 and m > 0
__device__ __forceinline__ float rem_positive(float x, float m)
{
    float r = fmodf(x, m);
    if (r != 0.f && r < 0.f) r = __fadd_rn(r, m);
    return r;
}

__device__ __forceinline__ float abs_angle_error(float pred, float target)
{
    const float two_pi = (float)(2.0 * M_PI);
    const float pi = (float)M_PI;
    // ONE copy of the fmodf expansion, walked three times (pred, target, their shifted difference):
    // three inlined copies cost the matched kernel more scalar registers than it has
    float x = pred, first = 0.f;
#pragma nounroll
    for (int k = 0; k < 3; ++k) {
        const float r = rem_positive(x, two_pi);
        if (k == 0) { first = r; x = target; }
        else if (k == 1) x = __fadd_rn(__fsub_rn(first, r), pi);
        else x = r;
    }
    return fabsf(__fsub_rn(x, pi));
}

// status bits of the kernels that made the tables (1 too many ids, 32 id out of range) -> ours
__device__ __forceinline__ int table_status(const int32_t* word)
{
    if (!word) return 0;
    const int v = *word;
    return ((v & 1) ? NMSA_ST_MAAE_WIDE_OVERFLOW : 0) | ((v & 32) ? NMSA_ST_MAAE_WIDE_RANGE : 0);
}

// lane -> wave -> workgroup in a fixed order, then ONE read-modify-write per state by thread 0
__device__ __forceinline__ void commit(double acc, long long cnt, int st, double* sum_state,
                                       long long* count_state, int32_t* status)
{
    acc = wave_reduce_sum(acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_down(cnt, o);
        st |= __shfl_down(st, o);
    }
    __shared__ double wave_sum[MAAE_THREADS / kWave];
    __shared__ long long wave_cnt[MAAE_THREADS / kWave];
    __shared__ int wave_st[MAAE_THREADS / kWave];
    const int wv = threadIdx.x / kWave;
    if (lane_id() == 0) { wave_sum[wv] = acc; wave_cnt[wv] = cnt; wave_st[wv] = st; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double bs = 0.0;
        long long bc = 0;
        int bst = 0;
#pragma unroll
        for (int i = 0; i < MAAE_THREADS / kWave; ++i) { bs += wave_sum[i]; bc += wave_cnt[i]; bst |= wave_st[i]; }
        if (bc) {
            *sum_state = *sum_state + bs;
            *count_state = *count_state + bc;
        }
        if (bst) atomicOr(status, bst);
    }
}

__global__ __launch_bounds__(MAAE_THREADS) void k_maae_keyed(
    OrientationTable pred, OrientationTable target, int B, double* __restrict__ sum_state,
    long long* __restrict__ count_state, int32_t* __restrict__ status)
{
    double acc = 0.0;
    long long cnt = 0;
    int st = 0;
    if (threadIdx.x == 0) st = table_status(pred.status) | table_status(target.status);
    for (int b = 0; b < B; ++b) {
        const int n = pred.keys ? row_length(pred.n, b, pred.K) : pred.K;
        for (int i = threadIdx.x; i < n; i += MAAE_THREADS) {
            const size_t at = (size_t)b * pred.K + i;
            if (!pred.valid[at]) continue;
            const long long key = pred.keys ? (long long)pred.keys[at] : (long long)i;
            float t;
            if (!orientation_lookup(target, b, key, t)) { st |= NMSA_ST_MAAE_MISSING_TARGET; continue; }
            acc += (double)abs_angle_error(pred.angle[at], t);
            cnt += 1;
        }
    }
    commit(acc, cnt, st, sum_state, count_state, status);
}

__global__ __launch_bounds__(MAAE_THREADS) void k_maae_matched(
    const int64_t* __restrict__ matches, const int32_t* __restrict__ n_matches, int cap,
    IdTable pred_ids, OrientationTable pred, IdTable target_ids, OrientationTable target, int B,
    double* __restrict__ sum_state, long long* __restrict__ count_state, int32_t* __restrict__ status)
{
    // The four table descriptors (14 pointers) live in LDS and the two sides of the join share one
    // copy of the lookup code: held in scalar registers across the loops they do not fit.
    __shared__ IdTable s_ids[2];
    __shared__ OrientationTable s_ori[2];
    double acc = 0.0;
    long long cnt = 0;
    int st = 0;
    if (threadIdx.x == 0) {
        st = table_status(pred.status) | table_status(target.status);
        s_ids[0] = target_ids; s_ids[1] = pred_ids;
        s_ori[0] = target; s_ori[1] = pred;
    }
    __syncthreads();
    for (int b = 0; b < B; ++b) {
        int n = n_matches[b];
        if (n > cap) {                  // the image contributes the rows the table holds
            if (threadIdx.x == 0) st |= NMSA_ST_MAAE_MATCH_OVERFLOW;
            n = cap;
        }
        for (int i = threadIdx.x; i < n; i += MAAE_THREADS) {
            const int64_t* m = matches + ((size_t)b * cap + i) * 2;
            const long long target_id = (long long)m[0], pred_id = (long long)m[1];
            if (target_id == 0) continue;               // stuff / void / background
            float t = 0.f, p = 0.f;
            bool hit = true;
#pragma nounroll
            for (int side = 0; side < 2 && hit; ++side) {       // the target first, then the prediction
                long long ins;
                float a;
                hit = id_lookup(s_ids[side], b, side ? pred_id : target_id, ins) &&
                      orientation_lookup(s_ori[side], b, ins, a);
                if (hit) { if (side) p = a; else t = a; }
            }
            if (!hit) continue;
            acc += (double)abs_angle_error(p, t);
            cnt += 1;
        }
    }
    commit(acc, cnt, st, sum_state, count_state, status);
}

bool bad_table(const OrientationTable& t)
{
    return !t.angle || !t.valid || t.K <= 0 || (t.keys && !t.n);
}

bool bad_table(const IdTable& t)
{
    return !t.pan || !t.ins || !t.n || t.K <= 0;
}

}  // namespace
}  // namespace nmsa

using namespace nmsa;

extern "C" int nmsa_maae_update_keyed(
    const int32_t* pred_keys, const float* pred_angle, const uint8_t* pred_valid, const int32_t* pred_n,
    int pred_K, const int32_t* pred_status,
    const int32_t* target_keys, const float* target_angle, const uint8_t* target_valid,
    const int32_t* target_n, int target_K, const int32_t* target_status,
    int B, double* sum_state, int64_t* count_state, int32_t* status, nmsa_stream_t stream_)
{
    const OrientationTable pred{pred_keys, pred_angle, pred_valid, pred_n, pred_status, pred_K};
    const OrientationTable target{target_keys, target_angle, target_valid, target_n, target_status,
                                  target_K};
    if (B <= 0 || !sum_state || !count_state || !status || bad_table(pred) || bad_table(target))
        return NMSA_ERR_ARG;
    hipLaunchKernelGGL(k_maae_keyed, dim3(1), dim3(MAAE_THREADS), 0, (hipStream_t)stream_, pred, target,
                       B, sum_state, (long long*)count_state, status);
    return check_launch();
}

extern "C" int nmsa_maae_update_matched(
    const int64_t* matches, const int32_t* n_matches, int match_capacity,
    const int64_t* pred_ids_pan, const int64_t* pred_ids_ins, const int32_t* pred_ids_n, int pred_ids_K,
    int pred_ids_ascending,
    const int32_t* pred_keys, const float* pred_angle, const uint8_t* pred_valid, const int32_t* pred_n,
    int pred_K, const int32_t* pred_status,
    const int64_t* target_ids_pan, const int64_t* target_ids_ins, const int32_t* target_ids_n,
    int target_ids_K, int target_ids_ascending,
    const int32_t* target_keys, const float* target_angle, const uint8_t* target_valid,
    const int32_t* target_n, int target_K, const int32_t* target_status,
    int B, double* sum_state, int64_t* count_state, int32_t* status, nmsa_stream_t stream_)
{
    const IdTable pred_ids{pred_ids_pan, pred_ids_ins, pred_ids_n, pred_ids_K, pred_ids_ascending};
    const IdTable target_ids{target_ids_pan, target_ids_ins, target_ids_n, target_ids_K,
                             target_ids_ascending};
    const OrientationTable pred{pred_keys, pred_angle, pred_valid, pred_n, pred_status, pred_K};
    const OrientationTable target{target_keys, target_angle, target_valid, target_n, target_status,
                                  target_K};
    if (B <= 0 || !matches || !n_matches || match_capacity <= 0 || !sum_state || !count_state ||
        !status || bad_table(pred_ids) || bad_table(target_ids) || bad_table(pred) || bad_table(target))
        return NMSA_ERR_ARG;
    hipLaunchKernelGGL(k_maae_matched, dim3(1), dim3(MAAE_THREADS), 0, (hipStream_t)stream_, matches,
                       n_matches, match_capacity, pred_ids, pred, target_ids, target, B, sum_state,
                       (long long*)count_state, status);
    return check_launch();
}
