// scene.hip — the scene-classification task's whole step in ONE launch on gfx950.
//
// Replaces, behind the C ABI of include/nmsa.h,
//   ScenePostprocessing._postprocess_inference   (model/postprocessing/scene.py:42-44: softmax, max)
//   SceneTaskHelper._compute_losses              (task_helper/scene.py:61-63: CrossEntropyLoss with
//                                                 weight, label_smoothing, ignore_index=-1, 'mean')
//   SceneTaskHelper.validation_step              (task_helper/scene.py:104-108: the masked
//                                                 ConfusionMatrix update, there on the host)
//
//   k_scene_step   logits [B, C] + labels [B] -> score, idx, loss, d loss / d logits, confusion
//                  matrix counts and status bits, each only where its pointer is given
//
// The data is tiny ([B, C] with C around 10-45), so the step is latency, not bandwidth: ONE
// workgroup of 16 waves takes the whole batch.  Waves take rows, lanes take classes (lane, lane +
// 64, ...); a row is read three times — maximum / argmax, sum of exponentials, gradient — the
// second and third time from cache, so no per-lane class array exists and every C runs the same
// code.  Row reductions are cross-lane butterflies (every lane ends with the same bits).
//
// Arithmetic.  The logits are promoted exactly (bf16 / f16 -> f32 -> f64); the argmax compares
// the promoted values (first index on equal values, like torch.max on the CPU); exponentials,
// logarithm, sums and quotients of a row are float64 and every output is rounded ONCE to its type:
// an output is within one rounding of the exact value of the torch expression, whatever the order
// of summation.  (A whole validation call takes 24 us; float64's share of it was not measured.)
//
// Determinism.  No float atomics.  The divisor (sum of w[target] over the non-void rows) and the
// weight sum are reduced lane -> wave -> workgroup in a fixed order BEFORE the rows are walked
// (they need the labels only), so the gradient is written in the same pass as the loss terms.  The
// rows' loss terms go to LDS, 1024 rows at a time; wave 0 adds them lane-strided in ascending row
// order and folds its lanes once at the end.  The confusion matrix takes 64-bit integer atomic
// adds, whose order does not matter.
#include "nmsa_common.hpp"

#include <limits.h>
#include <math.h>

namespace nmsa {
namespace {

constexpr int SC_THREADS = 1024;
constexpr int SC_WAVES = SC_THREADS / kWave;
constexpr int SC_CHUNK = 1024;                  // rows whose loss terms one pass keeps in LDS

struct SceneArgs {
    const void* logits;
    const void* labels;
    const float* weights;
    float* score;
    long long* idx;
    float* loss;
    void* grad;
    unsigned long long* confmat;
    int* status;
    int B, C, label_dtype;
    float smoothing;
};

template <int DTYPE>
__device__ __forceinline__ void st_grad(void* p, size_t i, double g)
{
    const float f = (float)g;
    if (DTYPE == NMSA_F32) {
        ((float*)p)[i] = f;
    } else if (DTYPE == NMSA_F16) {
        ((_Float16*)p)[i] = (_Float16)f;
    } else {
        uint32_t u = __float_as_uint(f);
        // round to nearest even on the upper half; a NaN stays one
        u = (f != f) ? 0x7fc00000u : u + 0x7fffu + ((u >> 16) & 1u);
        ((uint16_t*)p)[i] = (uint16_t)(u >> 16);
    }
}

__device__ __forceinline__ long long ld_label(const void* p, int dtype, long long r)
{
    if (dtype == NMSA_U8) return ((const uint8_t*)p)[r];
    if (dtype == NMSA_I32) return ((const int32_t*)p)[r];
    return ((const long long*)p)[r];
}

// every lane ends with the wave's sum; the same bits in every lane (a + b == b + a per level)
__device__ __forceinline__ double wave_allreduce_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// every thread ends with the workgroup's sum: lanes, then the waves in ascending order
__device__ __forceinline__ double block_allreduce_sum(double v, double* part)
{
    v = wave_allreduce_sum(v);
    __syncthreads();                             // `part` may still be read from the call before
    if (lane_id() == 0) part[threadIdx.x / kWave] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < SC_WAVES; ++i) s += part[i];
    return s;
}

template <int DTYPE>
__global__ __launch_bounds__(SC_THREADS) void k_scene_step(SceneArgs a)
{
    __shared__ double s_part[SC_WAVES];
    __shared__ double s_term[SC_CHUNK];
    const int lane = lane_id(), wave = (int)(threadIdx.x / kWave);
    const int B = a.B, C = a.C;
    const bool want_loss = a.loss != nullptr, want_grad = a.grad != nullptr;
    const double eps = (double)a.smoothing;
    const double eps_c = eps / (double)C;

    // divisor D = sum of w[target] over the non-void rows; W = sum of all class weights
    double D = 0.0, W = (double)C;
    if (want_loss || want_grad) {
        double d = 0.0;
        for (long long r = threadIdx.x; r < B; r += SC_THREADS) {
            const long long l = ld_label(a.labels, a.label_dtype, r);
            if (l >= 1 && l <= C) d += a.weights ? (double)a.weights[l - 1] : 1.0;
        }
        D = block_allreduce_sum(d, s_part);
        if (a.weights) {
            double w = 0.0;
            for (int c = (int)threadIdx.x; c < C; c += SC_THREADS) w += (double)a.weights[c];
            W = block_allreduce_sum(w, s_part);
        }
    }

    double acc = 0.0;                            // wave 0: this lane's share of the numerator
    for (long long chunk0 = 0; chunk0 < B; chunk0 += SC_CHUNK) {
        const int n = (int)min((long long)SC_CHUNK, (long long)B - chunk0);
        for (int k = wave; k < n; k += SC_WAVES) {
            const long long r = chunk0 + k;
            const size_t base = (size_t)r * (size_t)C;

            // maximum and its first index
            float bv = -INFINITY;
            int bi = INT_MAX;
            for (int c = lane; c < C; c += kWave) {
                const float x = ld_at<DTYPE>(a.logits, base + c);
                if (bi == INT_MAX || x > bv) { bv = x; bi = c; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o);
                const int oi = __shfl_xor(bi, o);
                if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            const double m = (double)bv;

            // S = sum exp(x - m); with label smoothing also A = sum w[c] * x[c]
            double s = 0.0, wx = 0.0;
            for (int c = lane; c < C; c += kWave) {
                const double x = (double)ld_at<DTYPE>(a.logits, base + c);
                s += exp(x - m);
                if (eps > 0.0) wx += (a.weights ? (double)a.weights[c] : 1.0) * x;
            }
            s = wave_allreduce_sum(s);
            // a row that holds a NaN or a +inf, or is all -inf: its softmax is all NaN (exp(x - m) has
            // a NaN term exactly then; every other row sums terms in [0, 1] with one of them 1), and
            // torch.max of an all-NaN row answers its first element: score NaN, index 0.  The argmax
            // of the raw logits above would drop a NaN and follow a +inf.
            const bool poisoned = s != s;
            if (poisoned) bi = 0;

            long long l = 0;
            if (a.labels) l = ld_label(a.labels, a.label_dtype, r);
            const bool valid = l >= 1 && l <= C;
            const int t = valid ? (int)(l - 1) : 0;
            if (lane == 0) {
                if (a.score) a.score[r] = (float)(1.0 / s);
                if (a.idx) a.idx[r] = (long long)bi;
                if (valid && a.confmat) atomicAdd(&a.confmat[(size_t)t * C + bi], 1ull);
                if (!valid && l != 0 && a.status) atomicOr(a.status, NMSA_ST_VALUE_RANGE);
            }
            if (!want_loss && !want_grad) continue;

            const double wt = (valid && a.weights) ? (double)a.weights[t] : 1.0;
            if (want_loss) {
                double term = 0.0;
                if (valid) {
                    const double log_s = log(s);
                    const double xt = (double)ld_at<DTYPE>(a.logits, base + t);
                    term = (1.0 - eps) * wt * (log_s + (m - xt));
                    if (eps > 0.0) term += eps_c * (W * (m + log_s) - wave_allreduce_sum(wx));
                }
                if (lane == 0) s_term[k] = term;
            }
            if (want_grad) {
                for (int c = lane; c < C; c += kWave) {
                    // a void row: 0, but NaN where its softmax is (F.cross_entropy hands an ignored row
                    // 0 - softmax * 0 through log_softmax's backward)
                    double g = poisoned ? (double)NAN : 0.0;
                    if (valid) {
                        const double x = (double)ld_at<DTYPE>(a.logits, base + c);
                        const double p = exp(x - m) / s;
                        const double wc = a.weights ? (double)a.weights[c] : 1.0;
                        g = ((1.0 - eps) * wt * (p - (c == t ? 1.0 : 0.0)) + eps_c * (W * p - wc)) / D;
                    }
                    st_grad<DTYPE>(a.grad, base + c, g);
                }
            }
        }
        if (want_loss) {
            __syncthreads();
            if (wave == 0)
                for (int i = lane; i < n; i += kWave) acc += s_term[i];
            __syncthreads();
        }
    }
    if (want_loss && wave == 0) {
        acc = wave_allreduce_sum(acc);
        if (lane == 0) {
            a.loss[0] = (float)acc;
            a.loss[1] = (float)D;
            a.loss[2] = (float)(acc / D);        // no non-void row: 0 / 0, as torch
        }
    }
}

}  // namespace
}  // namespace nmsa

extern "C" int nmsa_scene_step(const void* logits, int logits_dtype, const void* labels, int label_dtype,
                               int B, int C, const float* class_weights, float label_smoothing,
                               float* score, int64_t* idx, float* loss, void* grad, int64_t* confmat,
                               int32_t* status, nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    if (!logits || B < 1 || C < 1 || C > NMSA_SCENE_MAX_CLASSES) return NMSA_ERR_ARG;
    if (!(label_smoothing >= 0.0f && label_smoothing <= 1.0f)) return NMSA_ERR_ARG;       // NaN too
    if (!labels && (loss || grad || confmat)) return NMSA_ERR_ARG;
    if (logits_dtype != NMSA_F32 && logits_dtype != NMSA_BF16 && logits_dtype != NMSA_F16)
        return NMSA_ERR_UNSUPPORTED;
    if (labels && label_dtype != NMSA_U8 && label_dtype != NMSA_I32 && label_dtype != NMSA_I64)
        return NMSA_ERR_UNSUPPORTED;
    if (!score && !idx && !loss && !grad && !confmat && !(labels && status)) return NMSA_OK;  // nothing wanted
    const SceneArgs a{logits, labels, class_weights, score, (long long*)idx, loss, grad,
                      (unsigned long long*)confmat, status, B, C, label_dtype, label_smoothing};
    switch (logits_dtype) {
        case NMSA_F32: hipLaunchKernelGGL(k_scene_step<NMSA_F32>, dim3(1), dim3(SC_THREADS), 0, stream, a); break;
        case NMSA_BF16: hipLaunchKernelGGL(k_scene_step<NMSA_BF16>, dim3(1), dim3(SC_THREADS), 0, stream, a); break;
        default: hipLaunchKernelGGL(k_scene_step<NMSA_F16>, dim3(1), dim3(SC_THREADS), 0, stream, a); break;
    }
    return check_launch();
}
