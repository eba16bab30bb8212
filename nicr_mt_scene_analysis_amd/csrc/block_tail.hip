// block_tail.hip — the batch-norm tail of the residual blocks (reference model/block.py: BasicBlock,
// Bottleneck, NonBottleneck1D), every norm-to-activation segment as ONE chain of at most two launches
// per direction:
//
//   training: mean_c = sum(x) / M, var_c = sum((x - mean_c)^2) / M over M = B*H*W    eval: the running statistics
//   invstd = 1 / sqrt(var + eps)   xh = (x - mean) * invstd   u = xh * gamma + beta
//   v = u * s[b,c] (s absent: u)   z = v + id (id absent: v)   y = act(z), act = ReLU | SiLU
//   gz = gy * act'(z)   gid = gz   gu = gz * s   dbeta = sum(gu)   dgamma = sum(gu * xh)
//   training: gx = gamma * invstd * ((gu - dbeta / M) - xh * (dgamma / M))    eval: gx = gamma * invstd * gu
//
// Work split.  A plane [H*W] is cut into SEGMENTS of BNT_SEG = 2048 consecutive elements (the last may be
// shorter); a segment of a plane is a UNIT and belongs to ONE wave, in every kernel.  A unit is cut into
// chunks of V = 4 float32 / 8 half elements (16 bytes); lane t of the wave owns chunks t, t + 64, ... of
// the segment (at most BNT_KCH = 8 / 4).  VECTOR route: a chunk is one 16-byte access; ELEMENT route: the
// SAME lane touches the SAME chunk element by element (any H*W, any element-aligned pointer; what lies
// behind the plane counts as +0 in the sums and is not written), so both routes give the same bits.
// A channel has U = B * ceil(H*W / 2048) units, u = b * segments + segment.  The reduction kernels
// (k_bntail_stats, k_bntail_bwd_reduce) write one partial per unit into the caller's workspace
// `part` [C, U, 2]; the kernel behind them (k_bntail_apply, k_bntail_bwd_apply) merges the U partials
// of its channel in every wave, in a fixed order, so nothing is handed between workgroups inside a launch,
// there is no atomic and no barrier.  The wave of unit 0 of a channel writes the channel's results (saved
// mean and invstd, the running statistics, dgamma and dbeta).  k_bntail_bwd_reduce with dgamma / dbeta given
// finishes alone (no apply follows): ONE workgroup owns a channel, its four waves take the units in turn,
// and after a barrier wave 0 merges the partials the workgroup itself wrote, in the same order.
// Grids: min(items, BNT_BLOCKS_PER_CU per compute unit of nmsa_device_geometry) workgroups of four waves,
// looping over the rest; an item is four consecutive units (a channel when the reduce finishes alone).
// Addressing: 32-bit, B*C*H*W < 2^31 is checked.  The arithmetic contract is stated in include/nmsa.h.
#include "nmsa_common.hpp"
#include <math.h>

namespace nmsa {
namespace {

constexpr int BNT_THREADS = 256;
constexpr int BNT_WAVES = BNT_THREADS / kWave;
constexpr int BNT_SEG = NMSA_BNTAIL_SEGMENT;
constexpr int BNT_BLOCKS_PER_CU = 8;

// elem, ld, st, pack: nmsa_common.hpp

__device__ __forceinline__ float bnt_sigmoid(float z)
{
    return __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-z)));
}

template <int ACT>
__device__ __forceinline__ float bnt_act(float z)
{
    if constexpr (ACT == NMSA_BNTAIL_ACT_RELU) return z <= 0.0f ? 0.0f : z;     // a NaN passes, as torch.relu's
    else return __fmul_rn(z, bnt_sigmoid(z));
}

// SiLU'(z) = sig * (1 + z * (1 - sig))
__device__ __forceinline__ float bnt_silu_grad(float z)
{
    const float sg = bnt_sigmoid(z);
    return __fmul_rn(sg, __fadd_rn(1.0f, __fmul_rn(z, __fsub_rn(1.0f, sg))));
}

// V elements of a plane of HW elements from element e as float32; ELEMENT route: what lies behind the
// plane is +0.  The caller has checked e < HW.
template <int DTYPE, bool VECTOR>
__device__ __forceinline__ void bnt_load(const typename elem<DTYPE>::type* plane, uint32_t e, uint32_t HW, float* out)
{
    typedef typename elem<DTYPE>::type S;
    constexpr int V = 16 / sizeof(S);
    if constexpr (VECTOR) {
        const pack<S, V> p = *(const pack<S, V>*)(plane + e);
#pragma unroll
        for (int j = 0; j < V; ++j) out[j] = ld<DTYPE>(p.v[j]);
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) out[j] = e + j < HW ? ld<DTYPE>(plane[e + j]) : 0.0f;
    }
}

template <int DTYPE, bool VECTOR>
__device__ __forceinline__ void bnt_store(typename elem<DTYPE>::type* plane, uint32_t e, uint32_t HW, const float* in)
{
    typedef typename elem<DTYPE>::type S;
    constexpr int V = 16 / sizeof(S);
    if constexpr (VECTOR) {
        pack<S, V> p;
#pragma unroll
        for (int j = 0; j < V; ++j) p.v[j] = st<DTYPE>(in[j]);
        *(pack<S, V>*)(plane + e) = p;
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (e + j < HW) plane[e + j] = st<DTYPE>(in[j]);
    }
}

// a lane's V partial sums pairwise (a0 + a1) + (a2 + a3) ..., then the lanes of the wave by halves
// (lane l += lane l + 32, 16, ..., 1); the sum is handed to every lane
template <int V>
__device__ __forceinline__ float bnt_wave_sum(float* a)
{
#pragma unroll
    for (int st = 1; st < V; st *= 2)
#pragma unroll
        for (int j = 0; j < V; j += 2 * st) a[j] = __fadd_rn(a[j], a[j + st]);
    return __shfl(wave_reduce_sum(a[0]), 0);
}

// where a unit lies: g = (b * C + c) * nseg + segment
struct BntUnit {
    uint32_t plane, c, u, e0;   // plane b * C + c, channel, unit of the channel, first element in the plane
};

__device__ __forceinline__ BntUnit bnt_unit(uint32_t g, uint32_t C, uint32_t nseg)
{
    BntUnit r;
    r.plane = g / nseg;
    const uint32_t seg = g - r.plane * nseg, b = r.plane / C;
    r.c = r.plane - b * C;
    r.u = b * nseg + seg;
    r.e0 = seg * BNT_SEG;
    return r;
}

// elements of unit u of a channel
__device__ __forceinline__ float bnt_count(uint32_t u, uint32_t nseg, uint32_t HW)
{
    const uint32_t e0 = (u % nseg) * BNT_SEG, left = HW - e0;
    return (float)(left < (uint32_t)BNT_SEG ? left : (uint32_t)BNT_SEG);
}

// (na, ma, qa) <- (na, ma, qa) merged with (nb, mb, qb): count, mean, sum of squared deviations (Chan et al.)
__device__ __forceinline__ void bnt_chan(float& na, float& ma, float& qa, float nb, float mb, float qb)
{
    if (nb == 0.0f) return;
    if (na == 0.0f) { na = nb; ma = mb; qa = qb; return; }
    const float n = __fadd_rn(na, nb), d = __fsub_rn(mb, ma), r = __fdiv_rn(nb, n);
    ma = __fadd_rn(ma, __fmul_rn(d, r));
    qa = __fadd_rn(__fadd_rn(qa, qb), __fmul_rn(__fmul_rn(d, d), __fmul_rn(na, r)));
    na = n;
}

// mean and sum of squared deviations of a channel from its U unit partials (mean_u, M2_u): lane l merges the
// units l, l + 64, ... in ascending order, then the lanes by halves; every lane gets the result
__device__ __forceinline__ void bnt_merge_stats(const float* part_c, uint32_t U, uint32_t nseg, uint32_t HW,
                                                float& mean, float& m2)
{
    float n = 0.0f, m = 0.0f, q = 0.0f;
    for (uint32_t u = lane_id(); u < U; u += kWave) bnt_chan(n, m, q, bnt_count(u, nseg, HW), part_c[2 * u], part_c[2 * u + 1]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float nb = __shfl_down(n, o), mb = __shfl_down(m, o), qb = __shfl_down(q, o);
        if (lane_id() + o < kWave) bnt_chan(n, m, q, nb, mb, qb);
    }
    mean = __shfl(m, 0);
    m2 = __shfl(q, 0);
}

// the two sums of a channel from its U unit partials (sum gu, sum gu * xh), in the order of bnt_merge_stats
__device__ __forceinline__ void bnt_merge_sums(const float* part_c, uint32_t U, float& dbeta, float& dgamma)
{
    float a = 0.0f, b = 0.0f;
    for (uint32_t u = lane_id(); u < U; u += kWave) {
        a = __fadd_rn(a, part_c[2 * u]);
        b = __fadd_rn(b, part_c[2 * u + 1]);
    }
    dbeta = __shfl(wave_reduce_sum(a), 0);
    dgamma = __shfl(wave_reduce_sum(b), 0);
}

// ------------------------------------------------------------------------------------ statistics
// part[c, u] = (mean_u, M2_u) of the unit: the unit's values stay in registers; mean_u = S / n_u (IEEE
// division) with S summed per chunk position in ascending chunk order, then as in bnt_wave_sum;
// M2_u = sum (x - mean_u)^2 as fused multiply-adds from 0 in the same order
template <int DTYPE, bool VECTOR>
__global__ __launch_bounds__(BNT_THREADS) void k_bntail_stats(
    const typename elem<DTYPE>::type* __restrict__ x, float* __restrict__ part, const uint32_t HW,
    const uint32_t C, const uint32_t nseg, const uint32_t U, const uint32_t units, const uint32_t items)
{
    typedef typename elem<DTYPE>::type S;
    constexpr int V = 16 / sizeof(S);
    constexpr int KCH = BNT_SEG / (kWave * V);
    for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t g = item * BNT_WAVES + threadIdx.x / kWave;
        if (g >= units) continue;                                   // wave-uniform, no barrier in this kernel
        const BntUnit t = bnt_unit(g, C, nseg);
        const S* src = x + (size_t)t.plane * HW;
        float v[KCH][V], a[V];
#pragma unroll
        for (int j = 0; j < V; ++j) a[j] = 0.0f;
#pragma unroll
        for (int k = 0; k < KCH; ++k) {
            const uint32_t e = t.e0 + (uint32_t)(lane_id() + kWave * k) * V;
            if (e < HW) bnt_load<DTYPE, VECTOR>(src, e, HW, v[k]);
            else
#pragma unroll
                for (int j = 0; j < V; ++j) v[k][j] = 0.0f;
#pragma unroll
            for (int j = 0; j < V; ++j) a[j] = __fadd_rn(a[j], v[k][j]);
        }
        const float mean = __fdiv_rn(bnt_wave_sum<V>(a), bnt_count(t.u, nseg, HW));
#pragma unroll
        for (int j = 0; j < V; ++j) a[j] = 0.0f;
#pragma unroll
        for (int k = 0; k < KCH; ++k) {
            const uint32_t e = t.e0 + (uint32_t)(lane_id() + kWave * k) * V;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float d = e + j < HW ? __fsub_rn(v[k][j], mean) : 0.0f;
                a[j] = __fmaf_rn(d, d, a[j]);
            }
        }
        const float m2 = bnt_wave_sum<V>(a);
        if (lane_id() == 0) {
            float* dst = part + ((size_t)t.c * U + t.u) * 2;
            dst[0] = mean;
            dst[1] = m2;
        }
    }
}

// what every wave of the two apply kernels and of the backward reduction knows about its plane
struct BntChannel {
    float mean, invstd, gamma, beta, scale;
};

struct BntFwdArgs {
    const float* gamma;
    const float* beta;
    const float* part;          // training: the unit partials of k_bntail_stats; NULL: eval
    float* running_mean;        // training: updated; eval: read
    float* running_var;
    float* save_mean;           // NULL: not wanted
    float* save_invstd;
    float eps, momentum, count; // count = float(M)
    float unbias;               // float(M - 1)
};

// --------------------------------------------------------------------------------------- apply
// xh = (x - mean) * invstd; u = xh * gamma + beta; v = u * s; z = v + id; y = act(z): every operation
// rounded to float32, y rounded once to the maps' dtype.  training: var = M2 / float(M), the running
// statistics rm = (1 - m) * rm + m * mean, rv = (1 - m) * rv + m * (M2 / float(M - 1)); invstd = 1 / sqrt(var + eps),
// IEEE square root and division
template <int DTYPE, bool VECTOR, int ACT>
__global__ __launch_bounds__(BNT_THREADS) void k_bntail_apply(
    const typename elem<DTYPE>::type* __restrict__ x, const typename elem<DTYPE>::type* __restrict__ identity,
    const typename elem<DTYPE>::type* __restrict__ scale, const BntFwdArgs p,
    typename elem<DTYPE>::type* __restrict__ y, const uint32_t HW, const uint32_t C, const uint32_t nseg,
    const uint32_t U, const uint32_t units, const uint32_t items)
{
    typedef typename elem<DTYPE>::type S;
    constexpr int V = 16 / sizeof(S);
    constexpr int KCH = BNT_SEG / (kWave * V);
    for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t g = item * BNT_WAVES + threadIdx.x / kWave;
        if (g >= units) continue;
        const BntUnit t = bnt_unit(g, C, nseg);
        float mean, var, m2 = 0.0f;
        if (p.part) {
            bnt_merge_stats(p.part + (size_t)t.c * U * 2, U, nseg, HW, mean, m2);
            var = __fdiv_rn(m2, p.count);
        } else {
            mean = p.running_mean[t.c];
            var = p.running_var[t.c];
        }
        const float invstd = __fdiv_rn(1.0f, __fsqrt_rn(__fadd_rn(var, p.eps)));
        if (t.u == 0 && lane_id() == 0) {
            if (p.save_mean) {
                p.save_mean[t.c] = mean;
                p.save_invstd[t.c] = invstd;
            }
            if (p.part) {
                const float keep = __fsub_rn(1.0f, p.momentum);
                p.running_mean[t.c] = __fadd_rn(__fmul_rn(keep, p.running_mean[t.c]), __fmul_rn(p.momentum, mean));
                p.running_var[t.c] = __fadd_rn(__fmul_rn(keep, p.running_var[t.c]),
                                               __fmul_rn(p.momentum, __fdiv_rn(m2, p.unbias)));
            }
        }
        const float gamma = p.gamma[t.c], beta = p.beta[t.c];
        const float sc = scale ? ld<DTYPE>(scale[t.plane]) : 1.0f;
        const S* xs = x + (size_t)t.plane * HW;
        const S* is = identity ? identity + (size_t)t.plane * HW : nullptr;
        S* ys = y + (size_t)t.plane * HW;
#pragma unroll
        for (int k = 0; k < KCH; ++k) {
            const uint32_t e = t.e0 + (uint32_t)(lane_id() + kWave * k) * V;
            if (e >= HW) continue;
            float vx[V], vi[V], r[V];
            bnt_load<DTYPE, VECTOR>(xs, e, HW, vx);
            if (is) bnt_load<DTYPE, VECTOR>(is, e, HW, vi);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float xh = __fmul_rn(__fsub_rn(vx[j], mean), invstd);
                float z = __fadd_rn(__fmul_rn(xh, gamma), beta);
                if (scale) z = __fmul_rn(z, sc);
                if (is) z = __fadd_rn(z, vi[j]);
                r[j] = bnt_act<ACT>(z);
            }
            bnt_store<DTYPE, VECTOR>(ys, e, HW, r);
        }
    }
}

// ------------------------------------------------------------------------------------ backward
struct BntBwdArgs {
    const float* gamma;
    const float* beta;          // SiLU only (z is recomputed)
    const float* mean;          // the saved statistics of the forward pass
    const float* invstd;
    float* dgamma;              // NULL: not wanted
    float* dbeta;
    float count;                // float(M)
};

// gz and gu of V elements; `aux` is y under ReLU (the gate: 0 where y <= 0) and the identity (NULL: absent) under
// SiLU (z = (xh * gamma + beta) * s + id is recomputed as the forward pass computed it)
template <int ACT, int V>
__device__ __forceinline__ void bnt_grad(const float* gy, const float* xh, const float* aux, bool has_aux,
                                         bool has_scale, const BntChannel& ch, float* gz, float* gu)
{
#pragma unroll
    for (int j = 0; j < V; ++j) {
        if constexpr (ACT == NMSA_BNTAIL_ACT_RELU) {
            gz[j] = aux[j] <= 0.0f ? 0.0f : gy[j];                  // ATen's threshold backward: a NaN y passes gy
        } else {
            float z = __fadd_rn(__fmul_rn(xh[j], ch.gamma), ch.beta);
            if (has_scale) z = __fmul_rn(z, ch.scale);
            if (has_aux) z = __fadd_rn(z, aux[j]);
            gz[j] = __fmul_rn(gy[j], bnt_silu_grad(z));
        }
        gu[j] = has_scale ? __fmul_rn(gz[j], ch.scale) : gz[j];
    }
}

// the two sums of a unit: per chunk position in ascending chunk order from 0 (sum gu as additions,
// sum gu * xh as fused multiply-adds), then as in bnt_wave_sum
template <int DTYPE, bool VECTOR, int ACT>
__device__ __forceinline__ void bnt_bwd_unit(
    const typename elem<DTYPE>::type* gy, const typename elem<DTYPE>::type* x,
    const typename elem<DTYPE>::type* aux, const BntUnit& t, uint32_t HW, bool has_scale, const BntChannel& ch,
    float& sum_gu, float& sum_gux)
{
    typedef typename elem<DTYPE>::type S;
    constexpr int V = 16 / sizeof(S);
    constexpr int KCH = BNT_SEG / (kWave * V);
    const S* gs = gy + (size_t)t.plane * HW;
    const S* xs = x + (size_t)t.plane * HW;
    const S* as = aux ? aux + (size_t)t.plane * HW : nullptr;
    float a1[V], a2[V];
#pragma unroll
    for (int j = 0; j < V; ++j) a1[j] = a2[j] = 0.0f;
#pragma unroll
    for (int k = 0; k < KCH; ++k) {
        const uint32_t e = t.e0 + (uint32_t)(lane_id() + kWave * k) * V;
        if (e >= HW) continue;
        float vg[V], vx[V], va[V], gz[V], gu[V];
        bnt_load<DTYPE, VECTOR>(gs, e, HW, vg);
        bnt_load<DTYPE, VECTOR>(xs, e, HW, vx);
        if (as) bnt_load<DTYPE, VECTOR>(as, e, HW, va);
#pragma unroll
        for (int j = 0; j < V; ++j) vx[j] = __fmul_rn(__fsub_rn(vx[j], ch.mean), ch.invstd);
        bnt_grad<ACT, V>(vg, vx, va, as != nullptr, has_scale, ch, gz, gu);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            a1[j] = __fadd_rn(a1[j], gu[j]);
            a2[j] = __fmaf_rn(gu[j], vx[j], a2[j]);
        }
    }
    sum_gu = bnt_wave_sum<V>(a1);
    sum_gux = bnt_wave_sum<V>(a2);
}

template <int DTYPE>
__device__ __forceinline__ BntChannel bnt_channel(const BntBwdArgs& p, const typename elem<DTYPE>::type* scale,
                                                  const BntUnit& t, bool silu)
{
    BntChannel ch;
    ch.mean = p.mean[t.c];
    ch.invstd = p.invstd[t.c];
    ch.gamma = p.gamma[t.c];
    ch.beta = silu ? p.beta[t.c] : 0.0f;
    ch.scale = scale ? ld<DTYPE>(scale[t.plane]) : 1.0f;
    return ch;
}

// part[c, u] = (sum gu, sum gu * xh) of the unit.  With p.dgamma / p.dbeta the kernel finishes alone: a
// workgroup owns a channel (item = channel), and wave 0 merges what the workgroup wrote
template <int DTYPE, bool VECTOR, int ACT>
__global__ __launch_bounds__(BNT_THREADS) void k_bntail_bwd_reduce(
    const typename elem<DTYPE>::type* __restrict__ gy, const typename elem<DTYPE>::type* __restrict__ x,
    const typename elem<DTYPE>::type* __restrict__ aux, const typename elem<DTYPE>::type* __restrict__ scale,
    const BntBwdArgs p, float* part, const uint32_t HW, const uint32_t C, const uint32_t nseg, const uint32_t U,
    const uint32_t units, const uint32_t items)
{
    constexpr bool SILU = ACT == NMSA_BNTAIL_ACT_SILU;
    const uint32_t wave = threadIdx.x / kWave;
    if (!p.dgamma) {
        for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
            const uint32_t g = item * BNT_WAVES + wave;
            if (g >= units) continue;
            const BntUnit t = bnt_unit(g, C, nseg);
            const BntChannel ch = bnt_channel<DTYPE>(p, scale, t, SILU);
            float s1, s2;
            bnt_bwd_unit<DTYPE, VECTOR, ACT>(gy, x, aux, t, HW, scale != nullptr, ch, s1, s2);
            if (lane_id() == 0) {
                float* dst = part + ((size_t)t.c * U + t.u) * 2;
                dst[0] = s1;
                dst[1] = s2;
            }
        }
        return;
    }
    for (uint32_t c = blockIdx.x; c < items; c += gridDim.x) {     // items == C: workgroup-uniform trips
        for (uint32_t u = wave; u < U; u += BNT_WAVES) {
            const uint32_t b = u / nseg;
            const BntUnit t = bnt_unit((b * C + c) * nseg + (u - b * nseg), C, nseg);
            const BntChannel ch = bnt_channel<DTYPE>(p, scale, t, SILU);
            float s1, s2;
            bnt_bwd_unit<DTYPE, VECTOR, ACT>(gy, x, aux, t, HW, scale != nullptr, ch, s1, s2);
            if (lane_id() == 0) {
                float* dst = part + ((size_t)c * U + u) * 2;
                dst[0] = s1;
                dst[1] = s2;
            }
        }
        __syncthreads();                                            // the workgroup's own partials, its own channel
        if (wave == 0) {
            float db, dg;
            bnt_merge_sums(part + (size_t)c * U * 2, U, db, dg);
            if (lane_id() == 0) {
                p.dgamma[c] = dg;
                p.dbeta[c] = db;
            }
        }
    }
}

// gx = (gamma * invstd) * ((gu - dbeta / float(M)) - xh * (dgamma / float(M))) with part (training),
// gx = (gamma * invstd) * gu without (eval); gid = gz; every operation rounded to float32, IEEE divisions;
// a NULL gx / gid is not wanted
template <int DTYPE, bool VECTOR, int ACT>
__global__ __launch_bounds__(BNT_THREADS) void k_bntail_bwd_apply(
    const typename elem<DTYPE>::type* __restrict__ gy, const typename elem<DTYPE>::type* __restrict__ x,
    const typename elem<DTYPE>::type* __restrict__ aux, const typename elem<DTYPE>::type* __restrict__ scale,
    const BntBwdArgs p, const float* __restrict__ part, typename elem<DTYPE>::type* __restrict__ gx,
    typename elem<DTYPE>::type* __restrict__ gid, const uint32_t HW, const uint32_t C, const uint32_t nseg,
    const uint32_t U, const uint32_t units, const uint32_t items)
{
    typedef typename elem<DTYPE>::type S;
    constexpr int V = 16 / sizeof(S);
    constexpr int KCH = BNT_SEG / (kWave * V);
    constexpr bool SILU = ACT == NMSA_BNTAIL_ACT_SILU;
    for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t g = item * BNT_WAVES + threadIdx.x / kWave;
        if (g >= units) continue;
        const BntUnit t = bnt_unit(g, C, nseg);
        const BntChannel ch = bnt_channel<DTYPE>(p, scale, t, SILU);
        float qb = 0.0f, qg = 0.0f;
        if (part) {
            float db, dg;
            bnt_merge_sums(part + (size_t)t.c * U * 2, U, db, dg);
            if (t.u == 0 && lane_id() == 0 && p.dgamma) {
                p.dgamma[t.c] = dg;
                p.dbeta[t.c] = db;
            }
            qb = __fdiv_rn(db, p.count);
            qg = __fdiv_rn(dg, p.count);
        }
        const float kx = __fmul_rn(ch.gamma, ch.invstd);
        const S* gs = gy + (size_t)t.plane * HW;
        const S* xs = x + (size_t)t.plane * HW;
        const S* as = aux ? aux + (size_t)t.plane * HW : nullptr;
        S* gxs = gx ? gx + (size_t)t.plane * HW : nullptr;
        S* gis = gid ? gid + (size_t)t.plane * HW : nullptr;
#pragma unroll
        for (int k = 0; k < KCH; ++k) {
            const uint32_t e = t.e0 + (uint32_t)(lane_id() + kWave * k) * V;
            if (e >= HW) continue;
            float vg[V], vx[V], va[V], gz[V], gu[V];
            bnt_load<DTYPE, VECTOR>(gs, e, HW, vg);
            bnt_load<DTYPE, VECTOR>(xs, e, HW, vx);
            if (as) bnt_load<DTYPE, VECTOR>(as, e, HW, va);
#pragma unroll
            for (int j = 0; j < V; ++j) vx[j] = __fmul_rn(__fsub_rn(vx[j], ch.mean), ch.invstd);
            bnt_grad<ACT, V>(vg, vx, va, as != nullptr, scale != nullptr, ch, gz, gu);
            if (gis) bnt_store<DTYPE, VECTOR>(gis, e, HW, gz);
            if (gxs) {
#pragma unroll
                for (int j = 0; j < V; ++j)
                    gu[j] = part ? __fmul_rn(kx, __fsub_rn(__fsub_rn(gu[j], qb), __fmul_rn(vx[j], qg)))
                                 : __fmul_rn(kx, gu[j]);
                bnt_store<DTYPE, VECTOR>(gxs, e, HW, gu);
            }
        }
    }
}

// ------------------------------------------------------------------------------------ host side
bool bnt_f32(const void* p) { return aligned(p, 4); }
int bnt_vec(int dtype) { return dtype == NMSA_F32 ? 4 : 8; }

bool bnt_sizes_ok(int dtype, int B, int C, int H, int W)
{
    if (dtype != NMSA_F32 && dtype != NMSA_BF16 && dtype != NMSA_F16) return false;
    if (B < 1 || C < 1 || H < 1 || W < 1) return false;
    return (int64_t)B * C * (int64_t)H * W <= 0x7fffffffLL;        // 32-bit offsets
}

bool bnt_act_ok(int act) { return act == NMSA_BNTAIL_ACT_RELU || act == NMSA_BNTAIL_ACT_SILU; }

struct BntShape {
    uint32_t HW, C, nseg, U, units, items;
};

BntShape bnt_shape(int B, int C, int H, int W)
{
    BntShape s;
    s.HW = (uint32_t)(H * W);
    s.C = (uint32_t)C;
    s.nseg = (s.HW + BNT_SEG - 1) / BNT_SEG;
    s.U = (uint32_t)B * s.nseg;
    s.units = s.U * s.C;
    s.items = (s.units + BNT_WAVES - 1) / BNT_WAVES;
    return s;
}

size_t bnt_part_bytes(int B, int C, int H, int W)
{
    const BntShape s = bnt_shape(B, C, H, W);
    return (size_t)s.units * 2 * sizeof(float);
}

// THE route rule: 16-byte accesses need whole vectors per plane and every map of the call on 16 bytes
// (a NULL map is not part of the call)
bool bnt_vector(const void* const* maps, int n, int dtype, int64_t HW)
{
    if (HW % bnt_vec(dtype) != 0) return false;
    for (int i = 0; i < n; ++i)
        if (!aligned(maps[i], 16)) return false;
    return true;
}

}  // namespace
}  // namespace nmsa

// run LAUNCH(<dtype constant>, <vector route>, <activation constant>)
#define BNT_DISPATCH(DT, LAUNCH)                                        \
    do {                                                                \
        if (vector && act == NMSA_BNTAIL_ACT_RELU) LAUNCH(DT, true, NMSA_BNTAIL_ACT_RELU);  \
        else if (vector) LAUNCH(DT, true, NMSA_BNTAIL_ACT_SILU);        \
        else if (act == NMSA_BNTAIL_ACT_RELU) LAUNCH(DT, false, NMSA_BNTAIL_ACT_RELU);      \
        else LAUNCH(DT, false, NMSA_BNTAIL_ACT_SILU);                   \
    } while (0)

extern "C" size_t nmsa_bntail_workspace_bytes(int B, int C, int H, int W)
{
    using namespace nmsa;
    if (!bnt_sizes_ok(NMSA_F32, B, C, H, W)) return 0;
    return bnt_part_bytes(B, C, H, W);
}

extern "C" int nmsa_bntail_route(const void* t0, const void* t1, const void* t2, const void* t3, const void* t4,
                                 int dtype, int H, int W, int* segments)
{
    using namespace nmsa;
    if (!bnt_sizes_ok(dtype, 1, 1, H, W)) return NMSA_ERR_ARG;
    const void* maps[5] = {t0, t1, t2, t3, t4};
    if (!t0) return NMSA_ERR_ARG;
    for (int i = 0; i < 5; ++i)
        if (!elem_aligned(maps[i], dtype)) return NMSA_ERR_ARG;
    if (segments) *segments = (int)bnt_shape(1, 1, H, W).nseg;
    return bnt_vector(maps, 5, dtype, (int64_t)H * W) ? NMSA_BNTAIL_ROUTE_VECTOR : NMSA_BNTAIL_ROUTE_ELEMENT;
}

extern "C" int nmsa_bntail_stats(const void* x, int dtype, int B, int C, int H, int W, float* part, size_t part_bytes,
                                 nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    if (!bnt_sizes_ok(dtype, B, C, H, W)) return NMSA_ERR_ARG;
    if (!x || !part || !elem_aligned(x, dtype) || !bnt_f32(part)) return NMSA_ERR_ARG;
    if (part_bytes < bnt_part_bytes(B, C, H, W)) return NMSA_ERR_ARG;
    const BntShape s = bnt_shape(B, C, H, W);
    const void* maps[1] = {x};
    const bool vector = bnt_vector(maps, 1, dtype, s.HW);
    const dim3 grid(capped_grid(s.items, BNT_BLOCKS_PER_CU)), block(BNT_THREADS);
#define BNT_STATS(DT)                                                                                            \
    do {                                                                                                         \
        typedef elem<DT>::type S;                                                                                \
        if (vector)                                                                                              \
            hipLaunchKernelGGL((k_bntail_stats<DT, true>), grid, block, 0, stream, (const S*)x, part, s.HW, s.C, \
                               s.nseg, s.U, s.units, s.items);                                                   \
        else                                                                                                     \
            hipLaunchKernelGGL((k_bntail_stats<DT, false>), grid, block, 0, stream, (const S*)x, part, s.HW, s.C, \
                               s.nseg, s.U, s.units, s.items);                                                   \
    } while (0)
    NMSA_DISPATCH_DTYPE(dtype, BNT_STATS)
#undef BNT_STATS
    return check_launch();
}

extern "C" int nmsa_bntail_apply(const void* x, const void* identity, const void* scale, int dtype, int B, int C, int H,
                                 int W, const float* gamma, const float* beta, const float* part, size_t part_bytes,
                                 float* running_mean, float* running_var, float eps, float momentum, int act,
                                 float* save_mean, float* save_invstd, void* y, nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    if (!bnt_sizes_ok(dtype, B, C, H, W) || !bnt_act_ok(act)) return NMSA_ERR_ARG;
    if (!x || !y || !gamma || !beta || !running_mean || !running_var) return NMSA_ERR_ARG;
    if (!elem_aligned(x, dtype) || !elem_aligned(identity, dtype) || !elem_aligned(scale, dtype) || !elem_aligned(y, dtype))
        return NMSA_ERR_ARG;
    if (!bnt_f32(gamma) || !bnt_f32(beta) || !bnt_f32(part) || !bnt_f32(running_mean) || !bnt_f32(running_var) ||
        !bnt_f32(save_mean) || !bnt_f32(save_invstd))
        return NMSA_ERR_ARG;
    if (!save_mean != !save_invstd) return NMSA_ERR_ARG;
    if (part && part_bytes < bnt_part_bytes(B, C, H, W)) return NMSA_ERR_ARG;
    if (part && (int64_t)B * H * W < 2) return NMSA_ERR_ARG;        // no unbiased variance of one value
    const BntShape s = bnt_shape(B, C, H, W);
    const void* maps[3] = {x, identity, y};
    const bool vector = bnt_vector(maps, 3, dtype, s.HW);
    const double M = (double)B * H * W;
    const BntFwdArgs p = {gamma, beta, part, running_mean, running_var, save_mean, save_invstd,
                          eps, momentum, (float)M, (float)(M - 1.0)};
    const dim3 grid(capped_grid(s.items, BNT_BLOCKS_PER_CU)), block(BNT_THREADS);
#define BNT_APPLY_ONE(DT, VECTOR, ACT)                                                                         \
    hipLaunchKernelGGL((k_bntail_apply<DT, VECTOR, ACT>), grid, block, 0, stream, (const elem<DT>::type*)x,    \
                       (const elem<DT>::type*)identity, (const elem<DT>::type*)scale, p,                       \
                       (elem<DT>::type*)y, s.HW, s.C, s.nseg, s.U, s.units, s.items)
#define BNT_APPLY(DT) BNT_DISPATCH(DT, BNT_APPLY_ONE)
    NMSA_DISPATCH_DTYPE(dtype, BNT_APPLY)
#undef BNT_APPLY
#undef BNT_APPLY_ONE
    return check_launch();
}

namespace nmsa {
namespace {
// the checks the two backward entry points share
int bnt_bwd_check(const void* gy, const void* x, const void* aux, const void* scale, int dtype, int B, int C, int H,
                  int W, const float* gamma, const float* beta, const float* mean, const float* invstd, int act)
{
    if (!bnt_sizes_ok(dtype, B, C, H, W) || !bnt_act_ok(act)) return NMSA_ERR_ARG;
    if (!gy || !x || !gamma || !mean || !invstd) return NMSA_ERR_ARG;
    if (act == NMSA_BNTAIL_ACT_RELU ? !aux : !beta) return NMSA_ERR_ARG;     // y is the gate; z needs beta
    if (!elem_aligned(gy, dtype) || !elem_aligned(x, dtype) || !elem_aligned(aux, dtype) || !elem_aligned(scale, dtype))
        return NMSA_ERR_ARG;
    if (!bnt_f32(gamma) || !bnt_f32(beta) || !bnt_f32(mean) || !bnt_f32(invstd)) return NMSA_ERR_ARG;
    return NMSA_OK;
}
}  // namespace
}  // namespace nmsa

extern "C" int nmsa_bntail_bwd_reduce(const void* gy, const void* x, const void* aux, const void* scale, int dtype,
                                      int B, int C, int H, int W, const float* gamma, const float* beta,
                                      const float* mean, const float* invstd, int act, float* part, size_t part_bytes,
                                      float* dgamma, float* dbeta, nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = bnt_bwd_check(gy, x, aux, scale, dtype, B, C, H, W, gamma, beta, mean, invstd, act);
    if (rc != NMSA_OK) return rc;
    if (!part || !bnt_f32(part) || !bnt_f32(dgamma) || !bnt_f32(dbeta) || !dgamma != !dbeta) return NMSA_ERR_ARG;
    if (part_bytes < bnt_part_bytes(B, C, H, W)) return NMSA_ERR_ARG;
    const BntShape s = bnt_shape(B, C, H, W);
    const void* maps[3] = {gy, x, aux};
    const bool vector = bnt_vector(maps, 3, dtype, s.HW);
    const BntBwdArgs p = {gamma, beta, mean, invstd, dgamma, dbeta, (float)((double)B * H * W)};
    const uint32_t items = dgamma ? s.C : s.items;
    const dim3 grid(capped_grid(items, BNT_BLOCKS_PER_CU)), block(BNT_THREADS);
#define BNT_REDUCE_ONE(DT, VECTOR, ACT)                                                                             \
    hipLaunchKernelGGL((k_bntail_bwd_reduce<DT, VECTOR, ACT>), grid, block, 0, stream, (const elem<DT>::type*)gy,   \
                       (const elem<DT>::type*)x, (const elem<DT>::type*)aux, (const elem<DT>::type*)scale,          \
                       p, part, s.HW, s.C, s.nseg, s.U, s.units, items)
#define BNT_REDUCE(DT) BNT_DISPATCH(DT, BNT_REDUCE_ONE)
    NMSA_DISPATCH_DTYPE(dtype, BNT_REDUCE)
#undef BNT_REDUCE
#undef BNT_REDUCE_ONE
    return check_launch();
}

extern "C" int nmsa_bntail_bwd_apply(const void* gy, const void* x, const void* aux, const void* scale, int dtype,
                                     int B, int C, int H, int W, const float* gamma, const float* beta,
                                     const float* mean, const float* invstd, int act, const float* part,
                                     size_t part_bytes, void* gx, void* gid, float* dgamma, float* dbeta,
                                     nmsa_stream_t stream_)
{
    using namespace nmsa;
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = bnt_bwd_check(gy, x, aux, scale, dtype, B, C, H, W, gamma, beta, mean, invstd, act);
    if (rc != NMSA_OK) return rc;
    if (!elem_aligned(gx, dtype) || !elem_aligned(gid, dtype) || !bnt_f32(part) || !bnt_f32(dgamma) || !bnt_f32(dbeta) ||
        !dgamma != !dbeta)
        return NMSA_ERR_ARG;
    if (dgamma && !part) return NMSA_ERR_ARG;                       // the sums come from the partials
    if (part && part_bytes < bnt_part_bytes(B, C, H, W)) return NMSA_ERR_ARG;
    if (!gx && !gid && !dgamma) return NMSA_OK;
    const BntShape s = bnt_shape(B, C, H, W);
    const void* maps[5] = {gy, x, aux, gx, gid};
    const bool vector = bnt_vector(maps, 5, dtype, s.HW);
    const BntBwdArgs p = {gamma, beta, mean, invstd, dgamma, dbeta, (float)((double)B * H * W)};
    const dim3 grid(capped_grid(s.items, BNT_BLOCKS_PER_CU)), block(BNT_THREADS);
#define BNT_BAPPLY_ONE(DT, VECTOR, ACT)                                                                            \
    hipLaunchKernelGGL((k_bntail_bwd_apply<DT, VECTOR, ACT>), grid, block, 0, stream, (const elem<DT>::type*)gy,   \
                       (const elem<DT>::type*)x, (const elem<DT>::type*)aux, (const elem<DT>::type*)scale,         \
                       p, part, (elem<DT>::type*)gx, (elem<DT>::type*)gid, s.HW, s.C, s.nseg, s.U, s.units,        \
                       s.items)
#define BNT_BAPPLY(DT) BNT_DISPATCH(DT, BNT_BAPPLY_ONE)
    NMSA_DISPATCH_DTYPE(dtype, BNT_BAPPLY)
#undef BNT_BAPPLY
#undef BNT_BAPPLY_ONE
    return check_launch();
}
