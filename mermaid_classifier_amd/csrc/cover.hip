// cover.hip -- cover estimation on the device (gfx950): the kernels behind mmc_cover_proba / mmc_head_cover(_set).
// include/mmc.h, section "cover estimation", is the definition; this file follows it.
//
// Input: a resident n x K fp32 matrix of calibrated probabilities (rows = points) and contiguous groups of rows (images, transects,
// sources) given by offsets.  Per group: the argmax counts (cover.py's predicted counts), the order-free 2^-32 fixed-point sum of
// the probabilities, and the class prior re-estimated by EM (Saerens, Latinne and Decaestecker 2002) with a Dirichlet pseudo-count;
// per point, optionally, the k best classes of the posterior under the group's adapted prior.
//
// cover_count_kernel      one thread per point: usable check, first argmax, K fixed-point terms.  Integer atomics only.  A workgroup
//                         owns 256 consecutive rows, which lie in a contiguous run of groups; when that run's tables fit
//                         (COVER_LDS_ENTRIES) they are kept in LDS and flushed with one atomic per touched entry, so a source-sized
//                         group does not send every row to the same K counters in memory.
// cover_em_pass_kernel    the E-step.  The host cuts every group into slabs of at most COVER_SLAB_POINTS consecutive points (a slab
//                         never spans two groups, so the slab list is a function of the offsets alone).  One wave per slab, lane l
//                         owns classes l, l + 64, ...: the group's weights w = pi / train_prior in registers, per point one coalesced
//                         read of the row, Z by a fixed xor-butterfly, q = v w / Z added to the lane's fp64 accumulators in point
//                         order.  Each slab writes K doubles.  (K > 512: cover_em_pass_wide_kernel, accumulators in the slab's own
//                         output row.)
// cover_em_reduce_kernel  the M-step.  One workgroup per (group, 64 classes): wave j adds the group's slabs j, j + 4, ... in slab
//                         order, the four partial sums are added in wave order, then the smoothing; writes pi and w = pi / train_prior.
// cover_adapt_topk_kernel one wave per point: the posterior under the final weights as fp32 scores, then the selection rounds of
//                         calibrate_topk_kernel on topk_key.  The row is not kept: the owner lane of a winner recomputes its own
//                         scores (same operands, same operations: same bits) when it looks for its next candidate.
// No float atomics anywhere: every fp64 sum has an order fixed by the offsets and K, so a repeated call returns the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "topk_key.h"

namespace {

constexpr int COVER_LDS_ENTRIES = 6144;   // 48 KB of 64-bit counters per workgroup
constexpr int COVER_REG_MAX_K = 512;      // classes per lane held in registers: 1, 2, 4 or 8


typedef unsigned long long u64;

// the group of `row`: the g with offsets[g] <= row < offsets[g + 1] (empty groups are stepped over); 0 <= row < offsets[n_groups]
__device__ __forceinline__ int64_t cover_group_of(const int64_t* __restrict__ offsets, int64_t n_groups, int64_t row)
{
    int64_t lo = 0, hi = n_groups;   // offsets[lo] <= row < offsets[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (offsets[mid] <= row) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ double wave_sum_d(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ bool z_ok(double z) { return z > 0.0 && z < INFINITY; }   // finite and positive (false for NaN)

__global__ __launch_bounds__(256) void cover_count_kernel(const float* __restrict__ P, int64_t n, int K, const int64_t* __restrict__ offsets,
                                                          int64_t n_groups, u64* __restrict__ count, u64* __restrict__ soft,
                                                          u64* __restrict__ unusable)
{
    __shared__ u64 tab[COVER_LDS_ENTRIES];   // per group of the workgroup's run: [K] counts, [K] soft sums, unusable
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * 256, r1 = r0 + 256 < n ? r0 + 256 : n;
    const int64_t g0 = cover_group_of(offsets, n_groups, r0), g1 = cover_group_of(offsets, n_groups, r1 - 1);
    const int64_t per = 2 * (int64_t)K + 1, span = g1 - g0 + 1;
    const bool in_lds = span * per <= COVER_LDS_ENTRIES;   // (the same in every thread)
    const int used = in_lds ? (int)(span * per) : 0;
    if (in_lds) {
        for (int i = tid; i < used; i += 256) tab[i] = 0;
        __syncthreads();
    }
    const int64_t row = r0 + tid;
    if (row < r1) {
        const int64_t g = cover_group_of(offsets, n_groups, row);
        const float* v = P + (size_t)row * K;
        bool ok = true;
        float best = -INFINITY;
        int besti = 0;
        for (int c = 0; c < K; ++c) {
            const float x = v[c];
            ok = ok && finite_f(x);
            if (x > best) { best = x; besti = c; }
        }
        u64* cnt = in_lds ? tab + (g - g0) * per : count + (size_t)g * K;
        u64* sft = in_lds ? tab + (g - g0) * per + K : soft + (size_t)g * K;
        u64* bad = in_lds ? tab + (g - g0) * per + 2 * K : unusable + g;
        if (!ok) {
            atomicAdd(bad, 1ull);
        } else {
            atomicAdd(cnt + besti, 1ull);
            int c = tid % K;   // neighbouring threads start at different classes: fewer equal-address atomics per instruction
            for (int j = 0; j < K; ++j) {
                atomicAdd(sft + c, (u64)llrint((double)v[c] * 4294967296.0));
                c = c + 1 == K ? 0 : c + 1;
            }
        }
    }
    if (in_lds) {
        __syncthreads();
        for (int i = tid; i < used; i += 256) {
            const u64 t = tab[i];
            if (!t) continue;
            const int64_t g = g0 + i / per;
            const int e = (int)(i % per);
            if (e < K) atomicAdd(count + (size_t)g * K + e, t);
            else if (e < 2 * K) atomicAdd(soft + (size_t)g * K + (e - K), t);
            else atomicAdd(unusable + g, t);
        }
    }
}

// pi_0 = train_prior and w_0 = pi_0 / train_prior for every group
__global__ __launch_bounds__(256) void cover_em_init_kernel(const double* __restrict__ train_prior, int64_t cells, int K, double* __restrict__ pi,
                                                            double* __restrict__ w)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cells) return;
    const double p = train_prior[i % K];
    pi[i] = p;
    w[i] = p / p;
}

template <int CPL>   // classes per lane: K <= 64 CPL
__global__ __launch_bounds__(256) void cover_em_pass_kernel(const float* __restrict__ P, int K, const int64_t* __restrict__ slab_row0,
                                                            const int32_t* __restrict__ slab_group, const int64_t* __restrict__ offsets,
                                                            int64_t n_slabs, const double* __restrict__ w, double* __restrict__ part)
{
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= n_slabs) return;
    const int64_t g = slab_group[s], r0 = slab_row0[s], end = offsets[g + 1];
    const int cnt = (int)(end - r0 < COVER_SLAB_POINTS ? end - r0 : COVER_SLAB_POINTS);
    double wr[CPL], acc[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int c = lane + 64 * j;
        wr[j] = c < K ? w[(size_t)g * K + c] : 0.0;
        acc[j] = 0.0;
    }
    for (int p = 0; p < cnt; ++p) {
        const float* v = P + (size_t)(r0 + p) * K;
        float x[CPL];
        double tq[CPL], z = 0.0;
        bool fin = true;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int c = lane + 64 * j;
            x[j] = c < K ? v[c] : 0.f;
            fin = fin && finite_f(x[j]);
            tq[j] = __dmul_rn((double)x[j], wr[j]);
            z += tq[j];
        }
        if (!__all(fin)) continue;   // an unusable point enters nothing (the same in every lane)
        z = wave_sum_d(z);
        const bool ok = z_ok(z);
#pragma unroll
        for (int j = 0; j < CPL; ++j) acc[j] += ok ? tq[j] / z : (double)x[j];
    }
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int c = lane + 64 * j;
        if (c < K) part[(size_t)s * K + c] = acc[j];
    }
}

// any K: the lane's accumulators live in the slab's output row (only their owner touches them)
__global__ __launch_bounds__(256) void cover_em_pass_wide_kernel(const float* __restrict__ P, int K, const int64_t* __restrict__ slab_row0,
                                                                 const int32_t* __restrict__ slab_group, const int64_t* __restrict__ offsets,
                                                                 int64_t n_slabs, const double* __restrict__ w, double* part)
{
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= n_slabs) return;
    const int64_t g = slab_group[s], r0 = slab_row0[s], end = offsets[g + 1];
    const int cnt = (int)(end - r0 < COVER_SLAB_POINTS ? end - r0 : COVER_SLAB_POINTS);
    const double* wg = w + (size_t)g * K;
    double* out = part + (size_t)s * K;
    for (int c = lane; c < K; c += 64) out[c] = 0.0;
    for (int p = 0; p < cnt; ++p) {
        const float* v = P + (size_t)(r0 + p) * K;
        double z = 0.0;
        bool fin = true;
        for (int c = lane; c < K; c += 64) {
            const float x = v[c];
            fin = fin && finite_f(x);
            z += __dmul_rn((double)x, wg[c]);
        }
        if (!__all(fin)) continue;
        z = wave_sum_d(z);
        const bool ok = z_ok(z);
        for (int c = lane; c < K; c += 64) {
            const float x = v[c];
            out[c] += ok ? __dmul_rn((double)x, wg[c]) / z : (double)x;
        }
    }
}

// grid (group, ceil(K / 64)); pi_t[c] = (sum of the group's slabs + strength train_prior[c]) / (n_g + strength), train_prior for n_g = 0
__global__ __launch_bounds__(256) void cover_em_reduce_kernel(const double* __restrict__ part, const int64_t* __restrict__ group_slab0,
                                                              const int64_t* __restrict__ offsets, const u64* __restrict__ unusable,
                                                              const double* __restrict__ train_prior, double strength, int K,
                                                              double* __restrict__ pi, double* __restrict__ w)
{
    __shared__ double sums[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t g = blockIdx.x;
    const int c = blockIdx.y * 64 + lane;
    const int64_t s0 = group_slab0[g], s1 = group_slab0[g + 1];
    double s = 0.0;
    if (c < K) {
#pragma unroll 4
        for (int64_t sl = s0 + wave; sl < s1; sl += 4) s += part[(size_t)sl * K + c];
    }
    sums[wave][lane] = s;
    __syncthreads();
    if (wave != 0 || c >= K) return;
    s = ((sums[0][lane] + sums[1][lane]) + sums[2][lane]) + sums[3][lane];
    const int64_t ng = offsets[g + 1] - offsets[g] - (int64_t)unusable[g];
    const double pr = train_prior[c];
    const double p = ng > 0 ? __dadd_rn(s, __dmul_rn(strength, pr)) / ((double)ng + strength) : pr;
    pi[(size_t)g * K + c] = p;
    w[(size_t)g * K + c] = p / pr;
}

// the fp32 score of one class under the group's weights: q = v w / Z when Z is finite and positive, else v
__device__ __forceinline__ float adapt_score(float x, double wc, double z, bool ok)
{
    return ok ? (float)(__dmul_rn((double)x, wc) / z) : x;
}

__global__ __launch_bounds__(256) void cover_adapt_topk_kernel(const float* __restrict__ P, int64_t n, int K, const int64_t* __restrict__ offsets,
                                                               int64_t n_groups, const double* __restrict__ w, int k,
                                                               int32_t* __restrict__ idx_out, float* __restrict__ score_out)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const int64_t g = cover_group_of(offsets, n_groups, row);
    const float* v = P + (size_t)row * K;
    const double* wg = w + (size_t)g * K;
    double z = 0.0;
    for (int c = lane; c < K; c += 64) z += __dmul_rn((double)v[c], wg[c]);
    z = wave_sum_d(z);
    const bool ok = z_ok(z);
    unsigned long long cur = 0;   // this lane's largest key not yet selected (calibrate_topk_kernel)
    for (int c = lane; c < K; c += 64) {
        const unsigned long long key = topk_key(adapt_score(v[c], wg[c], z, ok), c);
        cur = key > cur ? key : cur;
    }
    for (int j = 0; j < k; ++j) {   // k <= K (checked by the launcher): a real key is left in every round
        unsigned long long win = cur;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long t = __shfl_xor(win, o);
            win = t > win ? t : win;
        }
        if (lane == 0) {
            idx_out[(size_t)row * k + j] = (int32_t)(0xFFFFFFFFu - (unsigned)win);
            score_out[(size_t)row * k + j] = __uint_as_float((unsigned)(win >> 32));
        }
        if (cur == win) {   // the owner (keys are distinct): its next candidate is its largest key below the winner
            unsigned long long nb = 0;
            for (int c = lane; c < K; c += 64) {
                const unsigned long long key = topk_key(adapt_score(v[c], wg[c], z, ok), c);
                nb = (key < win && key > nb) ? key : nb;
            }
            cur = nb;
        }
    }
}

}   // namespace

int launch_cover_count(const float* P, int64_t n, int K, const int64_t* offsets, int64_t n_groups, unsigned long long* count,
                       unsigned long long* soft, unsigned long long* unusable, hipStream_t st)
{
    if (n < 1 || K < 1 || n_groups < 1 || (n + 255) / 256 > 0x7FFFFFFFLL) return -18;
    hipLaunchKernelGGL(cover_count_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, P, n, K, offsets, n_groups, count, soft,
                       unusable);
    LAUNCH_CHECK();
    return 0;
}

int launch_cover_em_init(const double* train_prior, int64_t n_groups, int K, double* pi, double* w, hipStream_t st)
{
    const int64_t cells = n_groups * K;
    if (n_groups < 1 || K < 1 || (cells + 255) / 256 > 0x7FFFFFFFLL) return -18;
    hipLaunchKernelGGL(cover_em_init_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, train_prior, cells, K, pi, w);
    LAUNCH_CHECK();
    return 0;
}

int launch_cover_em_pass(const float* P, int K, const int64_t* slab_row0, const int32_t* slab_group, const int64_t* offsets, int64_t n_slabs,
                         const double* w, double* part, hipStream_t st)
{
    if (K < 1 || n_slabs < 1 || (n_slabs + 3) / 4 > 0x7FFFFFFFLL) return -18;
    const dim3 grid((unsigned)((n_slabs + 3) / 4)), block(256);
#define COVER_PASS(CPL) \
    hipLaunchKernelGGL((cover_em_pass_kernel<CPL>), grid, block, 0, st, P, K, slab_row0, slab_group, offsets, n_slabs, w, part)
    if (K <= 64) COVER_PASS(1);
    else if (K <= 128) COVER_PASS(2);
    else if (K <= 256) COVER_PASS(4);
    else if (K <= COVER_REG_MAX_K) COVER_PASS(8);
    else hipLaunchKernelGGL(cover_em_pass_wide_kernel, grid, block, 0, st, P, K, slab_row0, slab_group, offsets, n_slabs, w, part);
#undef COVER_PASS
    LAUNCH_CHECK();
    return 0;
}

int launch_cover_em_reduce(const double* part, const int64_t* group_slab0, const int64_t* offsets, const unsigned long long* unusable,
                           const double* train_prior, double strength, int64_t n_groups, int K, double* pi, double* w, hipStream_t st)
{
    if (n_groups < 1 || n_groups > 0x7FFFFFFFLL || K < 1 || (K + 63) / 64 > 65535) return -18;
    hipLaunchKernelGGL(cover_em_reduce_kernel, dim3((unsigned)n_groups, (unsigned)((K + 63) / 64)), dim3(256), 0, st, part, group_slab0, offsets,
                       unusable, train_prior, strength, K, pi, w);
    LAUNCH_CHECK();
    return 0;
}

int launch_cover_adapt_topk(const float* P, int64_t n, int K, const int64_t* offsets, int64_t n_groups, const double* w, int k, int32_t* idx,
                            float* scores, hipStream_t st)
{
    if (n < 1 || K < 1 || n_groups < 1 || k < 1 || k > K || !idx || !scores || (n + 3) / 4 > 0x7FFFFFFFLL) return -18;
    hipLaunchKernelGGL(cover_adapt_topk_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, P, n, K, offsets, n_groups, w, k, idx, scores);
    LAUNCH_CHECK();
    return 0;
}
