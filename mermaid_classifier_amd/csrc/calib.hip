// calib.hip -- evaluation and Platt calibration of the trained MLP classifier on the device (gfx950).
//
// Replaces the host steps the reference's MermaidTrainer takes after partial_fit, each fed there by predict_proba on the host:
//   mmc_trainer_evaluate       _calc_acc_batched / _calc_acc_and_log_loss_batched (reference trainer.py:295-342):
//                              argmax == y count and sum of sklearn.metrics.log_loss's per-row term
//   mmc_calibrator_*           _calibrate_in_batches (trainer.py:344-396) -> sklearn.calibration._fit_calibrator(.., "sigmoid"):
//                              one Platt sigmoid per class, all classes fitted at once
//   mmc_trainer_evaluate_classes(_set)   the same evaluation that also keeps the K x K table of (true class, argmax) counts: what
//                              compute_precision_recall_f1 / compute_balanced_accuracy_mcc (metrics/classification.py:171-302) are
//                              functions of, per epoch
//
// Probability store.  add_features runs the trainer's own forward (trainer_forward: the tgemm kernels of a training step) and
// softmax_store_kernel writes the probabilities of _forward_probs (torch_classifier.py here: fp32 max-subtract, exp, sum, divide,
// then float64 renormalisation, stored as fp32) CLASS-MAJOR: P[k][cap], row i of class k at P[k * cap + i], so each class's
// column is contiguous for the fit.  add_scores stores caller scores the same way (fp32).  Growth: when a call would pass `cap`,
// cap becomes max(2 cap, rows needed) rounded up to 1024 and the K columns move with one 2-D copy (pitch cap -> new cap).
//
// Platt fit (the Lin-Lin-Weng form of Platt's method; objective and start point exactly those of sklearn's
// _sigmoid_calibration, only the optimiser differs).  Class k: F = column k, n1 = #(y == k), n0 = N - n1, targets T1 =
// (n1+1)/(n1+2) on positives, T0 = 1/(n0+2) on negatives, start A = 0, B = log((n0+1)/(n1+1)); when max|F| >= 30, F is divided
// by max|F| and A is un-scaled at the end.  Damped Newton in fp64:
//   platt_pass_kernel    grid (active class, row chunk): at the class's trial point, r = -(A F + B), s = sigma(r):
//                        loss sum log1p(e^r) - T r, gradient (-sum (s-T) F, -sum (s-T)), Hessian sum s(1-s) [F^2, F; F, 1]
//                        -> one slab entry of 6 doubles per (class, chunk)
//   platt_step_kernel    one workgroup: per active class, reduce its chunks in order; accept the trial point (Armijo) or halve
//                        the step; on acceptance stop on |gradient| <= 1e-12 N or a negligible Newton step, else solve the 2x2
//                        system (1e-12 ridge on the diagonal) for the next trial point; then compact the active list.
// The host reads one pinned "classes still active" counter per iteration.  At most 100 trial evaluations per class.
//
// Every floating-point reduction runs in a fixed order (the only atomics are the integer adds of the class-wise table, which are
// exact in any order), so a run is bit-reproducible; the fit's row chunks depend only on N, so
// the same rows added in any number of calls give the same a / b bits.  mmc_trainer_evaluate sums the per-row log-loss as
// 2^-32 fixed point in int64 (exact and order-free); mmc_trainer_evaluate_q32 returns that integer, so sums over any split of
// the rows into calls are the same integer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cfloat>
#include <cmath>
#include <utility>
#include <vector>

#include "../../include/mmc.h"
#include "trainer_internal.h"

namespace {

constexpr double kLossFix = 4294967296.0;   // 2^32: fixed-point scale of mmc_trainer_evaluate's per-row log-loss
constexpr int kPlattChunkRows = 16384;      // rows per fit chunk before the chunk count is capped
constexpr int kPlattMaxChunks = 64;
constexpr int kPlattMaxIter = 100;
enum { ST_START = 0, ST_TRIAL = 1, ST_DONE = 2, ST_CAPPED = 3 };

struct PlattState {
    double A, B;       // accepted point (A on the scaled F)
    double At, Bt;     // point the next pass evaluates
    double dA, dB, t;  // Newton direction and step length
    double f, gA, gB;  // objective and gradient at (A, B)
    double inv_scale, max_f;   // 1 / scale and max|F| / scale
    double T1, T0;
    int iters, status;
};

__device__ inline float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
template <typename T>
__device__ inline T wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

struct RowSoftmax {
    float mx, s;
    double s64;
};

// _forward_probs of one row z[K] by one wave: fp32 max-subtract, exp, sum and divide; float64 sum of the fp32 quotients
__device__ inline RowSoftmax row_softmax(const float* z, int K, int lane)
{
    float mx = -INFINITY;
    for (int c = lane; c < K; c += 64) mx = fmaxf(mx, z[c]);
    mx = wave_max(mx);
    float s = 0.f;
    for (int c = lane; c < K; c += 64) s += expf(z[c] - mx);
    s = wave_sum(s);
    double s64 = 0.0;
    for (int c = lane; c < K; c += 64) s64 += (double)(expf(z[c] - mx) / s);
    s64 = wave_sum(s64);
    return {mx, s, s64};
}
__device__ inline double row_prob(const float* z, int c, const RowSoftmax& r) { return (double)(expf(z[c] - r.mx) / r.s) / r.s64; }

// logits [M][K] -> P[c * cap + off + row] (fp32 of the renormalised float64 probability).  64 rows per workgroup, 16 per wave;
// classes in slices of 64 staged through LDS so that every class's 64 rows leave as one contiguous store.
__global__ __launch_bounds__(256) void softmax_store_kernel(const float* __restrict__ logits, int M, int K, float* __restrict__ P,
                                                            int64_t cap, int64_t off)
{
    __shared__ float tile[64][65];
    __shared__ RowSoftmax rs[64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * 64;
    for (int j = 0; j < 16; ++j) {
        const int r = wave * 16 + j;
        if (r0 + r < M) {
            const RowSoftmax v = row_softmax(logits + (size_t)(r0 + r) * K, K, lane);
            if (lane == 0) rs[r] = v;
        }
    }
    __syncthreads();
    for (int c0 = 0; c0 < K; c0 += 64) {
        for (int j = 0; j < 16; ++j) {
            const int r = wave * 16 + j, c = c0 + lane;
            if (r0 + r < M && c < K) tile[lane][r] = (float)row_prob(logits + (size_t)(r0 + r) * K, c, rs[r]);
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < 64 * 64; idx += 256) {
            const int cl = idx >> 6, r = idx & 63;
            if (c0 + cl < K && r0 + r < M) P[(size_t)(c0 + cl) * cap + off + r0 + r] = tile[cl][r];
        }
        __syncthreads();
    }
}

// scores [M][K] float64 row-major -> P[c * cap + off + row] fp32 (64 x 64 tiles transposed through LDS)
__global__ __launch_bounds__(256) void scores_store_kernel(const double* __restrict__ S, int M, int K, float* __restrict__ P, int64_t cap,
                                                           int64_t off)
{
    __shared__ float tile[64][65];
    const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    for (int idx = threadIdx.x; idx < 64 * 64; idx += 256) {
        const int r = idx >> 6, c = idx & 63;
        if (r0 + r < M && c0 + c < K) tile[c][r] = (float)S[(size_t)(r0 + r) * K + c0 + c];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 64 * 64; idx += 256) {
        const int c = idx >> 6, r = idx & 63;
        if (r0 + r < M && c0 + c < K) P[(size_t)(c0 + c) * cap + off + r0 + r] = tile[c][r];
    }
}

// One wave per row: argmax of the renormalised probabilities (first index on ties, as np.argmax) == y, and
// -log(clip(p_y, DBL_EPSILON, 1 - DBL_EPSILON)) as 2^-32 fixed point.  slab[2 b] = correct rows, slab[2 b + 1] = loss of workgroup b.
// CONF (mmc_trainer_evaluate_classes*): the row's (true class, argmax) pair is kept as well -- lane 0 adds 1 to
// confusion[y * K + argmax], a 64-bit integer atomic on device memory, so the table is exact and order-free.  One atomic per row
// next to a forward of dims[0] x hidden MACs per row; no per-workgroup pre-aggregation (profiles/class_eval.txt).  A row whose
// probabilities are all NaN has no argmax (arg stays K) and enters no cell.
template <bool CONF>
__global__ __launch_bounds__(256) void eval_rows_kernel(const float* __restrict__ logits, const int32_t* __restrict__ y, int M, int K,
                                                        long long* __restrict__ slab, unsigned long long* __restrict__ confusion)
{
    __shared__ long long red[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave;
    long long correct = 0, q = 0;
    if (row < M) {
        const float* z = logits + (size_t)row * K;
        const RowSoftmax r = row_softmax(z, K, lane);
        double best = -1.0;
        int arg = K;
        for (int c = lane; c < K; c += 64) {
            const double p = row_prob(z, c, r);
            if (p > best) { best = p; arg = c; }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const double ob = __shfl_xor(best, o);
            const int oa = __shfl_xor(arg, o);
            if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
        }
        const int yi = y[row];
        const double py = fmin(fmax(row_prob(z, yi, r), DBL_EPSILON), 1.0 - DBL_EPSILON);
        correct = arg == yi;
        q = llrint(-log(py) * kLossFix);
        if (CONF && lane == 0 && arg < K) atomicAdd(&confusion[(size_t)yi * K + arg], 1ull);
    }
    if (lane == 0) { red[wave][0] = correct; red[wave][1] = q; }
    __syncthreads();
    if (threadIdx.x == 0) {
        slab[2 * blockIdx.x] = red[0][0] + red[1][0] + red[2][0] + red[3][0];
        slab[2 * blockIdx.x + 1] = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    }
}

// out[0..2) = column sums of slab[nb][2] (one workgroup).  ACC: out += instead -- the chunks of one call over a resident feature set
// add up on the device, in stream order, and the host reads the two totals once.
template <bool ACC>
__global__ __launch_bounds__(256) void eval_finalize_kernel(const long long* __restrict__ slab, int nb, long long* __restrict__ out)
{
    __shared__ long long red[256][2];
    long long a = 0, b = 0;
    for (int i = threadIdx.x; i < nb; i += 256) { a += slab[2 * i]; b += slab[2 * i + 1]; }
    red[threadIdx.x][0] = a;
    red[threadIdx.x][1] = b;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (threadIdx.x < o) { red[threadIdx.x][0] += red[threadIdx.x + o][0]; red[threadIdx.x][1] += red[threadIdx.x + o][1]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = (ACC ? out[0] : 0) + red[0][0];
        out[1] = (ACC ? out[1] : 0) + red[0][1];
    }
}

// grid (K, G): stats[(k G + g) * 2] = { #(y == k), max|F| } over chunk g of class k
__global__ __launch_bounds__(256) void platt_stats_kernel(const float* __restrict__ P, int64_t cap, const int32_t* __restrict__ y, int64_t N,
                                                          int64_t chunk, double* __restrict__ stats)
{
    __shared__ double red[2][4];
    const int k = blockIdx.x, g = blockIdx.y, G = gridDim.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t lo = (int64_t)g * chunk, hi = lo + chunk < N ? lo + chunk : N;
    const float* F = P + (size_t)k * cap;
    double cnt = 0.0;
    float mx = 0.f;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        cnt += y[i] == k ? 1.0 : 0.0;
        mx = fmaxf(mx, fabsf(F[i]));
    }
    cnt = wave_sum(cnt);
    mx = wave_max(mx);
    if (lane == 0) { red[0][wave] = cnt; red[1][wave] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        stats[((size_t)k * G + g) * 2] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        stats[((size_t)k * G + g) * 2 + 1] = fmax(fmax(red[1][0], red[1][1]), fmax(red[1][2], red[1][3]));
    }
}

// one workgroup: per class, n1 / max|F| from the chunks in order -> targets, scale, start point; every class active
__global__ __launch_bounds__(256) void platt_init_kernel(const double* __restrict__ stats, int K, int G, int64_t N, PlattState* __restrict__ st,
                                                         int* __restrict__ active, int* __restrict__ n_active)
{
    for (int k = threadIdx.x; k < K; k += 256) {
        double n1 = 0.0, mx = 0.0;
        for (int g = 0; g < G; ++g) {
            n1 += stats[((size_t)k * G + g) * 2];
            mx = fmax(mx, stats[((size_t)k * G + g) * 2 + 1]);
        }
        const double n0 = (double)N - n1;
        const double scale = mx >= 30.0 ? mx : 1.0;   // _sigmoid_calibration: max_abs_prediction_threshold = 30
        PlattState s;
        s.inv_scale = 1.0 / scale;
        s.max_f = mx / scale;
        s.T1 = (n1 + 1.0) / (n1 + 2.0);
        s.T0 = 1.0 / (n0 + 2.0);
        s.A = s.At = 0.0;
        s.B = s.Bt = log((n0 + 1.0) / (n1 + 1.0));
        s.dA = s.dB = 0.0;
        s.t = 1.0;
        s.f = s.gA = s.gB = 0.0;
        s.iters = 0;
        s.status = ST_START;
        st[k] = s;
        active[k] = k;
    }
    if (threadIdx.x == 0) *n_active = K;
}

// grid (n_active, G): objective / gradient / Hessian partials of class active[x] over row chunk y at its trial point.
// Each thread takes 4 consecutive rows per step (one float4 of F, one int4 of y: cap is a multiple of 1024 and chunk starts are
// multiples of 4, so a float4 that starts below N lies inside the allocation; lanes past N are masked).
__global__ __launch_bounds__(256) void platt_pass_kernel(const float* __restrict__ P, int64_t cap, const int32_t* __restrict__ y, int64_t N,
                                                         int64_t chunk, const int* __restrict__ active, const PlattState* __restrict__ st,
                                                         double* __restrict__ part)
{
    __shared__ double red[4][6];
    const int k = active[blockIdx.x], g = blockIdx.y, G = gridDim.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double A = st[k].At, B = st[k].Bt, inv_scale = st[k].inv_scale, T1 = st[k].T1, T0 = st[k].T0;
    const int64_t lo = (int64_t)g * chunk, hi = lo + chunk < N ? lo + chunk : N;
    const float* F = P + (size_t)k * cap;
    double L = 0.0, gA = 0.0, gB = 0.0, hAA = 0.0, hAB = 0.0, hBB = 0.0;
    for (int64_t i0 = lo + 4 * threadIdx.x; i0 < hi; i0 += 1024) {
        const float4 f4 = *reinterpret_cast<const float4*>(F + i0);
        const int4 y4 = *reinterpret_cast<const int4*>(y + i0);
        const float fv[4] = {f4.x, f4.y, f4.z, f4.w};
        const int yv[4] = {y4.x, y4.y, y4.z, y4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i0 + j >= hi) break;
            const double Fs = (double)fv[j] * inv_scale;
            const double T = yv[j] == k ? T1 : T0;
            const double r = -(A * Fs + B);
            const double e = exp(-fabs(r));                        // sigma and log1p(e^r) from one exp
            const double inv1pe = 1.0 / (1.0 + e);
            L += (r > 0.0 ? r : 0.0) + log1p(e) - T * r;
            const double s = r >= 0.0 ? inv1pe : e * inv1pe;
            const double w = e * inv1pe * inv1pe;                  // s (1 - s)
            const double d = s - T;
            gA -= d * Fs;
            gB -= d;
            hAA += w * Fs * Fs;
            hAB += w * Fs;
            hBB += w;
        }
    }
    double v[6] = {L, gA, gB, hAA, hAB, hBB};
#pragma unroll
    for (int j = 0; j < 6; ++j) v[j] = wave_sum(v[j]);
    if (lane == 0)
#pragma unroll
        for (int j = 0; j < 6; ++j) red[wave][j] = v[j];
    __syncthreads();
    if (threadIdx.x < 6) {
        const int j = threadIdx.x;
        part[((size_t)k * G + g) * 6 + j] = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
    }
}

// one workgroup: the Newton / backtracking update of every active class, then compaction of the active list
__global__ __launch_bounds__(256) void platt_step_kernel(const double* __restrict__ part, int K, int G, int64_t N, PlattState* __restrict__ st,
                                                         int* __restrict__ active, int* __restrict__ n_active)
{
    __shared__ int scan[256];
    __shared__ int base;
    const double ridge = 1e-12, gtol = 1e-12 * (double)N;
    for (int k = threadIdx.x; k < K; k += 256) {
        PlattState s = st[k];
        if (s.status != ST_START && s.status != ST_TRIAL) continue;
        double v[6] = {0, 0, 0, 0, 0, 0};
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int j = 0; j < 6; ++j) v[j] += part[((size_t)k * G + g) * 6 + j];
        const double L = v[0], gA = v[1], gB = v[2], hAA = v[3], hAB = v[4], hBB = v[5];
        bool accept = s.status == ST_START;
        if (s.status == ST_TRIAL) {
            ++s.iters;
            // Armijo with a slack of a few ulps of the objective: at the optimum the objective only moves by rounding
            accept = L <= s.f + 1e-4 * s.t * (s.gA * s.dA + s.gB * s.dB) + 64.0 * DBL_EPSILON * fabs(s.f);
            if (!accept) {
                s.t *= 0.5;
                if (s.t < 1e-6) s.status = ST_DONE;   // no decrease along a descent direction: the point is as good as rounding allows
                else if (s.iters >= kPlattMaxIter) s.status = ST_CAPPED;
                else { s.At = s.A + s.t * s.dA; s.Bt = s.B + s.t * s.dB; }
            }
        }
        if (accept) {
            s.A = s.At; s.B = s.Bt; s.f = L; s.gA = gA; s.gB = gB;
            const double a11 = hAA + ridge, a22 = hBB + ridge, det = a11 * a22 - hAB * hAB;
            double dA, dB;
            if (det > 0.0) { dA = -(a22 * gA - hAB * gB) / det; dB = -(a11 * gB - hAB * gA) / det; }
            else { dA = 0.0; dB = -gB / a22; }   // rounding made the (PSD) system look singular: a step in B alone
            if (fmax(fabs(gA), fabs(gB)) <= gtol || fabs(dA) * s.max_f + fabs(dB) <= 1e-13 * (1.0 + fabs(s.B))) s.status = ST_DONE;
            else if (s.iters >= kPlattMaxIter) s.status = ST_CAPPED;
            else {
                s.status = ST_TRIAL;
                s.dA = dA; s.dB = dB; s.t = 1.0;
                s.At = s.A + dA; s.Bt = s.B + dB;
            }
        }
        st[k] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int k0 = 0; k0 < K; k0 += 256) {
        const int k = k0 + threadIdx.x;
        const int flag = k < K && (st[k].status == ST_START || st[k].status == ST_TRIAL);
        scan[threadIdx.x] = flag;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {   // inclusive Hillis-Steele scan
            const int add = threadIdx.x >= o ? scan[threadIdx.x - o] : 0;
            __syncthreads();
            scan[threadIdx.x] += add;
            __syncthreads();
        }
        if (flag) active[base + scan[threadIdx.x] - 1] = k;
        __syncthreads();
        if (threadIdx.x == 0) base += scan[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) *n_active = base;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
struct mmc_calibrator {
    int K = 0, device = 0;
    int64_t n = 0, cap = 0;          // rows stored / rows allocated per class
    DevBuf<float> P;                 // [K][cap] class-major probabilities / scores
    DevBuf<int32_t> y;               // [cap]
    DevBuf<double> S;                // add_scores staging [kTrainerForwardRows][K]
    DevBuf<double> stats, part;
    DevBuf<PlattState> st;
    DevBuf<int> active, n_active;
    int* n_active_host = nullptr;    // pinned
};

int check_labels(const int32_t* y, int64_t n, int K)
{
    for (int64_t i = 0; i < n; ++i)
        if (y[i] < 0 || y[i] >= K) return mmc_fail(MMC_ERR_ARG, "label index y[%lld] = %d outside [0, %d)", (long long)i, y[i], K);
    return MMC_OK;
}

// room for `need` rows per class; growth doubles and moves the K columns with one 2-D copy
static int calib_reserve(mmc_calibrator* c, int64_t need, hipStream_t st)
{
    if (need <= c->cap) return MMC_OK;
    int64_t cap = c->cap * 2 > need ? c->cap * 2 : need;
    cap = (cap + 1023) / 1024 * 1024;
    DevBuf<float> P;
    DevBuf<int32_t> y;
    if (int r = P.reserve((int64_t)c->K * cap)) return r;
    if (!y.alloc(cap)) return mmc_fail(MMC_ERR_NOMEM, "hipMalloc of %lld labels failed", (long long)cap);
    if (c->n) {
        HIP_TRY(hipMemcpy2DAsync(P, (size_t)cap * 4, c->P, (size_t)c->cap * 4, (size_t)c->n * 4, (size_t)c->K, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(y, c->y, (size_t)c->n * 4, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    c->P = std::move(P);
    c->y = std::move(y);
    c->cap = cap;
    return MMC_OK;
}

extern "C" void mmc_calibrator_destroy(mmc_calibrator* c)
{
    if (!c) return;
    hipSetDevice(c->device);
    hipHostFree(c->n_active_host);
    delete c;
}

extern "C" int mmc_calibrator_create(int K, int device, mmc_calibrator** out)
{
    if (!out) return mmc_fail(MMC_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (K < 3) return mmc_fail(MMC_ERR_ARG, "K = %d: the calibrated head is multiclass only (K >= 3)", K);
    if (int r = check_device(device)) return r;
    HIP_TRY(hipSetDevice(device));
    mmc_calibrator* c = new mmc_calibrator();
    c->K = K;
    c->device = device;
    const size_t slots = (size_t)K * kPlattMaxChunks;
    bool ok = c->stats.alloc(slots * 2) && c->part.alloc(slots * 6) && c->st.alloc(K) && c->active.alloc(K) && c->n_active.alloc(1) &&
              hipHostMalloc((void**)&c->n_active_host, 4, hipHostMallocDefault) == hipSuccess;
    if (!ok) {
        mmc_calibrator_destroy(c);
        return mmc_fail(MMC_ERR_NOMEM, "hipMalloc failed while creating the calibrator");
    }
    *out = c;
    return MMC_OK;
}

extern "C" int mmc_calibrator_add_features(mmc_calibrator* c, mmc_trainer* t, const float* X, const int32_t* y, int64_t n, void* hip_stream)
{
    if (!c || !t) return mmc_fail(MMC_ERR_ARG, "calibrator/trainer handle is NULL");
    if (n < 0) return mmc_fail(MMC_ERR_ARG, "n = %lld is negative", (long long)n);
    if (trainer_classes(t) != c->K) return mmc_fail(MMC_ERR_ARG, "trainer has K = %d classes, calibrator K = %d", trainer_classes(t), c->K);
    if (trainer_device(t) != c->device) return mmc_fail(MMC_ERR_ARG, "trainer is on device %d, calibrator on device %d", trainer_device(t), c->device);
    if (n == 0) return MMC_OK;
    if (!X || !y) return mmc_fail(MMC_ERR_ARG, "X/y is NULL");
    int r = check_labels(y, n, c->K);
    if (r) return r;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(c->device));
    r = calib_reserve(c, c->n + n, st);
    if (r) return r;
    const int d0 = trainer_input_dim(t);
    for (int64_t off = 0; off < n; off += kTrainerForwardRows) {
        const int cur = (int)((n - off) < kTrainerForwardRows ? (n - off) : kTrainerForwardRows);
        const float* z = nullptr;
        r = trainer_forward(t, X + (size_t)off * d0, cur, st, &z);
        if (r) return r;
        hipLaunchKernelGGL(softmax_store_kernel, dim3((cur + 63) / 64), dim3(256), 0, st, z, cur, c->K, c->P, c->cap, c->n + off);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(c->y + c->n, y, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->n += n;
    return MMC_OK;
}

int check_set_range(const mmc_featureset* fs, int64_t first, int64_t n)
{
    if (first < 0 || n < 0 || first > fs->n || n > fs->n - first)
        return mmc_fail(MMC_ERR_ARG, "rows [%lld, %lld + %lld) outside the set's %lld rows", (long long)first, (long long)first, (long long)n,
                        (long long)fs->n);
    return MMC_OK;
}

int check_set_matches(const mmc_featureset* fs, mmc_trainer* t)
{
    if (fs->dim != trainer_input_dim(t)) return mmc_fail(MMC_ERR_ARG, "feature set has %d columns, trainer expects %d", fs->dim, trainer_input_dim(t));
    if (fs->K != trainer_classes(t)) return mmc_fail(MMC_ERR_ARG, "feature set has %d classes, trainer %d", fs->K, trainer_classes(t));
    if (fs->device != trainer_device(t)) return mmc_fail(MMC_ERR_ARG, "feature set is on device %d, trainer on device %d", fs->device, trainer_device(t));
    return MMC_OK;
}

// mmc_calibrator_add_features on rows [first, first + n) of a resident feature set: the forward reads the set, the labels move device to
// device, and the stream is synchronised once
extern "C" int mmc_calibrator_add_set(mmc_calibrator* c, mmc_trainer* t, mmc_featureset* fs, int64_t first, int64_t n, void* hip_stream)
{
    if (!c || !t) return mmc_fail(MMC_ERR_ARG, "calibrator/trainer handle is NULL");
    if (!fs) return mmc_fail(MMC_ERR_ARG, "feature set handle is NULL");
    if (trainer_classes(t) != c->K) return mmc_fail(MMC_ERR_ARG, "trainer has K = %d classes, calibrator K = %d", trainer_classes(t), c->K);
    if (trainer_device(t) != c->device) return mmc_fail(MMC_ERR_ARG, "trainer is on device %d, calibrator on device %d", trainer_device(t), c->device);
    int r = check_set_matches(fs, t);
    if (r) return r;
    r = check_set_range(fs, first, n);
    if (r) return r;
    if (n == 0) return MMC_OK;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(c->device));
    r = calib_reserve(c, c->n + n, st);
    if (r) return r;
    for (int64_t off = 0; off < n; off += kTrainerForwardRows) {
        const int cur = (int)((n - off) < kTrainerForwardRows ? (n - off) : kTrainerForwardRows);
        const float* z = nullptr;
        r = trainer_forward_device(t, fs->X + (size_t)(first + off) * fs->dim, cur, st, &z);
        if (r) return r;
        hipLaunchKernelGGL(softmax_store_kernel, dim3((cur + 63) / 64), dim3(256), 0, st, z, cur, c->K, c->P, c->cap, c->n + off);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(c->y + c->n, fs->y + first, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->n += n;
    return MMC_OK;
}

extern "C" int mmc_calibrator_add_scores(mmc_calibrator* c, const double* scores, const int32_t* y, int64_t n, void* hip_stream)
{
    if (!c) return mmc_fail(MMC_ERR_ARG, "calibrator handle is NULL");
    if (n < 0) return mmc_fail(MMC_ERR_ARG, "n = %lld is negative", (long long)n);
    if (n == 0) return MMC_OK;
    if (!scores || !y) return mmc_fail(MMC_ERR_ARG, "scores/y is NULL");
    int r = check_labels(y, n, c->K);
    if (r) return r;
    for (int64_t i = 0; i < n * c->K; ++i) {
        if (!std::isfinite(scores[i]))
            return mmc_fail(MMC_ERR_ARG, "scores[%lld][%d] = %g is not finite", (long long)(i / c->K), (int)(i % c->K), scores[i]);
        if (std::fabs(scores[i]) > (double)FLT_MAX)   // stored as fp32: it would become inf
            return mmc_fail(MMC_ERR_ARG, "scores[%lld][%d] = %g is outside the fp32 range", (long long)(i / c->K), (int)(i % c->K), scores[i]);
    }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(c->device));
    r = calib_reserve(c, c->n + n, st);
    if (r) return r;
    if ((r = c->S.reserve((int64_t)kTrainerForwardRows * c->K))) return r;
    for (int64_t off = 0; off < n; off += kTrainerForwardRows) {
        const int cur = (int)((n - off) < kTrainerForwardRows ? (n - off) : kTrainerForwardRows);
        HIP_TRY(hipMemcpyAsync(c->S, scores + (size_t)off * c->K, (size_t)cur * c->K * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(scores_store_kernel, dim3((cur + 63) / 64, (c->K + 63) / 64), dim3(256), 0, st, c->S, cur, c->K, c->P, c->cap,
                           c->n + off);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));   // the staging buffer is reused by the next chunk
    }
    HIP_TRY(hipMemcpyAsync(c->y + c->n, y, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->n += n;
    return MMC_OK;
}

extern "C" int mmc_calibrator_fit(mmc_calibrator* c, double* a, double* b, int32_t* iterations, void* hip_stream)
{
    if (!c) return mmc_fail(MMC_ERR_ARG, "calibrator handle is NULL");
    if (!a || !b) return mmc_fail(MMC_ERR_ARG, "a/b is NULL");
    if (c->n < 1) return mmc_fail(MMC_ERR_ARG, "fit with no rows: add features or scores first");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(c->device));
    const int64_t N = c->n;
    int G = (int)((N + kPlattChunkRows - 1) / kPlattChunkRows);
    G = G < kPlattMaxChunks ? G : kPlattMaxChunks;
    int64_t chunk = (N + G - 1) / G;
    chunk = (chunk + 1023) / 1024 * 1024;
    G = (int)((N + chunk - 1) / chunk);
    const int K = c->K;
    hipLaunchKernelGGL(platt_stats_kernel, dim3(K, G), dim3(256), 0, st, c->P, c->cap, c->y, N, chunk, c->stats);
    hipLaunchKernelGGL(platt_init_kernel, dim3(1), dim3(256), 0, st, c->stats, K, G, N, c->st, c->active, c->n_active);
    HIP_TRY(hipGetLastError());
    int n_active = K;
    for (int pass = 0; n_active > 0; ++pass) {
        if (pass > kPlattMaxIter + 1) return mmc_fail(MMC_ERR_HIP, "Platt fit did not stop after %d passes", pass);
        hipLaunchKernelGGL(platt_pass_kernel, dim3(n_active, G), dim3(256), 0, st, c->P, c->cap, c->y, N, chunk, c->active, c->st, c->part);
        hipLaunchKernelGGL(platt_step_kernel, dim3(1), dim3(256), 0, st, c->part, K, G, N, c->st, c->active, c->n_active);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c->n_active_host, c->n_active, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        n_active = *c->n_active_host;
    }
    std::vector<PlattState> h(K);
    HIP_TRY(hipMemcpyAsync(h.data(), c->st, (size_t)K * sizeof(PlattState), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < K; ++k) {
        a[k] = h[k].A * h[k].inv_scale;   // the slope back on the caller's scale of F
        b[k] = h[k].B;
        if (iterations) iterations[k] = h[k].iters;
    }
    return MMC_OK;
}

// rows [0, n) of X / y through t's current parameters: *n_correct and the 2^-32 fixed-point sum of the per-row log-loss
static int trainer_evaluate(mmc_trainer* t, const float* X, const int32_t* y, int64_t n, int64_t* n_correct, int64_t* sum_q32,
                            void* hip_stream)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!n_correct || !sum_q32) return mmc_fail(MMC_ERR_ARG, "n_correct/sum_log_loss is NULL");
    if (n < 0) return mmc_fail(MMC_ERR_ARG, "n = %lld is negative", (long long)n);
    // the int64 fixed-point sum holds 2^63 / (36.05 * 2^32) > 5.9e7 rows of the largest per-row loss
    if (n > ((int64_t)1 << 25)) return mmc_fail(MMC_ERR_ARG, "n = %lld rows in one call: split it (at most 2^25)", (long long)n);
    *n_correct = 0;
    *sum_q32 = 0;
    if (n == 0) return MMC_OK;
    if (!X || !y) return mmc_fail(MMC_ERR_ARG, "X/y is NULL");
    const int K = trainer_classes(t);
    int r = check_labels(y, n, K);
    if (r) return r;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(trainer_device(t)));
    // scratch: slab [max_nb][2] int64, the two totals, then the chunk's labels
    const int max_nb = (kTrainerForwardRows + 3) / 4;
    void* scratch = nullptr;
    r = trainer_scratch(t, ((size_t)max_nb * 2 + 2) * 8 + (size_t)kTrainerForwardRows * 4, &scratch);
    if (r) return r;
    long long* slab = static_cast<long long*>(scratch);
    long long* totals = slab + 2 * max_nb;
    int32_t* dy = reinterpret_cast<int32_t*>(totals + 2);
    const int d0 = trainer_input_dim(t);
    long long tot[2] = {0, 0};
    for (int64_t off = 0; off < n; off += kTrainerForwardRows) {
        const int cur = (int)((n - off) < kTrainerForwardRows ? (n - off) : kTrainerForwardRows);
        const int nb = (cur + 3) / 4;
        const float* z = nullptr;
        long long h[2];
        r = trainer_forward(t, X + (size_t)off * d0, cur, st, &z);
        if (r) return r;
        HIP_TRY(hipMemcpyAsync(dy, y + off, (size_t)cur * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(eval_rows_kernel<false>, dim3(nb), dim3(256), 0, st, z, dy, cur, K, slab, (unsigned long long*)nullptr);
        hipLaunchKernelGGL(eval_finalize_kernel<false>, dim3(1), dim3(256), 0, st, slab, nb, totals);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h, totals, 16, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));   // before the next chunk reuses the labels / slab
        tot[0] += h[0];
        tot[1] += h[1];
    }
    *n_correct = tot[0];
    *sum_q32 = tot[1];
    return MMC_OK;
}

extern "C" int mmc_trainer_evaluate(mmc_trainer* t, const float* X, const int32_t* y, int64_t n, int64_t* n_correct, double* sum_log_loss,
                                    void* hip_stream)
{
    if (!sum_log_loss) return mmc_fail(MMC_ERR_ARG, "n_correct/sum_log_loss is NULL");
    int64_t q = 0;
    const int r = trainer_evaluate(t, X, y, n, n_correct, &q, hip_stream);
    *sum_log_loss = r ? 0.0 : (double)q / kLossFix;
    return r;
}

extern "C" int mmc_trainer_evaluate_q32(mmc_trainer* t, const float* X, const int32_t* y, int64_t n, int64_t* n_correct,
                                        int64_t* sum_log_loss_q32, void* hip_stream)
{
    return trainer_evaluate(t, X, y, n, n_correct, sum_log_loss_q32, hip_stream);
}

// mmc_trainer_evaluate_q32 on rows [first, first + n) of a resident feature set.  The forward and the labels read the set; every
// chunk's totals are added on the device; one 16-byte copy and one synchronisation per call.
extern "C" int mmc_trainer_evaluate_set_q32(mmc_trainer* t, mmc_featureset* fs, int64_t first, int64_t n, int64_t* n_correct,
                                            int64_t* sum_log_loss_q32, void* hip_stream)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!fs) return mmc_fail(MMC_ERR_ARG, "feature set handle is NULL");
    if (!n_correct || !sum_log_loss_q32) return mmc_fail(MMC_ERR_ARG, "n_correct/sum_log_loss is NULL");
    *n_correct = 0;
    *sum_log_loss_q32 = 0;
    int r = check_set_matches(fs, t);
    if (r) return r;
    r = check_set_range(fs, first, n);
    if (r) return r;
    // a row adds at most -log(DBL_EPSILON) * 2^32 < 36.05 * 2^32, so the int64 total holds 2^31 / 36.05 > 5.95e7 rows of the largest loss
    if (n > MMC_EVALUATE_SET_MAX_ROWS)
        return mmc_fail(MMC_ERR_ARG, "n = %lld rows in one call: split it (at most %lld)", (long long)n, (long long)MMC_EVALUATE_SET_MAX_ROWS);
    if (n == 0) return MMC_OK;
    const int K = trainer_classes(t);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(trainer_device(t)));
    const int max_nb = (kTrainerForwardRows + 3) / 4;
    void* scratch = nullptr;
    r = trainer_scratch(t, ((size_t)max_nb * 2 + 2) * 8, &scratch);   // slab [max_nb][2] int64, then the two totals
    if (r) return r;
    long long* slab = static_cast<long long*>(scratch);
    long long* totals = slab + 2 * max_nb;
    HIP_TRY(hipMemsetAsync(totals, 0, 16, st));
    for (int64_t off = 0; off < n; off += kTrainerForwardRows) {
        const int cur = (int)((n - off) < kTrainerForwardRows ? (n - off) : kTrainerForwardRows);
        const int nb = (cur + 3) / 4;
        const float* z = nullptr;
        r = trainer_forward_device(t, fs->X + (size_t)(first + off) * fs->dim, cur, st, &z);
        if (r) return r;
        hipLaunchKernelGGL(eval_rows_kernel<false>, dim3(nb), dim3(256), 0, st, z, fs->y + first + off, cur, K, slab,
                           (unsigned long long*)nullptr);
        hipLaunchKernelGGL(eval_finalize_kernel<true>, dim3(1), dim3(256), 0, st, slab, nb, totals);
        HIP_TRY(hipGetLastError());
    }
    long long h[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(h, totals, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_correct = h[0];
    *sum_log_loss_q32 = h[1];
    return MMC_OK;
}

// The class-wise form of the two evaluations above.  Scratch: slab [max_nb][2] int64, the two totals, the K x K table (totals and
// table are contiguous: one copy brings both back), then -- host-fed only -- the chunk's labels.  Totals and table are zeroed on
// the stream, every chunk adds to them on the device (eval_finalize_kernel<ACC>, the kernel's atomics), and the host reads them
// once after the last chunk.  Integer adds: the totals are those of the calls above on the same rows.
static int trainer_evaluate_classes(mmc_trainer* t, const float* X, const int32_t* y, mmc_featureset* fs, bool from_set, int64_t first,
                                    int64_t n, int64_t* n_correct, int64_t* sum_q32, int64_t* confusion, void* hip_stream)
{
    if (n_correct) *n_correct = 0;
    if (sum_q32) *sum_q32 = 0;
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    const int K = trainer_classes(t);
    const size_t cells = (size_t)K * K;
    if (confusion) for (size_t i = 0; i < cells; ++i) confusion[i] = 0;
    if (!n_correct || !sum_q32) return mmc_fail(MMC_ERR_ARG, "n_correct/sum_log_loss is NULL");
    if (!confusion) return mmc_fail(MMC_ERR_ARG, "confusion is NULL");
    int r;
    if (from_set) {
        if (!fs) return mmc_fail(MMC_ERR_ARG, "feature set handle is NULL");
        r = check_set_matches(fs, t);
        if (r) return r;
        r = check_set_range(fs, first, n);
        if (r) return r;
        if (n > MMC_EVALUATE_SET_MAX_ROWS)
            return mmc_fail(MMC_ERR_ARG, "n = %lld rows in one call: split it (at most %lld)", (long long)n, (long long)MMC_EVALUATE_SET_MAX_ROWS);
    } else {
        if (n < 0) return mmc_fail(MMC_ERR_ARG, "n = %lld is negative", (long long)n);
        if (n > ((int64_t)1 << 25)) return mmc_fail(MMC_ERR_ARG, "n = %lld rows in one call: split it (at most 2^25)", (long long)n);
    }
    if (n == 0) return MMC_OK;
    if (!from_set) {
        if (!X || !y) return mmc_fail(MMC_ERR_ARG, "X/y is NULL");
        r = check_labels(y, n, K);
        if (r) return r;
    }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(trainer_device(t)));
    const int max_nb = (kTrainerForwardRows + 3) / 4;
    void* scratch = nullptr;
    r = trainer_scratch(t, ((size_t)max_nb * 2 + 2 + cells) * 8 + (from_set ? 0 : (size_t)kTrainerForwardRows * 4), &scratch);
    if (r) return r;
    long long* slab = static_cast<long long*>(scratch);
    long long* totals = slab + 2 * max_nb;
    unsigned long long* table = reinterpret_cast<unsigned long long*>(totals + 2);
    int32_t* dy = reinterpret_cast<int32_t*>(table + cells);   // (host-fed only)
    const int d0 = trainer_input_dim(t);
    HIP_TRY(hipMemsetAsync(totals, 0, (2 + cells) * 8, st));
    for (int64_t off = 0; off < n; off += kTrainerForwardRows) {
        const int cur = (int)((n - off) < kTrainerForwardRows ? (n - off) : kTrainerForwardRows);
        const int nb = (cur + 3) / 4;
        const float* z = nullptr;
        const int32_t* labels = dy;
        if (from_set) {
            r = trainer_forward_device(t, fs->X + (size_t)(first + off) * fs->dim, cur, st, &z);
            labels = fs->y + first + off;
        } else {
            if (off) HIP_TRY(hipStreamSynchronize(st));   // the previous chunk has read the labels this one overwrites
            r = trainer_forward(t, X + (size_t)off * d0, cur, st, &z);
        }
        if (r) return r;
        if (!from_set) HIP_TRY(hipMemcpyAsync(dy, y + off, (size_t)cur * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(eval_rows_kernel<true>, dim3(nb), dim3(256), 0, st, z, labels, cur, K, slab, table);
        hipLaunchKernelGGL(eval_finalize_kernel<true>, dim3(1), dim3(256), 0, st, slab, nb, totals);
        HIP_TRY(hipGetLastError());
    }
    std::vector<long long> h(2 + cells, 0);
    HIP_TRY(hipMemcpyAsync(h.data(), totals, (2 + cells) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_correct = h[0];
    *sum_q32 = h[1];
    for (size_t i = 0; i < cells; ++i) confusion[i] = h[2 + i];
    return MMC_OK;
}

extern "C" int mmc_trainer_evaluate_classes(mmc_trainer* t, const float* X, const int32_t* y, int64_t n, int64_t* n_correct,
                                            int64_t* sum_log_loss_q32, int64_t* confusion, void* hip_stream)
{
    return trainer_evaluate_classes(t, X, y, nullptr, false, 0, n, n_correct, sum_log_loss_q32, confusion, hip_stream);
}

extern "C" int mmc_trainer_evaluate_classes_set(mmc_trainer* t, mmc_featureset* fs, int64_t first, int64_t n, int64_t* n_correct,
                                                int64_t* sum_log_loss_q32, int64_t* confusion, void* hip_stream)
{
    return trainer_evaluate_classes(t, nullptr, nullptr, fs, true, first, n, n_correct, sum_log_loss_q32, confusion, hip_stream);
}
