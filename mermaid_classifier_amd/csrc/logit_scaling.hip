// logit_scaling.hip -- logit calibration on the device (gfx950): temperature, bias and vector scaling of a trained head's logits.
// The definition is include/mmc.h, section "logit calibration"; the Newton iteration is logit_newton.h (host); this file holds the
// logit store, the one pass over it, and the C ABI.
//
// Store.  Raw fp32 logits ROW-major, Z[cap][K], next to the labels y[cap]; growth as the Platt calibrator's (doubling, rounded up
// to 1024 rows).  add_features / add_set run the trainer's own forward in chunks of kTrainerForwardRows and copy its logits device
// to device; add_logits uploads the caller's.  The per-class row counts are kept on the host (labels are host data in every add).
//
// Pass (logitcal_pass_kernel<HESS>).  Workgroup b owns rows [b B, (b + 1) B), B = MMC_LOGITCAL_BLOCK_ROWS = 1024, and walks them 32
// at a time: 8 waves x 4 rows.  Each 16-lane row of a wave owns one data row; lane l of it takes classes l, l + 16, ..., so the row
// maximum and the sum of exponentials are butterflies inside the 16 lanes (every lane ends with the same bits).  Float64 throughout:
//   u = fma(a, z, c)   m = max u   e = exp(u - m)   s = sum e   p = e / s   lse = m + log(s)
// The lane that holds class y adds lse - u_y to its loss sum.  v = [z p ; p] (2K entries, zero-padded to T = ceil(2K / 16) tiles of
// 16) goes to LDS, V[32 rows][272], with the row's logits and label beside it.  After a barrier thread k < K walks the 32 rows of its
// class in row order: r = p - [k == y], g_a += z r (fma), g_c += r and, HESS, D_aa += z (z p) (fma), D_ac += z p, D_cc += p -- one
// chain per class over the block's rows, in row order.
//   HESS: the upper triangle of T x T tiles of sum_n v v^T is dealt round-robin to the 8 waves (tile e to wave e % 8: at most 17
//   each, 4 f64 per lane per tile).  For v^T v the A operand of tile i and the B operand of tile j of v_mfma_f64_16x16x4_f64 have
//   the same lane layout (index = lane & 15, k = lane >> 4), so a wave reads V[4 q + (lane >> 4)][16 i + (lane & 15)] and the same
//   with j and issues one MFMA per row quad q = 0..7: a tile's chain runs over the block's row quads in row order.
// The workgroup writes its partials: [g_a K][g_c K][D_aa K][D_ac K][D_cc K][loss] (the loss folded over the 32 row slots in slot
// order) and, HESS, its tiles as they sit in the registers.
// logitcal_sums_kernel folds the blocks' partials in block order; logitcal_hess_kernel does the same per tile, then writes
// H = D - sum v v^T for row <= col and mirrors it, so H is symmetric bit for bit.  No atomics.  The result bits depend on the stored
// logits, labels, K, a, c and N only.  HESS = false is the same code without the D sums and the tiles -- the same loss / gradient
// bits (the file is compiled with contraction off; every fma is written out).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <utility>
#include <vector>

#include "../../include/mmc.h"
#include "logit_newton.h"
#include "trainer_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlockRows = MMC_LOGITCAL_BLOCK_ROWS;   // rows per workgroup: the fixed partition
constexpr int kStepRows = 32;                         // 8 waves x 4 rows
constexpr int kMaxK = MMC_LOGITCAL_MAX_CLASSES;
constexpr int kSlices = kMaxK / 16;                   // classes per lane
constexpr int kVStride = 2 * kMaxK + 16;              // 272 doubles: row r and r + 1 start 32 banks apart
constexpr int kWaves = 8;
constexpr int kMaxTiles = (2 * kMaxK / 16) * (2 * kMaxK / 16 + 1) / 2;   // 136
constexpr int kTilesPerWave = (kMaxTiles + kWaves - 1) / kWaves;         // 17
static_assert(kBlockRows % kStepRows == 0, "a block is a whole number of steps");

typedef double f64x4 __attribute__((ext_vector_type(4)));

inline int tiles_per_side(int K) { return (2 * K + 15) / 16; }
inline int tile_count(int K) { return tiles_per_side(K) * (tiles_per_side(K) + 1) / 2; }
inline size_t sums_len(int K) { return (size_t)5 * K + 1; }

// e-th tile of the upper triangle, row by row: (0,0) (0,1) .. (0,T-1) (1,1) ..
__host__ __device__ inline void tile_of(int e, int T, int& ti, int& tj)
{
    ti = 0;
    int len = T;
    while (e >= len) { e -= len; ++ti; --len; }
    tj = ti + e;
}

__device__ inline double group_max(double v)
{
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ inline double group_sum(double v)
{
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <bool HESS>
__global__ __launch_bounds__(512) void logitcal_pass_kernel(const float* __restrict__ Z, const int32_t* __restrict__ y, int64_t N, int K,
                                                            const double* __restrict__ ac, double* __restrict__ part_s,
                                                            double* __restrict__ part_h)
{
    __shared__ double V[kStepRows][kVStride];   // [z p | p | zero pad] of the step's 32 rows
    __shared__ float Zs[kStepRows][kMaxK];      // their logits
    __shared__ int ys[kStepRows];               // their labels (-1 past the block's last row)
    __shared__ double acs[2 * kMaxK];
    __shared__ int tile_tab[kMaxTiles];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int grp = lane >> 4, l = lane & 15, slot = wave * 4 + grp;
    const int P = 2 * K, T = (P + 15) / 16, nt = T * (T + 1) / 2;
    const int64_t lo = (int64_t)blockIdx.x * kBlockRows, hi = lo + kBlockRows < N ? lo + kBlockRows : N;

    for (int i = tid; i < P; i += 512) acs[i] = ac[i];
    for (int i = tid; i < kStepRows * kVStride; i += 512) (&V[0][0])[i] = 0.0;   // the pad columns [2K, 16 T) stay zero
    if (HESS) {
        for (int e = tid; e < nt; e += 512) {
            int ti, tj;
            tile_of(e, T, ti, tj);
            tile_tab[e] = ti | (tj << 8);
        }
    }
    __syncthreads();

    double ga = 0.0, gc = 0.0, daa = 0.0, dac = 0.0, dcc = 0.0;   // thread k < K: class k's sums over the block's rows, in row order
    double loss = 0.0;                                            // the lane that holds a row's class y: that row's lse - u_y
    f64x4 acc[kTilesPerWave];
    if (HESS) {
#pragma unroll
        for (int t = 0; t < kTilesPerWave; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    }

    for (int64_t r0 = lo; r0 < hi; r0 += kStepRows) {
        const int64_t row = r0 + slot;
        const bool valid = row < hi;
        const float* zrow = Z + (size_t)(valid ? row : lo) * K;
        const int yi = valid ? y[row] : -1;
        if (l == 0) ys[slot] = yi;
        double u[kSlices];
        double m = -INFINITY;
#pragma unroll
        for (int t = 0; t < kSlices; ++t) {
            const int k = l + 16 * t;
            u[t] = -INFINITY;
            if (k < K) {
                const float z = valid ? zrow[k] : 0.f;
                Zs[slot][k] = z;
                if (valid) {
                    u[t] = fma(acs[k], (double)z, acs[K + k]);
                    m = fmax(m, u[t]);
                }
            }
        }
        m = group_max(m);
        double uy = 0.0, s = 0.0;
#pragma unroll
        for (int t = 0; t < kSlices; ++t) {
            const int k = l + 16 * t;
            const bool on = valid && k < K;
            if (on && k == yi) uy = u[t];
            u[t] = on ? exp(u[t] - m) : 0.0;   // u now holds e
            s += u[t];
        }
        s = group_sum(s);
        if (valid && (yi & 15) == l) loss += (m + log(s)) - uy;
#pragma unroll
        for (int t = 0; t < kSlices; ++t) {
            const int k = l + 16 * t;
            if (k < K) {
                const double p = valid ? u[t] / s : 0.0;
                V[slot][k] = (double)Zs[slot][k] * p;
                V[slot][K + k] = p;
            }
        }
        __syncthreads();
        if (tid < K) {
#pragma unroll 4
            for (int rr = 0; rr < kStepRows; ++rr) {
                const double z = (double)Zs[rr][tid], zp = V[rr][tid], p = V[rr][K + tid];
                const double r = p - (ys[rr] == tid ? 1.0 : 0.0);
                ga = fma(z, r, ga);
                gc += r;
                if (HESS) {
                    daa = fma(z, zp, daa);
                    dac += zp;
                    dcc += p;
                }
            }
        }
        if (HESS) {
#pragma unroll
            for (int t = 0; t < kTilesPerWave; ++t) {
                const int e = wave + kWaves * t;
                if (e < nt) {
                    const int tt = __builtin_amdgcn_readfirstlane(tile_tab[e]);
                    const int ca = 16 * (tt & 255) + l, cb = 16 * (tt >> 8) + l;
#pragma unroll
                    for (int q = 0; q < kStepRows / 4; ++q)
                        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(V[4 * q + grp][ca], V[4 * q + grp][cb], acc[t], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // the block's partials: [g_a K][g_c K][D_aa K][D_ac K][D_cc K][loss]
    double* ps = part_s + (size_t)blockIdx.x * ((size_t)5 * K + 1);
    if (tid < K) {
        ps[tid] = ga;
        ps[K + tid] = gc;
        ps[2 * K + tid] = daa;
        ps[3 * K + tid] = dac;
        ps[4 * K + tid] = dcc;
    }
    loss = group_sum(loss);
    if (l == 0) V[slot][0] = loss;
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int rr = 0; rr < kStepRows; ++rr) sum += V[rr][0];
        ps[5 * K] = sum;
    }
    if (HESS) {
        double* ph = part_h + (size_t)blockIdx.x * nt * 256;
#pragma unroll
        for (int t = 0; t < kTilesPerWave; ++t) {
            const int e = wave + kWaves * t;
            if (e < nt) {
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) ph[(size_t)e * 256 + reg * 64 + lane] = acc[t][reg];
            }
        }
    }
}

// sums[i] = the blocks' part_s[b][i] added in block order
__global__ __launch_bounds__(256) void logitcal_sums_kernel(const double* __restrict__ part_s, int nb, int len, double* __restrict__ sums)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += part_s[(size_t)b * len + i];
    sums[i] = s;
}

// one workgroup per tile: the blocks' tiles added in block order, then H = D - sum for row <= col, mirrored
__global__ __launch_bounds__(256) void logitcal_hess_kernel(const double* __restrict__ part_h, int nb, int K, const double* __restrict__ sums,
                                                            double* __restrict__ H)
{
    const int P = 2 * K, T = (P + 15) / 16, nt = T * (T + 1) / 2;
    const int e = blockIdx.x, lane = threadIdx.x & 63, reg = threadIdx.x >> 6;
    int ti, tj;
    tile_of(e, T, ti, tj);
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += part_h[((size_t)b * nt + e) * 256 + threadIdx.x];
    const int row = 16 * ti + (lane >> 4) + 4 * reg, col = 16 * tj + (lane & 15);
    if (row >= P || col >= P || row > col) return;
    double v = -s;
    if (row == col) v = sums[(row < K ? 2 * K : 3 * K) + row] - s;   // D_aa[k] at 2K + k; D_cc[k] at 4K + k = 3K + (K + k)
    else if (row < K && col == row + K) v = sums[3 * K + row] - s;    // D_ac[k]
    H[(size_t)row * P + col] = v;
    H[(size_t)col * P + row] = v;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
struct mmc_logitcal {
    int K = 0, device = 0;
    int64_t n = 0, cap = 0;          // rows stored / allocated
    DevBuf<float> Z;                 // [cap][K] raw logits
    DevBuf<int32_t> y;               // [cap]
    std::vector<int64_t> counts;     // rows per class
    DevBuf<double> ac, sums, H;      // [2K], [5K + 1], [2K][2K]
    DevBuf<double> part;             // the blocks' partials: sums, then tiles
};

static int logitcal_reserve(mmc_logitcal* c, int64_t need, hipStream_t st)
{
    if (need <= c->cap) return MMC_OK;
    int64_t cap = c->cap * 2 > need ? c->cap * 2 : need;
    cap = (cap + 1023) / 1024 * 1024;
    DevBuf<float> Z;
    DevBuf<int32_t> y;
    if (!Z.alloc(cap * c->K)) return mmc_fail(MMC_ERR_NOMEM, "hipMalloc of %lld x %d logits failed", (long long)cap, c->K);
    if (!y.alloc(cap)) return mmc_fail(MMC_ERR_NOMEM, "hipMalloc of %lld labels failed", (long long)cap);
    if (c->n) {
        hipError_t e = hipMemcpyAsync(Z, c->Z, (size_t)c->n * c->K * 4, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(y, c->y, (size_t)c->n * 4, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return mmc_fail(MMC_ERR_HIP, "moving the logit store: %s", hipGetErrorString(e));
    }
    c->Z = std::move(Z);
    c->y = std::move(y);
    c->cap = cap;
    return MMC_OK;
}

extern "C" void mmc_logitcal_destroy(mmc_logitcal* c)
{
    if (!c) return;
    hipSetDevice(c->device);
    delete c;
}

extern "C" int mmc_logitcal_create(int K, int device, mmc_logitcal** out)
{
    if (!out) return mmc_fail(MMC_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (K < 2 || K > kMaxK) return mmc_fail(MMC_ERR_ARG, "K = %d outside [2, %d]", K, kMaxK);
    if (int r = check_device(device)) return r;
    HIP_TRY(hipSetDevice(device));
    mmc_logitcal* c = new mmc_logitcal();
    c->K = K;
    c->device = device;
    c->counts.assign(K, 0);
    const bool ok = c->ac.alloc(2 * K) && c->sums.alloc((int64_t)sums_len(K)) && c->H.alloc((int64_t)4 * K * K);
    if (!ok) {
        mmc_logitcal_destroy(c);
        return mmc_fail(MMC_ERR_NOMEM, "hipMalloc failed while creating the logit calibrator");
    }
    *out = c;
    return MMC_OK;
}

extern "C" int64_t mmc_logitcal_rows(const mmc_logitcal* c) { return c ? c->n : 0; }

static int logitcal_check_trainer(const mmc_logitcal* c, mmc_trainer* t)
{
    if (!c || !t) return mmc_fail(MMC_ERR_ARG, "logit calibrator/trainer handle is NULL");
    if (trainer_classes(t) != c->K) return mmc_fail(MMC_ERR_ARG, "trainer has K = %d classes, logit calibrator K = %d", trainer_classes(t), c->K);
    if (trainer_device(t) != c->device)
        return mmc_fail(MMC_ERR_ARG, "trainer is on device %d, logit calibrator on device %d", trainer_device(t), c->device);
    return MMC_OK;
}

extern "C" int mmc_logitcal_add_features(mmc_logitcal* c, mmc_trainer* t, const float* X, const int32_t* y, int64_t n, void* hip_stream)
{
    int r = logitcal_check_trainer(c, t);
    if (r) return r;
    if (n < 0) return mmc_fail(MMC_ERR_ARG, "n = %lld is negative", (long long)n);
    if (n == 0) return MMC_OK;
    if (!X || !y) return mmc_fail(MMC_ERR_ARG, "X/y is NULL");
    r = check_labels(y, n, c->K);
    if (r) return r;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(c->device));
    r = logitcal_reserve(c, c->n + n, st);
    if (r) return r;
    const int d0 = trainer_input_dim(t);
    for (int64_t off = 0; off < n; off += kTrainerForwardRows) {
        const int cur = (int)((n - off) < kTrainerForwardRows ? (n - off) : kTrainerForwardRows);
        const float* z = nullptr;
        r = trainer_forward(t, X + (size_t)off * d0, cur, st, &z);
        if (r) return r;
        HIP_TRY(hipMemcpyAsync(c->Z + (size_t)(c->n + off) * c->K, z, (size_t)cur * c->K * 4, hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(c->y + c->n, y, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int64_t i = 0; i < n; ++i) ++c->counts[y[i]];
    c->n += n;
    return MMC_OK;
}

extern "C" int mmc_logitcal_add_set(mmc_logitcal* c, mmc_trainer* t, mmc_featureset* fs, int64_t first, int64_t n, void* hip_stream)
{
    int r = logitcal_check_trainer(c, t);
    if (r) return r;
    if (!fs) return mmc_fail(MMC_ERR_ARG, "feature set handle is NULL");
    r = check_set_matches(fs, t);
    if (r) return r;
    r = check_set_range(fs, first, n);
    if (r) return r;
    if (n == 0) return MMC_OK;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(c->device));
    r = logitcal_reserve(c, c->n + n, st);
    if (r) return r;
    for (int64_t off = 0; off < n; off += kTrainerForwardRows) {
        const int cur = (int)((n - off) < kTrainerForwardRows ? (n - off) : kTrainerForwardRows);
        const float* z = nullptr;
        r = trainer_forward_device(t, fs->X + (size_t)(first + off) * fs->dim, cur, st, &z);
        if (r) return r;
        HIP_TRY(hipMemcpyAsync(c->Z + (size_t)(c->n + off) * c->K, z, (size_t)cur * c->K * 4, hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(c->y + c->n, fs->y + first, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int64_t i = 0; i < n; ++i) ++c->counts[fs->y_host[(size_t)(first + i)]];
    c->n += n;
    return MMC_OK;
}

extern "C" int mmc_logitcal_add_logits(mmc_logitcal* c, const float* logits, const int32_t* y, int64_t n, void* hip_stream)
{
    if (!c) return mmc_fail(MMC_ERR_ARG, "logit calibrator handle is NULL");
    if (n < 0) return mmc_fail(MMC_ERR_ARG, "n = %lld is negative", (long long)n);
    if (n == 0) return MMC_OK;
    if (!logits || !y) return mmc_fail(MMC_ERR_ARG, "logits/y is NULL");
    int r = check_labels(y, n, c->K);
    if (r) return r;
    for (int64_t i = 0; i < n * c->K; ++i)
        if (!std::isfinite(logits[i]))
            return mmc_fail(MMC_ERR_ARG, "logits[%lld][%d] = %g is not finite", (long long)(i / c->K), (int)(i % c->K), (double)logits[i]);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(c->device));
    r = logitcal_reserve(c, c->n + n, st);
    if (r) return r;
    HIP_TRY(hipMemcpyAsync(c->Z + (size_t)c->n * c->K, logits, (size_t)n * c->K * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c->y + c->n, y, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int64_t i = 0; i < n; ++i) ++c->counts[y[i]];
    c->n += n;
    return MMC_OK;
}

static int check_finite_params(const double* a, const double* cc, int K)
{
    for (int k = 0; k < K; ++k)
        if (!std::isfinite(a[k]) || !std::isfinite(cc[k])) return mmc_fail(MMC_ERR_ARG, "a[%d] = %g / c[%d] = %g is not finite", k, a[k], k, cc[k]);
    return MMC_OK;
}

// one pass at (a, cc): *nll = data term, grad[2K], hess[2K x 2K] when not NULL.  Arguments are checked by the callers.
static int logitcal_pass(mmc_logitcal* c, const double* a, const double* cc, double* nll, double* grad, double* hess, hipStream_t st)
{
    const int K = c->K, P = 2 * K, nt = tile_count(K);
    const int64_t nb64 = (c->n + kBlockRows - 1) / kBlockRows;
    if (nb64 > (int64_t)1 << 22) return mmc_fail(MMC_ERR_ARG, "%lld stored rows: more than 2^32", (long long)c->n);
    const int nb = (int)nb64;
    const size_t len_s = sums_len(K), need = (size_t)nb * len_s + (hess ? (size_t)nb * nt * 256 : 0);
    if ((int64_t)need > c->part.cap) {
        DevBuf<double> p;
        if (!p.alloc((int64_t)need)) return mmc_fail(MMC_ERR_NOMEM, "hipMalloc of %zu bytes of block partials failed", need * 8);
        c->part = std::move(p);
    }
    double* part_s = c->part;
    double* part_h = c->part + (size_t)nb * len_s;
    std::vector<double> host(P);
    for (int k = 0; k < K; ++k) { host[k] = a[k]; host[K + k] = cc[k]; }
    HIP_TRY(hipMemcpyAsync(c->ac, host.data(), (size_t)P * 8, hipMemcpyHostToDevice, st));
    if (hess) hipLaunchKernelGGL(logitcal_pass_kernel<true>, dim3(nb), dim3(512), 0, st, c->Z, c->y, c->n, K, c->ac, part_s, part_h);
    else hipLaunchKernelGGL(logitcal_pass_kernel<false>, dim3(nb), dim3(512), 0, st, c->Z, c->y, c->n, K, c->ac, part_s, (double*)nullptr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(logitcal_sums_kernel, dim3(((int)len_s + 255) / 256), dim3(256), 0, st, part_s, nb, (int)len_s, c->sums);
    HIP_TRY(hipGetLastError());
    if (hess) {
        hipLaunchKernelGGL(logitcal_hess_kernel, dim3(nt), dim3(256), 0, st, part_h, nb, K, c->sums, c->H);
        HIP_TRY(hipGetLastError());
    }
    std::vector<double> sums(len_s);
    HIP_TRY(hipMemcpyAsync(sums.data(), c->sums, len_s * 8, hipMemcpyDeviceToHost, st));
    if (hess) HIP_TRY(hipMemcpyAsync(hess, c->H, (size_t)P * P * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // (also before `host` leaves scope)
    for (int i = 0; i < P; ++i) grad[i] = sums[i];
    *nll = sums[5 * K];
    return MMC_OK;
}

extern "C" int mmc_logitcal_stats(mmc_logitcal* c, const double* a, const double* cc, double* nll_sum, double* grad, double* hess,
                                  int64_t* counts, void* hip_stream)
{
    if (!c) return mmc_fail(MMC_ERR_ARG, "logit calibrator handle is NULL");
    if (!a || !cc) return mmc_fail(MMC_ERR_ARG, "a/c is NULL");
    if (!nll_sum || !grad) return mmc_fail(MMC_ERR_ARG, "nll_sum/grad is NULL");
    int r = check_finite_params(a, cc, c->K);
    if (r) return r;
    if (c->n < 1) return mmc_fail(MMC_ERR_ARG, "stats with no rows: add features or logits first");
    HIP_TRY(hipSetDevice(c->device));
    r = logitcal_pass(c, a, cc, nll_sum, grad, hess, static_cast<hipStream_t>(hip_stream));
    if (r) return r;
    if (counts)
        for (int k = 0; k < c->K; ++k) counts[k] = c->counts[k];
    return MMC_OK;
}

extern "C" int mmc_logitcal_fit(mmc_logitcal* c, int mode, double l2, double tol, int max_trials, double* a, double* cc, uint8_t* frozen,
                                double* nll_before, double* nll_after, int32_t* trials, int32_t* converged, void* hip_stream)
{
    if (!c) return mmc_fail(MMC_ERR_ARG, "logit calibrator handle is NULL");
    if (!a || !cc) return mmc_fail(MMC_ERR_ARG, "a/c is NULL");
    if (!nll_before || !nll_after || !trials || !converged) return mmc_fail(MMC_ERR_ARG, "nll_before/nll_after/trials/converged is NULL");
    if (mode != MMC_LOGITCAL_TEMPERATURE && mode != MMC_LOGITCAL_BIAS && mode != MMC_LOGITCAL_VECTOR)
        return mmc_fail(MMC_ERR_ARG, "mode %d is none of TEMPERATURE, BIAS, VECTOR", mode);
    if (!(l2 >= 0.0) || !std::isfinite(l2)) return mmc_fail(MMC_ERR_ARG, "l2 = %g must be finite and >= 0", l2);
    if (!(tol > 0.0) || !std::isfinite(tol)) return mmc_fail(MMC_ERR_ARG, "tol = %g must be finite and > 0", tol);
    if (max_trials < 1 || max_trials > 1000) return mmc_fail(MMC_ERR_ARG, "max_trials = %d outside [1, 1000]", max_trials);
    if (c->n < 1) return mmc_fail(MMC_ERR_ARG, "fit with no rows: add features or logits first");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(c->device));
    const int K = c->K;
    std::vector<uint8_t> fz(K);
    logit_newton::frozen_mask(K, mode, c->counts.data(), fz.data());
    logit_newton::FitResult res;
    auto eval = [&](const double* pa, const double* pc, bool want_hess, double* f, double* g, double* H) {
        return logitcal_pass(c, pa, pc, f, g, want_hess ? H : nullptr, st);
    };
    const int r = logit_newton::fit(K, mode, l2, tol, max_trials, c->n, fz.data(), eval, a, cc, &res);
    if (r < 0) return mmc_fail(MMC_ERR_ARG, "the stored logits give a non-finite loss at the identity");
    if (r) return r;
    if (frozen)
        for (int k = 0; k < K; ++k) frozen[k] = fz[k];
    *nll_before = res.f_before / (double)c->n;
    *nll_after = res.f_after / (double)c->n;
    *trials = res.trials;
    *converged = res.converged;
    return MMC_OK;
}
