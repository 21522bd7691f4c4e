// features.hip -- fitted linear feature transforms on a resident feature set (gfx950): mmc_featureset_moments,
// mmc_featureset_scatter, mmc_featureset_transform.  No reference counterpart: include/mmc.h "feature transforms" is the definition.
//
// The reference trains its MLP on raw pooled activations (mermaid_classifier/pyspacer/trainer.py:118-145); its research notes
// (docs/research/hidden-layer-experiments.md section 5) point at the feature representation as the next thing to vary.  The three
// entries are what standardisation, PCA and whitening need from the device: per-class and global moments, the scatter matrix of the
// centred rows, and the fused centre-and-project pass into another resident set.  The eigen-decomposition of the dim x dim scatter is
// host work (feature_transform.py).
//
// Determinism: no float atomics.  Every fp64 sum is cut into pieces by a table the host derives from (labels, first, n) -- moments --
// or from (n, dim) -- scatter --, each piece is summed in row order by one thread or one MFMA accumulator chain, and a second launch
// adds the pieces in ascending order.  Neither the CU count nor the dispatch order enters.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <new>
#include <vector>

#include "../../include/mmc.h"
#include "trainer_internal.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// ---- moments ------------------------------------------------------------------------------------------------------------------
// A slab: at most 256 consecutive members of one group.  Groups 0..K-1 are the classes, whose members are order[start .. start+count)
// (rows in ascending order: a stable counting sort of the labels); group K is every row, members start .. start+count themselves.
struct Slab { int32_t group, start, count; };
constexpr int kSlabRows = 256;

// one thread per (slab, column): the slab's rows in order, fp64.  CENTRED: squares of the deviation from the group's mean.
template <bool CENTRED>
__global__ __launch_bounds__(256) void moments_pass_kernel(const float* __restrict__ X, int dim, const int32_t* __restrict__ order,
                                                           const Slab* __restrict__ slabs, int K, const double* __restrict__ mean,
                                                           double* __restrict__ partial)
{
    const int j = blockIdx.y * 256 + threadIdx.x;
    if (j >= dim) return;
    const Slab s = slabs[blockIdx.x];
    const double mu = CENTRED ? mean[(size_t)s.group * dim + j] : 0.0;
    double acc = 0.0;
    for (int i = 0; i < s.count; ++i) {
        const int64_t row = s.group == K ? (int64_t)s.start + i : (int64_t)order[s.start + i];
        const double v = (double)X[row * dim + j];
        if (CENTRED) {
            const double d = v - mu;
            acc = fma(d, d, acc);
        } else {
            acc += v;
        }
    }
    partial[(size_t)blockIdx.x * dim + j] = acc;
}

// one thread per (group, column): the group's slabs in ascending order; divide: the mean (0 for an empty group)
__global__ __launch_bounds__(256) void moments_reduce_kernel(const double* __restrict__ partial, const int32_t* __restrict__ slab_off,
                                                             const int64_t* __restrict__ counts, int dim, int divide,
                                                             double* __restrict__ out)
{
    const int j = blockIdx.y * 256 + threadIdx.x, g = blockIdx.x;
    if (j >= dim) return;
    double acc = 0.0;
    for (int s = slab_off[g]; s < slab_off[g + 1]; ++s) acc += partial[(size_t)s * dim + j];
    if (divide) {
        const int64_t c = counts[g];
        acc = c ? acc / (double)c : 0.0;
    }
    out[(size_t)g * dim + j] = acc;
}

// ---- scatter ------------------------------------------------------------------------------------------------------------------
// S = sum over rows of (x - c)^T (x - c): tgemm_f32_tile's TA = 1, TB = 0 form with A = B = X, so the k-major LDS tiles are rows of X.
// 128 x 128 output tile per 256-thread workgroup, 16 rows per stage; wave w owns the 64 x 64 quadrant (w>>1, w&1) as 4 x 4 fragments of
// v_mfma_f32_16x16x4_f32 (16 independent accumulators per wave).  Rows come in chunks of MMC_SCATTER_CHUNK_ROWS: inside a chunk the
// accumulators are fp32 (one k-ordered fmaf chain per element), at its end each lane adds them into fp64 registers and clears them.
// A workgroup handles one tile pair (tile_m <= tile_n) over one contiguous range of chunks and writes its 128 x 128 fp64 partial.
constexpr int kST = 128;    // tile edge
constexpr int kSK = 16;     // rows per stage
constexpr int kSLD = 144;   // LDS row stride in floats: the four k-rows of one fragment read land on disjoint banks; 16-byte rows
constexpr int kStagesPerChunk = MMC_SCATTER_CHUNK_ROWS / kSK;

struct Staged {   // one thread's share of a stage: 4 columns of rows r and r + 8, of both operands; x and its centre, uncentred
    f4 xa[2], ca[2], xb[2], cb[2];
};

template <bool VEC>
__device__ __forceinline__ void stage_load4(const float* __restrict__ X, const int32_t* __restrict__ y,
                                            const float* __restrict__ centres, int64_t row, int64_t n, int col, int dim, f4& x, f4& c)
{
    // rows past n and columns past dim stay 0 - 0: zero AFTER centring
    x = (f4){0.f, 0.f, 0.f, 0.f};
    c = (f4){0.f, 0.f, 0.f, 0.f};
    if (row >= n || col >= dim) return;
    const float* xp = X + (size_t)row * dim + col;
    const float* cp = centres + (y ? (size_t)y[row] * dim : (size_t)0) + col;
    if (VEC) {
        x = *reinterpret_cast<const f4*>(xp);
        c = *reinterpret_cast<const f4*>(cp);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (col + e < dim) {
                x[e] = xp[e];
                c[e] = cp[e];
            }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256, 2) void scatter_kernel(const float* __restrict__ X, const int32_t* __restrict__ y /* null: one centre */,
                                                      const float* __restrict__ centres, int64_t n, int dim, int n_chunks, int n_splits,
                                                      int tiles, double* __restrict__ partial)
{
    __shared__ __attribute__((aligned(16))) float As[kSK][kSLD];
    __shared__ __attribute__((aligned(16))) float Bs[kSK][kSLD];
    // blockIdx.x walks the upper triangle row by row: (0,0) (0,1) .. (0,T-1) (1,1) ..
    int tm = 0, tn = blockIdx.x;
    for (int len = tiles; tn >= len; --len) {
        tn -= len;
        ++tm;
    }
    tn += tm;
    const int split = blockIdx.y;
    const int c0 = (int)((int64_t)split * n_chunks / n_splits), c1 = (int)((int64_t)(split + 1) * n_chunks / n_splits);
    const int64_t all_stages = (n + kSK - 1) / kSK;
    const int64_t st0 = (int64_t)c0 * kStagesPerChunk;
    const int64_t st1 = (int64_t)c1 * kStagesPerChunk < all_stages ? (int64_t)c1 * kStagesPerChunk : all_stages;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int li = lane & 15, lq = lane >> 4;
    const int srow = tid >> 5, scol = (tid & 31) * 4;          // staging: rows srow and srow + 8, columns scol .. scol + 3
    const int col_a = tm * kST + scol, col_b = tn * kST + scol;

    f4 acc[4][4];
    double sum[4][4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            acc[a][b] = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 4; ++r) sum[a][b][r] = 0.0;
        }

    Staged g;
    if (st0 < st1) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int64_t row = st0 * kSK + srow + 8 * r;
            stage_load4<VEC>(X, y, centres, row, n, col_a, dim, g.xa[r], g.ca[r]);
            stage_load4<VEC>(X, y, centres, row, n, col_b, dim, g.xb[r], g.cb[r]);
        }
    }
    for (int64_t st = st0; st < st1; ++st) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            // the operand: fl32(x - c), one rounding
            *reinterpret_cast<f4*>(&As[srow + 8 * r][scol]) = g.xa[r] - g.ca[r];
            *reinterpret_cast<f4*>(&Bs[srow + 8 * r][scol]) = g.xb[r] - g.cb[r];
        }
        __syncthreads();
        if (st + 1 < st1) {   // the next stage's loads fly during this stage's MFMAs
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int64_t row = (st + 1) * kSK + srow + 8 * r;
                stage_load4<VEC>(X, y, centres, row, n, col_a, dim, g.xa[r], g.ca[r]);
                stage_load4<VEC>(X, y, centres, row, n, col_b, dim, g.xb[r], g.cb[r]);
            }
        }
#pragma unroll
        for (int kk = 0; kk < kSK; kk += 4) {
            float av[4], bv[4];
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                av[f] = As[kk + lq][wm + f * 16 + li];
                bv[f] = Bs[kk + lq][wn + f * 16 + li];
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bv[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();
        if ((st + 1) % kStagesPerChunk == 0 || st + 1 == st1) {   // the chunk's end: fold into fp64, clear
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) sum[a][b][r] += (double)acc[a][b][r];
                    acc[a][b] = (f4){0.f, 0.f, 0.f, 0.f};
                }
        }
    }
    // lane (li, lq) holds element [wm + 16a + 4 lq + r][wn + 16b + li] of the tile
    double* out = partial + ((size_t)split * gridDim.x + blockIdx.x) * (kST * kST);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(size_t)(wm + 16 * a + 4 * lq + r) * kST + wn + 16 * b + li] = sum[a][b][r];
}

// one thread per element of a tile pair's upper part: the splits in ascending order, written to (i, j) and mirrored to (j, i)
__global__ __launch_bounds__(256) void scatter_reduce_kernel(const double* __restrict__ partial, int n_splits, int tiles, int dim,
                                                             double* __restrict__ S)
{
    int tm = 0, tn = blockIdx.x;
    for (int len = tiles; tn >= len; --len) {
        tn -= len;
        ++tm;
    }
    tn += tm;
    const int e = blockIdx.y * 256 + threadIdx.x, mi = e / kST, nj = e % kST;
    const int gi = tm * kST + mi, gj = tn * kST + nj;
    if (gi >= dim || gj >= dim || (tm == tn && mi > nj)) return;
    double acc = 0.0;
    for (int s = 0; s < n_splits; ++s) acc += partial[((size_t)s * gridDim.x + blockIdx.x) * (kST * kST) + e];
    S[(size_t)gi * dim + gj] = acc;
    S[(size_t)gj * dim + gi] = acc;
}

// ---- transform ----------------------------------------------------------------------------------------------------------------
// Y[n][m] = (X - centre) . T^T: tgemm_f32_tile's TA = 0, TB = 1 form with the centring at staging time; 64 x 64 tile, 2 x 2 fragments
// per wave, one fp32 accumulator chain over dim in ascending k -- the rounding of every other fp32 GEMM here.
__global__ __launch_bounds__(256) void transform_kernel(const float* __restrict__ X, const float* __restrict__ centre,
                                                        const float* __restrict__ T, float* __restrict__ Y, int64_t n, int dim, int m)
{
    __shared__ float As[16][68];
    __shared__ float Bs[16][68];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * 64;
    const int n0 = blockIdx.y * 64;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int li = lane & 15, lq = lane >> 4;
    f4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (f4){0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < dim; k0 += 16) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int idx = tid + 256 * r, rr = idx >> 4, k = idx & 15, gk = k0 + k;
            const int64_t gm = m0 + rr;
            const int gn = n0 + rr;
            float va = 0.f, vb = 0.f;
            if (gm < n && gk < dim) va = X[(size_t)gm * dim + gk] - centre[gk];   // zero AFTER centring
            if (gn < m && gk < dim) vb = T[(size_t)gn * dim + gk];
            As[k][rr] = va;
            Bs[k][rr] = vb;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; kk += 4) {
            float av[2], bv[2];
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                av[f] = As[kk + lq][wm + f * 16 + li];
                bv[f] = Bs[kk + lq][wn + f * 16 + li];
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bv[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = m0 + wm + 16 * a + 4 * lq + r;
                const int col = n0 + wn + 16 * b + li;
                if (row < n && col < m) Y[(size_t)row * m + col] = acc[a][b][r];
            }
}

int check_range(const mmc_featureset* fs, int64_t first, int64_t n)
{
    if (!fs) return mmc_fail(MMC_ERR_ARG, "feature set handle is NULL");
    if (first < 0 || n < 0 || first > fs->n || n > fs->n - first)
        return mmc_fail(MMC_ERR_ARG, "rows [%lld, %lld + %lld) outside the set's %lld rows", (long long)first, (long long)first,
                        (long long)n, (long long)fs->n);
    if (n > 0x7fffffff) return mmc_fail(MMC_ERR_ARG, "n = %lld: at most 2^31 - 1 rows per call", (long long)n);
    return MMC_OK;
}

// zeroes / fills an output that is host memory (flag set) or device memory
int put_output(void* dst, const void* host_src /* null: zeros */, size_t bytes, bool host, hipStream_t st)
{
    if (host) {
        if (host_src) memcpy(dst, host_src, bytes);
        else memset(dst, 0, bytes);
        return MMC_OK;
    }
    if (host_src) HIP_TRY(hipMemcpyAsync(dst, host_src, bytes, hipMemcpyHostToDevice, st));
    else HIP_TRY(hipMemsetAsync(dst, 0, bytes, st));
    return MMC_OK;
}

}   // namespace

// the number of contiguous chunk ranges mmc_featureset_scatter cuts n rows of width dim into: include/mmc.h gives the rule
static int scatter_splits(int64_t n, int dim)
{
    const int64_t chunks = (n + MMC_SCATTER_CHUNK_ROWS - 1) / MMC_SCATTER_CHUNK_ROWS;
    const int tiles = (dim + kST - 1) / kST, pairs = tiles * (tiles + 1) / 2;
    int64_t s = 512 / pairs;
    if (s > MMC_SCATTER_MAX_SPLITS) s = MMC_SCATTER_MAX_SPLITS;
    if (s > chunks) s = chunks;
    return s < 1 ? 1 : (int)s;
}

extern "C" int mmc_featureset_moments(mmc_featureset* fs, int64_t first, int64_t n, int64_t* counts, double* mean, double* m2,
                                      unsigned flags, void* hip_stream)
{
    const int rc = check_range(fs, first, n);
    if (rc) return rc;
    if (!counts || !mean || !m2) return mmc_fail(MMC_ERR_ARG, "counts / mean / m2 is NULL");
    if (flags & ~MMC_OUT_HOST) return mmc_fail(MMC_ERR_ARG, "flags 0x%x: only MMC_OUT_HOST is defined here", flags);
    const bool host = flags & MMC_OUT_HOST;
    const int K = fs->K, dim = fs->dim;
    const size_t cells = (size_t)(K + 1) * dim;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(fs->device));

    // the slab table: a stable counting sort of the labels gives every class its rows in ascending order
    std::vector<int64_t> cnt;
    std::vector<int32_t> order, slab_off;
    std::vector<Slab> slabs;
    try {
        cnt.assign((size_t)K + 1, 0);
        const int32_t* y = fs->y_host.data() + first;
        for (int64_t i = 0; i < n; ++i) ++cnt[(size_t)y[i]];
        cnt[(size_t)K] = n;
        std::vector<int64_t> at((size_t)K, 0);
        for (int g = 1; g < K; ++g) at[(size_t)g] = at[(size_t)g - 1] + cnt[(size_t)g - 1];
        const std::vector<int64_t> off(at);
        order.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) order[(size_t)at[(size_t)y[i]]++] = (int32_t)i;
        slab_off.resize((size_t)K + 2);
        for (int g = 0; g <= K; ++g) {
            slab_off[(size_t)g] = (int32_t)slabs.size();
            const int64_t base = g == K ? 0 : off[(size_t)g];
            for (int64_t s = 0; s < cnt[(size_t)g]; s += kSlabRows) {
                const int64_t left = cnt[(size_t)g] - s;
                slabs.push_back(Slab{g, (int32_t)(base + s), (int32_t)(left < kSlabRows ? left : kSlabRows)});
            }
        }
        slab_off[(size_t)K + 1] = (int32_t)slabs.size();
    } catch (const std::bad_alloc&) {
        return mmc_fail(MMC_ERR_NOMEM, "no host memory for the slab table of %lld rows", (long long)n);
    }
    if (n == 0) {
        int r = put_output(counts, nullptr, (size_t)K * 8, host, st);
        if (!r) r = put_output(mean, nullptr, cells * 8, host, st);
        if (!r) r = put_output(m2, nullptr, cells * 8, host, st);
        if (r) return r;
        HIP_TRY(hipStreamSynchronize(st));
        return MMC_OK;
    }

    const size_t n_slabs = slabs.size();
    const size_t o_order = 0, o_slabs = o_order + align256((size_t)n * 4), o_off = o_slabs + align256(n_slabs * sizeof(Slab)),
                 o_cnt = o_off + align256(((size_t)K + 2) * 4), o_partial = o_cnt + align256(((size_t)K + 1) * 8),
                 o_mean = o_partial + align256(n_slabs * dim * 8), o_m2 = o_mean + align256(cells * 8), total = o_m2 + align256(cells * 8);
    DevBuf<char> mem;   // a per-call device allocation, freed on every way out
    if (!mem.alloc((int64_t)total)) return mmc_fail(MMC_ERR_NOMEM, "hipMalloc of %zu bytes of moments scratch failed", total);
    int32_t* d_order = (int32_t*)(mem.p + o_order);
    Slab* d_slabs = (Slab*)(mem.p + o_slabs);
    int32_t* d_off = (int32_t*)(mem.p + o_off);
    int64_t* d_cnt = (int64_t*)(mem.p + o_cnt);
    double* d_partial = (double*)(mem.p + o_partial);
    double* d_mean = host ? (double*)(mem.p + o_mean) : mean;
    double* d_m2 = host ? (double*)(mem.p + o_m2) : m2;
    HIP_TRY(hipMemcpyAsync(d_order, order.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_slabs, slabs.data(), n_slabs * sizeof(Slab), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_off, slab_off.data(), ((size_t)K + 2) * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_cnt, cnt.data(), ((size_t)K + 1) * 8, hipMemcpyHostToDevice, st));

    const float* X = fs->X + (size_t)first * dim;
    const dim3 pass_grid((unsigned)n_slabs, (unsigned)((dim + 255) / 256)), red_grid((unsigned)(K + 1), (unsigned)((dim + 255) / 256));
    moments_pass_kernel<false><<<pass_grid, 256, 0, st>>>(X, dim, d_order, d_slabs, K, nullptr, d_partial);
    moments_reduce_kernel<<<red_grid, 256, 0, st>>>(d_partial, d_off, d_cnt, dim, 1, d_mean);
    moments_pass_kernel<true><<<pass_grid, 256, 0, st>>>(X, dim, d_order, d_slabs, K, d_mean, d_partial);
    moments_reduce_kernel<<<red_grid, 256, 0, st>>>(d_partial, d_off, d_cnt, dim, 0, d_m2);
    HIP_TRY(hipGetLastError());
    if (host) {
        HIP_TRY(hipMemcpyAsync(mean, d_mean, cells * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(m2, d_m2, cells * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        memcpy(counts, cnt.data(), (size_t)K * 8);
    } else {
        HIP_TRY(hipMemcpyAsync(counts, d_cnt, (size_t)K * 8, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));   // the scratch is freed on return
    }
    return MMC_OK;
}

extern "C" int mmc_featureset_scatter(mmc_featureset* fs, int64_t first, int64_t n, const float* centres, int by_label, double* scatter,
                                      unsigned flags, void* hip_stream)
{
    const int rc = check_range(fs, first, n);
    if (rc) return rc;
    if (!centres || !scatter) return mmc_fail(MMC_ERR_ARG, "centres / scatter is NULL");
    if (by_label != 0 && by_label != 1) return mmc_fail(MMC_ERR_ARG, "by_label = %d must be 0 or 1", by_label);
    if (flags & ~(MMC_IN_HOST | MMC_OUT_HOST)) return mmc_fail(MMC_ERR_ARG, "flags 0x%x: only MMC_IN_HOST and MMC_OUT_HOST are defined", flags);
    const int dim = fs->dim;
    if (dim > MMC_SCATTER_MAX_DIM) return mmc_fail(MMC_ERR_ARG, "dim = %d exceeds MMC_SCATTER_MAX_DIM = %d", dim, MMC_SCATTER_MAX_DIM);
    const bool in_host = flags & MMC_IN_HOST, out_host = flags & MMC_OUT_HOST;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(fs->device));
    const size_t out_bytes = (size_t)dim * dim * 8;
    if (n == 0) {
        const int r = put_output(scatter, nullptr, out_bytes, out_host, st);
        if (r) return r;
        HIP_TRY(hipStreamSynchronize(st));
        return MMC_OK;
    }
    const int splits = scatter_splits(n, dim);
    const int chunks = (int)((n + MMC_SCATTER_CHUNK_ROWS - 1) / MMC_SCATTER_CHUNK_ROWS);
    const int tiles = (dim + kST - 1) / kST, pairs = tiles * (tiles + 1) / 2;
    const size_t centre_bytes = (size_t)(by_label ? fs->K : 1) * dim * 4;
    const size_t o_partial = 0, o_centres = o_partial + align256((size_t)splits * pairs * kST * kST * 8),
                 o_out = o_centres + align256(in_host ? centre_bytes : 0), total = o_out + align256(out_host ? out_bytes : 0);
    DevBuf<char> mem;   // a per-call device allocation, freed on every way out
    if (!mem.alloc((int64_t)total)) return mmc_fail(MMC_ERR_NOMEM, "hipMalloc of %zu bytes of scatter scratch failed", total);
    double* d_partial = (double*)(mem.p + o_partial);
    const float* d_centres = centres;
    if (in_host) {
        HIP_TRY(hipMemcpyAsync(mem.p + o_centres, centres, centre_bytes, hipMemcpyHostToDevice, st));
        d_centres = (const float*)(mem.p + o_centres);
    }
    double* d_out = out_host ? (double*)(mem.p + o_out) : scatter;
    const float* X = fs->X + (size_t)first * dim;
    const int32_t* y = by_label ? fs->y + first : nullptr;
    const dim3 grid((unsigned)pairs, (unsigned)splits);
    const bool vec = dim % 4 == 0 && (uintptr_t)X % 16 == 0 && (uintptr_t)d_centres % 16 == 0;
    if (vec) scatter_kernel<true><<<grid, 256, 0, st>>>(X, y, d_centres, n, dim, chunks, splits, tiles, d_partial);
    else scatter_kernel<false><<<grid, 256, 0, st>>>(X, y, d_centres, n, dim, chunks, splits, tiles, d_partial);
    scatter_reduce_kernel<<<dim3((unsigned)pairs, kST * kST / 256), 256, 0, st>>>(d_partial, splits, tiles, dim, d_out);
    HIP_TRY(hipGetLastError());
    if (out_host) HIP_TRY(hipMemcpyAsync(scatter, d_out, out_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // the scratch is freed on return
    return MMC_OK;
}

extern "C" int mmc_featureset_transform(mmc_featureset* src, int64_t first, int64_t n, const float* centre, const float* T, int m,
                                        mmc_featureset* dst, unsigned flags, void* hip_stream)
{
    const int rc = check_range(src, first, n);
    if (rc) return rc;
    if (!dst) return mmc_fail(MMC_ERR_ARG, "dst is NULL");
    if (dst == src) return mmc_fail(MMC_ERR_ARG, "dst is src: a set cannot be transformed into itself");
    if (!centre || !T) return mmc_fail(MMC_ERR_ARG, "centre / T is NULL");
    if (m < 1) return mmc_fail(MMC_ERR_ARG, "m = %d must be positive", m);
    if (dst->dim != m) return mmc_fail(MMC_ERR_ARG, "dst has width %d, the transform writes %d", dst->dim, m);
    if (dst->K != src->K) return mmc_fail(MMC_ERR_ARG, "dst has %d classes, src %d", dst->K, src->K);
    if (dst->device != src->device) return mmc_fail(MMC_ERR_ARG, "dst is on device %d, src on device %d", dst->device, src->device);
    if (flags & ~MMC_IN_HOST) return mmc_fail(MMC_ERR_ARG, "flags 0x%x: only MMC_IN_HOST is defined here", flags);
    if (n == 0) return MMC_OK;
    const int dim = src->dim;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(src->device));
    try {
        dst->y_host.reserve((size_t)(dst->n + n));
    } catch (const std::bad_alloc&) {
        return mmc_fail(MMC_ERR_NOMEM, "no host memory for %lld labels", (long long)(dst->n + n));
    }
    DevBuf<char> mem;   // a per-call device allocation, freed on every way out
    const float *d_centre = centre, *d_T = T;
    if (flags & MMC_IN_HOST) {
        const size_t o_T = align256((size_t)dim * 4), total = o_T + align256((size_t)m * dim * 4);
        if (!mem.alloc((int64_t)total)) return mmc_fail(MMC_ERR_NOMEM, "hipMalloc of %zu bytes for the transform's matrix failed", total);
        HIP_TRY(hipMemcpyAsync(mem.p, centre, (size_t)dim * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(mem.p + o_T, T, (size_t)m * dim * 4, hipMemcpyHostToDevice, st));
        d_centre = (const float*)mem.p;
        d_T = (const float*)(mem.p + o_T);
    }
    const int r = featureset_reserve(dst, dst->n + n, st);
    if (r) return r;
    const dim3 grid((unsigned)((n + 63) / 64), (unsigned)((m + 63) / 64));
    transform_kernel<<<grid, 256, 0, st>>>(src->X + (size_t)first * dim, d_centre, d_T, dst->X + (size_t)dst->n * m, n, dim, m);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(dst->y + dst->n, src->y + first, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    dst->y_host.insert(dst->y_host.end(), src->y_host.begin() + first, src->y_host.begin() + first + n);   // the row count moves last
    dst->n += n;
    return MMC_OK;
}
