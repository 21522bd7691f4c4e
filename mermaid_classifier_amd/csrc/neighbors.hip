// neighbors.hip -- exact-f32 nearest neighbours between resident feature sets (gfx950): mmc_featureset_knn.
// No reference counterpart: include/mmc.h "nearest neighbours" is the definition.
//
// The nq x nb score matrix is never written.  knn_tile_kernel computes it 128 x 128 at a time on v_mfma_f32_16x16x4_f32 (the tile of
// scatter_kernel in features.hip: 16 k-values per stage, wave w owns the 64 x 64 quadrant (w>>1, w&1) as 4 x 4 fragments), applies
// the metric and the eligibility mask, and folds every tile into a per-query list of the k best 64-bit keys that lives in LDS.  A
// workgroup owns one query tile and one contiguous range of base tiles (a split); the splits' lists meet in knn_merge_kernel, a second
// launch.  No flags, no spin waits, no float atomics.
//
// Determinism: a key is (order-preserving map of the score) << 32 | (0xFFFFFFFF - base row), so the keys of one query are distinct and
// totally ordered; the k largest of a set are then unique, whatever order the candidates arrive in.  Tiles, splits and chunks only
// change that order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mmc.h"
#include "trainer_internal.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

constexpr int kT = MMC_KNN_TILE_ROWS;   // tile edge, query rows and base rows
constexpr int kSK = 16;                 // k-values per stage
constexpr int kSLD = 144;               // LDS row stride in floats: features.hip's kSLD note (the k-rows of one fragment read, two per
                                        // 32-lane group, land on disjoint banks)
constexpr int kPC = 32;                 // base columns per fold phase: 16 of either column half
constexpr int kPLD = 132;               // the phase buffer's stride over queries: 16-byte rows, a 16-lane b128 store spreads over all banks
static_assert(2 * kSK * kSLD >= kPC * kPLD, "the phase buffer reuses the operand tiles");
static_assert(kT == 128, "the wave / fragment layout below is for 128 x 128 tiles");

// ---- the key ------------------------------------------------------------------------------------------------------------------
// The high word: 0 = no entry; 1 = NaN (below every number); otherwise the fp32 bit pattern, sign bit flipped for s >= 0 and all bits
// flipped for s < 0, which orders like the value (-inf -> 0x007FFFFF ... +inf -> 0xFF800000).  -0 is keyed, and returned, as +0.
__device__ __forceinline__ unsigned knn_score_word(float s)
{
    if (s != s) return 1u;
    const unsigned u = __float_as_uint(s + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float knn_word_score(unsigned w)
{
    if (w == 0u) return __uint_as_float(0xFF800000u);   // the tail fill
    if (w == 1u) return __uint_as_float(0x7FC00000u);
    return __uint_as_float((w & 0x80000000u) ? (w ^ 0x80000000u) : ~w);
}

__device__ __forceinline__ u64 knn_key(unsigned word, unsigned row) { return ((u64)word << 32) | (u64)(0xFFFFFFFFu - row); }

// List[j][q]: thread q's sorted list (descending, empty entries 0 at the tail).  key > List[k-1][q] on entry.
__device__ __forceinline__ u64 knn_insert(u64 (*List)[kT], int q, int k, u64 key)
{
    int j = k - 1;
    while (j > 0) {
        const u64 up = List[j - 1][q];
        if (up >= key) break;
        List[j][q] = up;
        --j;
    }
    List[j][q] = key;
    return List[k - 1][q];
}

// ---- norms ----------------------------------------------------------------------------------------------------------------------
// one thread per row, columns in ascending order, fp64: s = fl32(sum x^2), r = fl32(1 / sqrt(sum x^2)), 0 for a zero row
__global__ __launch_bounds__(256) void knn_norms_kernel(const float* __restrict__ X, int64_t n, int dim, float* __restrict__ s,
                                                        float* __restrict__ r)
{
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    const float* x = X + (size_t)row * dim;
    double acc = 0.0;
    for (int j = 0; j < dim; ++j) {
        const double v = (double)x[j];
        acc = fma(v, v, acc);
    }
    s[row] = (float)acc;
    r[row] = acc > 0.0 ? (float)(1.0 / sqrt(acc)) : 0.f;
}

// ---- tiles ----------------------------------------------------------------------------------------------------------------------
struct KnnArgs {
    const float* Q;          // the chunk's first query row
    const float* B;          // the base range's first row
    const float *q_s, *q_r;  // per query row of the chunk: sum of squares, reciprocal norm
    const float *b_s, *b_r;  // per base row of the range
    const int32_t* q_group;  // per query row of the chunk, or null
    const int32_t* b_group;  // per base row of the range, or null (both or neither)
    int64_t self_shift;      // EXCLUDE_SELF: base row j is query row i itself when i + self_shift == j; INT64_MIN: off
    int nq, nb, dim, k, metric, splits, base_tiles, q_cap;
    u64* partial;            // [split][k][q_cap]
};

template <bool VEC>
__device__ __forceinline__ f4 knn_load4(const float* __restrict__ X, int64_t row, int64_t n, int col, int dim)
{
    f4 v = (f4){0.f, 0.f, 0.f, 0.f};
    if (row >= n || col >= dim) return v;
    const float* p = X + (size_t)row * dim + col;
    if (VEC) {
        v = *reinterpret_cast<const f4*>(p);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (col + e < dim) v[e] = p[e];
    }
    return v;
}

template <bool VEC>
__global__ __launch_bounds__(256, 2) void knn_tile_kernel(const KnnArgs A)
{
    // As[k][m], Bs[k][m] with m ^= ((k >> 2) & 3) << 4: the staging stores of one 32-lane group then hit 32 banks; between the tiles'
    // products the same memory is the phase buffer P[column][query] of score words
    __shared__ __attribute__((aligned(16))) float smem[2 * kSK * kSLD];
    __shared__ u64 List[MMC_KNN_MAX_K][kT];
    __shared__ float q_s[kT], q_r[kT];
    __shared__ int32_t q_g[kT];
    float (*As)[kSLD] = reinterpret_cast<float (*)[kSLD]>(smem);
    float (*Bs)[kSLD] = reinterpret_cast<float (*)[kSLD]>(smem + kSK * kSLD);
    unsigned* P = reinterpret_cast<unsigned*>(smem);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int li = lane & 15, lq = lane >> 4;
    const int srow = (tid & 15) + 16 * (tid >> 6), sk = ((tid >> 4) & 3) * 4;   // staging: rows srow and srow + 64, k-values sk .. sk + 3
    const int64_t q0 = (int64_t)blockIdx.x * kT;
    const int split = blockIdx.y;
    const int t0 = (int)((int64_t)split * A.base_tiles / A.splits), t1 = (int)((int64_t)(split + 1) * A.base_tiles / A.splits);
    const int k = A.k, dim = A.dim, stages = (dim + kSK - 1) / kSK;
    const bool grouped = A.q_group != nullptr;

    if (tid < kT) {
        const int64_t qi = q0 + tid;
        const bool in = qi < A.nq;
        q_s[tid] = in ? A.q_s[qi] : 0.f;
        q_r[tid] = in ? A.q_r[qi] : 0.f;
        q_g[tid] = in && grouped ? A.q_group[qi] : 0;
        for (int j = 0; j < k; ++j) List[j][tid] = 0;
    }
    u64 thr = 0;   // thread q < 128: the k-th key of query q0 + q
    __syncthreads();

    for (int t = t0; t < t1; ++t) {
        const int64_t b0 = (int64_t)t * kT;
        f4 acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = (f4){0.f, 0.f, 0.f, 0.f};
        f4 ga[2], gb[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            ga[r] = knn_load4<VEC>(A.Q, q0 + srow + 64 * r, A.nq, sk, dim);
            gb[r] = knn_load4<VEC>(A.B, b0 + srow + 64 * r, A.nb, sk, dim);
        }
        for (int st = 0; st < stages; ++st) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int m = (srow + 64 * r) ^ ((sk >> 2) << 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    As[sk + e][m] = ga[r][e];
                    Bs[sk + e][m] = gb[r][e];
                }
            }
            __syncthreads();
            if (st + 1 < stages) {   // the next stage's loads fly during this stage's MFMAs
                const int col = (st + 1) * kSK + sk;
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    ga[r] = knn_load4<VEC>(A.Q, q0 + srow + 64 * r, A.nq, col, dim);
                    gb[r] = knn_load4<VEC>(A.B, b0 + srow + 64 * r, A.nb, col, dim);
                }
            }
#pragma unroll
            for (int kk = 0; kk < kSK; kk += 4) {
                const int sw = (kk >> 2) << 4;
                float av[4], bv[4];
#pragma unroll
                for (int f = 0; f < 4; ++f) {
                    av[f] = As[kk + lq][(wm + f * 16 + li) ^ sw];
                    bv[f] = Bs[kk + lq][(wn + f * 16 + li) ^ sw];
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bv[b], acc[a][b], 0, 0, 0);
            }
            __syncthreads();
        }
        // lane (li, lq) holds d of query wm + 16a + 4 lq + r and base column wn + 16b + li.  Phase b: every wave writes the score words
        // of its fragments (., b) -- 32 columns of the tile --, then thread q folds those 32 into query q's list.
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t j = b0 + wn + 16 * b + li;   // relative to the base range
            const bool j_in = j < A.nb;
            const float bs = j_in ? A.b_s[j] : 0.f, br = j_in ? A.b_r[j] : 0.f;
            const int32_t bg = j_in && grouped ? A.b_group[j] : 0;
            const int pc = (wn >> 2) + li;            // 0..15 for the left column half, 16..31 for the right
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                unsigned w[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int q = wm + 16 * a + 4 * lq + r;
                    const float d = acc[a][b][r];
                    float s;
                    if (A.metric == MMC_KNN_COSINE) s = (d * q_r[q]) * br;
                    else if (A.metric == MMC_KNN_L2) s = -fmaf(-2.f, d, q_s[q] + bs);
                    else s = d;
                    const int64_t qi = q0 + q;
                    bool ok = j_in && qi < A.nq;
                    if (grouped && q_g[q] == bg) ok = false;
                    if (qi + A.self_shift == j) ok = false;
                    w[r] = ok ? knn_score_word(s) : 0u;
                }
                *reinterpret_cast<uint4*>(&P[pc * kPLD + wm + 16 * a + 4 * lq]) = make_uint4(w[0], w[1], w[2], w[3]);
            }
            __syncthreads();
            if (tid < kT) {
                const unsigned thr_word = (unsigned)(thr >> 32);
                for (int c = 0; c < kPC; ++c) {
                    const unsigned word = P[c * kPLD + tid];
                    if (word < thr_word || word == 0u) continue;   // the one compare; 0: not eligible
                    const u64 key = knn_key(word, (unsigned)(b0 + (c >> 4) * 64 + 16 * b + (c & 15)));
                    if (key > thr) thr = knn_insert(List, tid, k, key);
                }
            }
            __syncthreads();
        }
    }
    if (tid < kT)
        for (int j = 0; j < k; ++j) A.partial[((size_t)split * k + j) * A.q_cap + q0 + tid] = List[j][tid];
}

// ---- merge ------------------------------------------------------------------------------------------------------------------------
// one thread per query of the chunk: the splits' sorted lists into one, then index / score / label.  splits = 0: the tail fill only.
__global__ __launch_bounds__(kT) void knn_merge_kernel(const u64* __restrict__ partial, int splits, int k, int q_cap, int nq,
                                                       const int32_t* __restrict__ base_y, int32_t* __restrict__ index,
                                                       float* __restrict__ score, int32_t* __restrict__ label)
{
    __shared__ u64 List[MMC_KNN_MAX_K][kT];
    const int tid = threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x * kT + tid;
    if (q >= nq) return;
    for (int j = 0; j < k; ++j) List[j][tid] = 0;
    u64 thr = 0;
    for (int s = 0; s < splits; ++s)
        for (int j = 0; j < k; ++j) {
            const u64 key = partial[((size_t)s * k + j) * q_cap + q];
            if (key <= thr) break;   // a split's list is sorted: nothing further down can enter.  An empty entry is 0.
            thr = knn_insert(List, tid, k, key);
        }
    for (int j = 0; j < k; ++j) {
        const u64 key = List[j][tid];
        const unsigned word = (unsigned)(key >> 32);
        const int32_t row = word ? (int32_t)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFu)) : -1;
        index[(size_t)q * k + j] = row;
        score[(size_t)q * k + j] = knn_word_score(word);
        if (label) label[(size_t)q * k + j] = word ? base_y[row] : -1;
    }
}

int check_range(const mmc_featureset* fs, int64_t first, int64_t n, const char* what)
{
    if (!fs) return mmc_fail(MMC_ERR_ARG, "%s feature set handle is NULL", what);
    if (first < 0 || n < 0 || first > fs->n || n > fs->n - first)
        return mmc_fail(MMC_ERR_ARG, "%s rows [%lld, %lld + %lld) outside the set's %lld rows", what, (long long)first, (long long)first,
                        (long long)n, (long long)fs->n);
    if (n > 0x7fffffff) return mmc_fail(MMC_ERR_ARG, "%s n = %lld: at most 2^31 - 1 rows per call", what, (long long)n);
    return MMC_OK;
}

}   // namespace

// the number of contiguous base-tile ranges one chunk's query tiles are crossed with: include/mmc.h gives the rule
static int knn_splits(int64_t nq, int64_t nb)
{
    const int64_t chunk = nq < MMC_KNN_CHUNK_ROWS ? nq : MMC_KNN_CHUNK_ROWS;
    const int64_t query_tiles = (chunk + kT - 1) / kT, base_tiles = (nb + kT - 1) / kT;
    int64_t s = query_tiles ? 1024 / query_tiles : 1;
    if (s < 1) s = 1;
    if (s > base_tiles) s = base_tiles;
    if (s > MMC_KNN_MAX_SPLITS) s = MMC_KNN_MAX_SPLITS;
    return s < 1 ? 1 : (int)s;
}

extern "C" int mmc_featureset_knn(mmc_featureset* query, int64_t q_first, int64_t nq, mmc_featureset* base, int64_t b_first, int64_t nb,
                                  int k, int metric, const int32_t* q_group, const int32_t* b_group, int32_t* index, float* score,
                                  int32_t* label, unsigned flags, void* hip_stream)
{
    int rc = check_range(query, q_first, nq, "query");
    if (!rc) rc = check_range(base, b_first, nb, "base");
    if (rc) return rc;
    if (!index || !score) return mmc_fail(MMC_ERR_ARG, "index / score is NULL");
    if (k < 1 || k > MMC_KNN_MAX_K) return mmc_fail(MMC_ERR_ARG, "k = %d outside [1, MMC_KNN_MAX_K = %d]", k, MMC_KNN_MAX_K);
    if (metric != MMC_KNN_DOT && metric != MMC_KNN_COSINE && metric != MMC_KNN_L2)
        return mmc_fail(MMC_ERR_ARG, "metric = %d: MMC_KNN_DOT, MMC_KNN_COSINE or MMC_KNN_L2", metric);
    if (flags & ~(MMC_IN_HOST | MMC_OUT_HOST | MMC_KNN_EXCLUDE_SELF))
        return mmc_fail(MMC_ERR_ARG, "flags 0x%x: only MMC_IN_HOST, MMC_OUT_HOST and MMC_KNN_EXCLUDE_SELF are defined here", flags);
    if ((flags & MMC_KNN_EXCLUDE_SELF) && query != base)
        return mmc_fail(MMC_ERR_ARG, "MMC_KNN_EXCLUDE_SELF needs query and base to be the same set");
    if ((q_group == nullptr) != (b_group == nullptr)) return mmc_fail(MMC_ERR_ARG, "q_group and b_group: both, or neither");
    if (query->dim != base->dim) return mmc_fail(MMC_ERR_ARG, "query has width %d, base %d", query->dim, base->dim);
    if (query->device != base->device) return mmc_fail(MMC_ERR_ARG, "query is on device %d, base on device %d", query->device, base->device);
    if (nq == 0) return MMC_OK;

    const bool in_host = flags & MMC_IN_HOST, out_host = flags & MMC_OUT_HOST, grouped = q_group != nullptr;
    const int dim = query->dim;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(query->device));

    const int splits = nb ? knn_splits(nq, nb) : 0;
    const int base_tiles = (int)((nb + kT - 1) / kT);
    const int64_t chunk = nq < MMC_KNN_CHUNK_ROWS ? nq : MMC_KNN_CHUNK_ROWS;
    const int q_cap = (int)((chunk + kT - 1) / kT) * kT;   // whole tiles: a ragged tile's rows write (empty) lists too
    const size_t o_bs = 0, o_br = o_bs + align256((size_t)nb * 4), o_bg = o_br + align256((size_t)nb * 4),
                 o_qs = o_bg + align256(grouped && in_host ? (size_t)nb * 4 : 0), o_qr = o_qs + align256((size_t)q_cap * 4),
                 o_qg = o_qr + align256((size_t)q_cap * 4), o_partial = o_qg + align256(grouped && in_host ? (size_t)q_cap * 4 : 0),
                 o_idx = o_partial + align256((size_t)splits * k * q_cap * 8), o_score = o_idx + align256(out_host ? (size_t)chunk * k * 4 : 0),
                 o_label = o_score + align256(out_host ? (size_t)chunk * k * 4 : 0),
                 total = o_label + align256(out_host && label ? (size_t)chunk * k * 4 : 0);
    DevBuf<char> mem;   // a per-call device allocation, freed on every way out
    if (!mem.alloc((int64_t)total)) return mmc_fail(MMC_ERR_NOMEM, "hipMalloc of %zu bytes of nearest-neighbour scratch failed", total);
    float *d_bs = (float*)(mem.p + o_bs), *d_br = (float*)(mem.p + o_br), *d_qs = (float*)(mem.p + o_qs), *d_qr = (float*)(mem.p + o_qr);
    const float* Bx = base->X + (size_t)b_first * dim;
    const int32_t* d_bg = b_group;
    if (nb) {
        if (grouped && in_host) {
            HIP_TRY(hipMemcpyAsync(mem.p + o_bg, b_group, (size_t)nb * 4, hipMemcpyHostToDevice, st));
            d_bg = (const int32_t*)(mem.p + o_bg);
        }
        knn_norms_kernel<<<(unsigned)((nb + 255) / 256), 256, 0, st>>>(Bx, nb, dim, d_bs, d_br);
    }
    const int64_t self_shift = (flags & MMC_KNN_EXCLUDE_SELF) ? q_first - b_first : INT64_MIN;

    for (int64_t c0 = 0; c0 < nq; c0 += chunk) {
        const int64_t cn = nq - c0 < chunk ? nq - c0 : chunk;
        const float* Qx = query->X + (size_t)(q_first + c0) * dim;
        int32_t* d_index = out_host ? (int32_t*)(mem.p + o_idx) : index + (size_t)c0 * k;
        float* d_score = out_host ? (float*)(mem.p + o_score) : score + (size_t)c0 * k;
        int32_t* d_label = !label ? nullptr : out_host ? (int32_t*)(mem.p + o_label) : label + (size_t)c0 * k;
        if (nb) {
            const int32_t* d_qg = grouped ? q_group + c0 : nullptr;
            if (grouped && in_host) {
                HIP_TRY(hipMemcpyAsync(mem.p + o_qg, q_group + c0, (size_t)cn * 4, hipMemcpyHostToDevice, st));
                d_qg = (const int32_t*)(mem.p + o_qg);
            }
            knn_norms_kernel<<<(unsigned)((cn + 255) / 256), 256, 0, st>>>(Qx, cn, dim, d_qs, d_qr);
            KnnArgs a;
            a.Q = Qx;
            a.B = Bx;
            a.q_s = d_qs;
            a.q_r = d_qr;
            a.b_s = d_bs;
            a.b_r = d_br;
            a.q_group = d_qg;
            a.b_group = grouped ? d_bg : nullptr;
            a.self_shift = self_shift == INT64_MIN ? INT64_MIN : self_shift + c0;
            a.nq = (int)cn;
            a.nb = (int)nb;
            a.dim = dim;
            a.k = k;
            a.metric = metric;
            a.splits = splits;
            a.base_tiles = base_tiles;
            a.q_cap = q_cap;
            a.partial = (u64*)(mem.p + o_partial);
            const dim3 grid((unsigned)((cn + kT - 1) / kT), (unsigned)splits);
            const bool vec = dim % 4 == 0 && (uintptr_t)Qx % 16 == 0 && (uintptr_t)Bx % 16 == 0;
            if (vec) knn_tile_kernel<true><<<grid, 256, 0, st>>>(a);
            else knn_tile_kernel<false><<<grid, 256, 0, st>>>(a);
        }
        knn_merge_kernel<<<(unsigned)((cn + kT - 1) / kT), kT, 0, st>>>((const u64*)(mem.p + o_partial), splits, k, q_cap, (int)cn,
                                                                        base->y + b_first, d_index, d_score, d_label);
        HIP_TRY(hipGetLastError());
        if (out_host) {
            HIP_TRY(hipMemcpyAsync(index + (size_t)c0 * k, d_index, (size_t)cn * k * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(score + (size_t)c0 * k, d_score, (size_t)cn * k * 4, hipMemcpyDeviceToHost, st));
            if (label) HIP_TRY(hipMemcpyAsync(label + (size_t)c0 * k, d_label, (size_t)cn * k * 4, hipMemcpyDeviceToHost, st));
        }
    }
    HIP_TRY(hipStreamSynchronize(st));   // the scratch is freed on return
    return MMC_OK;
}
