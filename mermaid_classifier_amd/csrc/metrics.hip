// metrics.hip -- grouped validation on the device (gfx950): the whole-split passes behind mmc_head_evaluate_grouped(_set).
//
// Replaces the host loops of the reference's MetricsCoordinator.compute_and_log_all (mermaid_classifier/pyspacer/metrics/):
//   cover.py:44-72          per-image class counts, then per-class sums over images            group_rows_kernel, cover_*_kernel
//   per_source.py:88-140    one confusion table per data source                                group_rows_kernel
//   probability.py:43-60    per-true-class sums of the loss (and, calibration.py:139-140,      group_rows_kernel
//                           of the confidence)
//   calibration.py:32-79    _adaptive_ece: equal-mass bins over the sorted confidences         select_*_kernel, bin_sums_kernel
//
// group_rows_kernel runs once per 65 536-row chunk, behind calibrate_eval_kernel, on that kernel's per-row outputs (scored class,
// est, score, p_true).  One thread per row: the row's image by binary search in the offsets, then integer atomics only --
// true_cnt / pred_cnt [image][class] and points [image] (int32), source_confusion [source][g][est] (int64), and the three per-class
// sums support / nll_q32 / score_q32, kept in LDS per workgroup (K <= GROUP_CLS_LDS_MAX_K) and flushed with one atomic per touched
// entry.  It also stores the row's 31-bit reliability key (bits(score) << 1) | (est == g), GROUP_KEY_NONE for a row that is not
// scored.  Every table is an integer, so nothing depends on the order of rows, chunks or workgroups.
//
// Cover.  t = true_cnt / points and p = pred_cnt / points in fp64 over the images with points > 0.  cover_pass1_kernel: grid (image
// chunk, 64 classes), lane = class, so that the [image][class] tables are read along the class dimension; each lane walks its chunk's
// images in order and writes one slab entry of 8 doubles.  cover_reduce1_kernel adds the chunks in order per class.  The second pass
// (cover_pass2 / cover_reduce2) re-reads the resident tables for sum (t - mean t)^2.  No float atomics: the chunking depends on
// n_images alone, so two runs give the same bits.
//
// Reliability bins without a sort.  The sorted position b * n_scored / n_bins of every bin's first and last key is a target (at most
// 128).  Three levels of radix select over key digits of 11 / 10 / 10 bits: select_hist_kernel counts, per distinct prefix among the
// targets (a "slot"), the next digit of every key with that prefix; select_scan_kernel (one workgroup) walks each target's histogram
// to its digit and residual rank and rebuilds the slot list.  Calibrated scores pile up near 1.0, so a few counters are hot: a
// workgroup keeps the table in LDS when slots x digits <= GROUP_LDS_HIST (always at level 1) and flushes one atomic per touched
// counter; a wider table is counted in memory with one atomic per wave and distinct counter (the wave's equal bins are found by
// ballot).  After level 3 the slots are the distinct edge keys e_0 < e_1 < ...; bin_sums_kernel counts, in LDS, the rows equal to
// each e_j and count / n_correct / conf_q32 of the rows strictly between e_j and e_j+1.  Such a region lies inside one bin, and rows
// with equal keys contribute identically, so the host splits the equal-key groups between bins by position arithmetic on integers.
//
// Per-category bins (mmc_head_evaluate_categories; calibration.py:120-161, one _adaptive_ece per top-level category over the rows whose
// true class lies in it, n_bins = min(20, max(2, n // 10)) at :137).  group_rows_kernel also stores one category byte per row;
// category_counts_kernel sums support over each category's classes for its rows and bins; then, per category, category_mask_kernel
// copies the keys of its rows into a second key buffer (GROUP_KEY_NONE elsewhere), select_init_category_kernel seeds the targets
// from the category's own counts, and the select and bin_sums kernels above run unchanged on that buffer into the category's own
// GroupSelect / raw slot.  9 kernels and 4 memsets per category; five of the kernels read 4 or 5 B per row of the call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace {

constexpr int GROUP_CLS_LDS_MAX_K = 1024;    // 3 x K x 8 B of per-class sums in LDS
constexpr int GROUP_LDS_HIST = 8192;         // counters of a select level kept in LDS (32 KB)
constexpr int GROUP_COVER_CHUNKS = 1024;     // at most this many image chunks


template <bool CLS_IN_LDS>
__global__ __launch_bounds__(256) void group_rows_kernel(GroupRowsArgs a)
{
    extern __shared__ unsigned long long cls_lds[];   // CLS_IN_LDS: [3][K]
    const int K = a.K;
    if (CLS_IN_LDS) {
        for (int i = threadIdx.x; i < 3 * K; i += 256) cls_lds[i] = 0;
        __syncthreads();
    }
    unsigned long long* cls = CLS_IN_LDS ? cls_lds : a.cls_tab;
    for (int r = blockIdx.x * 256 + threadIdx.x; r < a.rows; r += gridDim.x * 256) {
        const int g = a.scored[r];
        const int64_t row = a.row0 + r;
        uint32_t key = GROUP_KEY_NONE;
        if (g >= 0) {
            const int est = a.est[r];
            const float sc = a.score[r];
            const float pt = a.p_true[r];
            int lo = 0, hi = (int)a.n_images;   // offsets[lo] <= row < offsets[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (a.offsets[mid] <= row) lo = mid;
                else hi = mid;
            }
            atomicAdd(&a.true_cnt[(size_t)lo * K + g], 1);
            atomicAdd(&a.pred_cnt[(size_t)lo * K + est], 1);
            atomicAdd(&a.points[lo], 1);
            if (a.source_of_image) atomicAdd(&a.source_conf[((size_t)a.source_of_image[lo] * K + g) * K + est], 1ull);
            atomicAdd(&cls[g], 1ull);
            atomicAdd(&cls[K + g], (unsigned long long)llrint(-log(fmin(fmax((double)pt, 1e-15), 1.0)) * 4294967296.0));
            atomicAdd(&cls[2 * K + g], (unsigned long long)llrint((double)sc * 4294967296.0));
            uint32_t bits = __float_as_uint(sc);
            if (bits > 0x3F800000u) bits = 0x3F800000u;   // (a scored row's score is finite and in [0, 1]: the key stays below 2^31)
            key = (bits << 1) | (uint32_t)(est == g);
        }
        a.keys[row] = key;
        if (a.seg) {
            const int c = g >= 0 ? a.category_of_class[g] : -1;
            a.seg[row] = c >= 0 ? (uint8_t)c : GROUP_SEG_NONE;
        }
    }
    if (CLS_IN_LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < 3 * K; i += 256)
            if (cls_lds[i]) atomicAdd(&a.cls_tab[i], cls_lds[i]);
    }
}

// ---- cover --------------------------------------------------------------------------------------------------------------
// slab[(chunk * K + c) * 8 + j], j = sum t, sum p, sum (p - t), sum (p - t)^2, sum |p - t|, min t, max t, images with points
__global__ __launch_bounds__(64) void cover_pass1_kernel(const int32_t* __restrict__ true_cnt, const int32_t* __restrict__ pred_cnt,
                                                         const int32_t* __restrict__ points, int64_t n_images, int K, int64_t per_chunk,
                                                         double* __restrict__ slab)
{
    const int c = blockIdx.y * 64 + threadIdx.x;
    if (c >= K) return;
    const int64_t i0 = (int64_t)blockIdx.x * per_chunk, i1 = i0 + per_chunk < n_images ? i0 + per_chunk : n_images;
    double st = 0, sp = 0, sd = 0, sdd = 0, sad = 0, mn = INFINITY, mx = -INFINITY, used = 0;
    for (int64_t i = i0; i < i1; ++i) {
        const int pts = points[i];
        if (pts <= 0) continue;
        const double t = (double)true_cnt[(size_t)i * K + c] / (double)pts;
        const double p = (double)pred_cnt[(size_t)i * K + c] / (double)pts;
        const double d = p - t;
        st += t; sp += p; sd += d; sdd += d * d; sad += fabs(d);
        mn = fmin(mn, t); mx = fmax(mx, t);
        used += 1.0;
    }
    double* o = slab + ((size_t)blockIdx.x * K + c) * 8;
    o[0] = st; o[1] = sp; o[2] = sd; o[3] = sdd; o[4] = sad; o[5] = mn; o[6] = mx; o[7] = used;
}

// cov[c * 8 + j] = the chunks of slab in order (j < 5 sums, 5 min, 6 max; 7 is written by the second pass); *n_used = images with points
__global__ __launch_bounds__(256) void cover_reduce1_kernel(const double* __restrict__ slab, int chunks, int K, double* __restrict__ cov,
                                                            long long* __restrict__ n_used)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= K) return;
    double s[5] = {0, 0, 0, 0, 0}, mn = INFINITY, mx = -INFINITY, used = 0;
    for (int g = 0; g < chunks; ++g) {
        const double* p = slab + ((size_t)g * K + c) * 8;
#pragma unroll
        for (int j = 0; j < 5; ++j) s[j] += p[j];
        mn = fmin(mn, p[5]); mx = fmax(mx, p[6]);
        used += p[7];
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) cov[(size_t)c * 8 + j] = s[j];
    cov[(size_t)c * 8 + 5] = used > 0 ? mn : 0.0;
    cov[(size_t)c * 8 + 6] = used > 0 ? mx : 0.0;
    cov[(size_t)c * 8 + 7] = 0.0;
    if (c == 0) *n_used = (long long)used;
}

__global__ __launch_bounds__(64) void cover_pass2_kernel(const int32_t* __restrict__ true_cnt, const int32_t* __restrict__ points,
                                                         int64_t n_images, int K, int64_t per_chunk, const double* __restrict__ cov,
                                                         const long long* __restrict__ n_used, double* __restrict__ slab)
{
    const int c = blockIdx.y * 64 + threadIdx.x;
    if (c >= K) return;
    const int64_t i0 = (int64_t)blockIdx.x * per_chunk, i1 = i0 + per_chunk < n_images ? i0 + per_chunk : n_images;
    const long long nu = *n_used;
    const double tbar = nu > 0 ? cov[(size_t)c * 8] / (double)nu : 0.0;
    double ss = 0;
    for (int64_t i = i0; i < i1; ++i) {
        const int pts = points[i];
        if (pts <= 0) continue;
        const double d = (double)true_cnt[(size_t)i * K + c] / (double)pts - tbar;
        ss += d * d;
    }
    slab[(size_t)blockIdx.x * K + c] = ss;
}

__global__ __launch_bounds__(256) void cover_reduce2_kernel(const double* __restrict__ slab, int chunks, int K, double* __restrict__ cov)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= K) return;
    double s = 0;
    for (int g = 0; g < chunks; ++g) s += slab[(size_t)g * K + c];
    cov[(size_t)c * 8 + 7] = s;
}

// ---- reliability bins: radix select of the keys at the bin edges ---------------------------------------------------------
// target 2 b / 2 b + 1 = the sorted position of bin b's first / last key (an empty bin: both its first position, which always
// exists); positions never decrease with the target index, so neither do the prefixes
__device__ void select_seed(long long ns, int n_bins, GroupSelect* sel)
{
    const int t = threadIdx.x;
    if (ns > 0 && t < 2 * n_bins) {
        const long long b = t >> 1;
        const long long lo = b * ns / n_bins, hi = (b + 1) * ns / n_bins;
        sel->tgt_prefix[t] = 0;
        sel->tgt_rank[t] = (uint32_t)(((t & 1) && hi > lo) ? hi - 1 : lo);
        sel->tgt_slot[t] = 0;
    }
    if (t == 0) {
        sel->n_scored = (uint32_t)(ns > 0 ? ns : 0);
        sel->n_targets = ns > 0 ? 2u * n_bins : 0u;
        sel->n_slots = ns > 0 ? 1u : 0u;
        sel->slot_prefix[0] = 0;
    }
}

__global__ __launch_bounds__(GROUP_MAX_TARGETS) void select_init_kernel(const long long* __restrict__ totals, int n_bins, GroupSelect* sel)
{
    select_seed(totals[0] - totals[2] - totals[3], n_bins, sel);
}

// the targets of one category: its rows and its bins as category_counts_kernel left them
__global__ __launch_bounds__(GROUP_MAX_TARGETS) void select_init_category_kernel(const long long* __restrict__ cat_rows,
                                                                                 const int32_t* __restrict__ cat_bins, int c, GroupSelect* sel)
{
    select_seed(cat_rows[c], cat_bins[c], sel);
}

// ---- per-category reliability bins ----------------------------------------------------------------------------------------
// lane = category: the rows of its classes, and from them its bins
__global__ __launch_bounds__(GROUP_MAX_CATEGORIES) void category_counts_kernel(const unsigned long long* __restrict__ support,
                                                                               const int32_t* __restrict__ category_of_class, int K,
                                                                               int n_categories, long long* __restrict__ cat_rows,
                                                                               int32_t* __restrict__ cat_bins)
{
    const int c = threadIdx.x;
    if (c >= n_categories) return;
    long long n = 0;
    for (int k = 0; k < K; ++k)
        if (category_of_class[k] == c) n += (long long)support[k];
    long long nb = n / GROUP_CAT_ROWS_PER_BIN;
    nb = nb < GROUP_CAT_BINS_MIN ? GROUP_CAT_BINS_MIN : nb;
    nb = nb > GROUP_CAT_BINS_MAX ? GROUP_CAT_BINS_MAX : nb;
    cat_rows[c] = n;
    cat_bins[c] = n > 0 ? (int32_t)nb : 0;
}

// the keys of category c's rows, GROUP_KEY_NONE elsewhere: the select kernels then see that category alone
__global__ __launch_bounds__(256) void category_mask_kernel(const uint32_t* __restrict__ keys, const uint8_t* __restrict__ seg, int64_t n, int c,
                                                            uint32_t* __restrict__ ckeys)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        ckeys[i] = seg[i] == (uint8_t)c ? keys[i] : GROUP_KEY_NONE;
}

// hist[(slot << bits) | digit] += 1 for every key whose bits above (shift + bits) are a slot's prefix; digit = (key >> shift) % 2^bits
__global__ __launch_bounds__(256) void select_hist_kernel(const uint32_t* __restrict__ keys, int64_t n, int shift, int bits,
                                                          const GroupSelect* __restrict__ sel, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t sp[GROUP_MAX_TARGETS];
    __shared__ uint32_t lh[GROUP_LDS_HIST];
    const int ns = (int)sel->n_slots;
    if (ns == 0) return;
    const int lane = threadIdx.x & 63;
    const int cells = ns << bits;
    const bool in_lds = cells <= GROUP_LDS_HIST;
    if ((int)threadIdx.x < ns) sp[threadIdx.x] = sel->slot_prefix[threadIdx.x];
    if (in_lds)
        for (int i = threadIdx.x; i < cells; i += 256) lh[i] = 0;
    __syncthreads();
    for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {   // (uniform over the workgroup)
        const int64_t i = base + threadIdx.x;
        bool valid = false;
        uint32_t bin = 0;
        if (i < n) {
            const uint32_t key = keys[i];
            if (key != GROUP_KEY_NONE) {
                const uint32_t p = key >> (shift + bits);   // level 1: shift + bits = 31 and every key is below 2^31, p = 0
                int lo = 0, hi = ns;                        // the first slot whose prefix is >= p
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (sp[mid] < p) lo = mid + 1;
                    else hi = mid;
                }
                if (lo < ns && sp[lo] == p) {
                    valid = true;
                    bin = ((uint32_t)lo << bits) | ((key >> shift) & ((1u << bits) - 1u));
                }
            }
        }
        if (in_lds) {
            if (valid) atomicAdd(&lh[bin], 1u);
        } else {
            unsigned long long todo = __ballot(valid);
            while (todo) {   // one atomic per distinct bin of the wave
                const int leader = __ffsll((long long)todo) - 1;
                const uint32_t lb = __shfl(bin, leader);
                const unsigned long long same = __ballot(valid && bin == lb) & todo;
                if (lane == leader) atomicAdd(&hist[lb], (uint32_t)__popcll(same));
                todo &= ~same;
            }
        }
    }
    if (in_lds) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += 256)
            if (lh[i]) atomicAdd(&hist[i], lh[i]);
    }
}

// one workgroup: every target walks its slot's histogram to the digit that holds its rank; then the distinct prefixes, in order,
// become the next level's slots
__global__ __launch_bounds__(GROUP_MAX_TARGETS) void select_scan_kernel(int bits, GroupSelect* sel, const uint32_t* __restrict__ hist)
{
    const int nt = (int)sel->n_targets, t = threadIdx.x;
    if (t < nt) {
        const uint32_t* h = hist + ((size_t)sel->tgt_slot[t] << bits);
        uint32_t r = sel->tgt_rank[t];
        const int nd = 1 << bits;
        int d = 0;
        for (; d < nd - 1; ++d) {
            const uint32_t c = h[d];
            if (r < c) break;
            r -= c;
        }
        sel->tgt_prefix[t] = (sel->tgt_prefix[t] << bits) | (uint32_t)d;
        sel->tgt_rank[t] = r;
    }
    __syncthreads();
    if (t == 0 && nt > 0) {
        uint32_t ns = 0;
        for (int j = 0; j < nt; ++j) {
            const uint32_t p = sel->tgt_prefix[j];
            if (ns == 0 || sel->slot_prefix[ns - 1] != p) sel->slot_prefix[ns++] = p;
            sel->tgt_slot[j] = ns - 1;
        }
        sel->n_slots = ns;
    }
}

// with e_j = sel->slot_prefix[j] (the distinct edge keys, ascending; e_0 is the smallest key):
// raw[0][j] = #(key == e_j);   raw[1..3][j] = count, n_correct, sum llrint(score * 2^32) over e_j < key < e_j+1
__global__ __launch_bounds__(256) void bin_sums_kernel(const uint32_t* __restrict__ keys, int64_t n, const GroupSelect* __restrict__ sel,
                                                       unsigned long long* __restrict__ raw)
{
    __shared__ uint32_t ek[GROUP_MAX_TARGETS];
    __shared__ unsigned long long acc[4][GROUP_MAX_TARGETS];
    const int ne = (int)sel->n_slots;
    if (ne == 0) return;
    if (threadIdx.x < GROUP_MAX_TARGETS) {
        ek[threadIdx.x] = (int)threadIdx.x < ne ? sel->slot_prefix[threadIdx.x] : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j][threadIdx.x] = 0;
    }
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint32_t key = keys[i];
        if (key == GROUP_KEY_NONE) continue;
        int lo = 0, hi = ne;   // ek[lo] <= key < ek[hi] (ek[0] is the smallest key of all)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (ek[mid] <= key) lo = mid;
            else hi = mid;
        }
        if (ek[lo] == key) atomicAdd(&acc[0][lo], 1ull);
        else {
            atomicAdd(&acc[1][lo], 1ull);
            if (key & 1u) atomicAdd(&acc[2][lo], 1ull);
            atomicAdd(&acc[3][lo], (unsigned long long)llrint((double)__uint_as_float(key >> 1) * 4294967296.0));
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < ne)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (acc[j][threadIdx.x]) atomicAdd(&raw[(size_t)j * GROUP_MAX_TARGETS + threadIdx.x], acc[j][threadIdx.x]);
}

int pass_grid(int64_t n)
{
    const int64_t nb = (n + 255) / 256;
    return (int)(nb < 1024 ? (nb < 1 ? 1 : nb) : 1024);
}

}  // namespace

int launch_group_rows(const GroupRowsArgs& a, hipStream_t st)
{
    if (a.rows < 1 || a.K < 1 || a.n_images < 1 || !a.scored || !a.est || !a.score || !a.p_true || !a.offsets || !a.true_cnt || !a.pred_cnt ||
        !a.points || !a.cls_tab || !a.keys || (a.source_of_image && !a.source_conf) || (a.seg && !a.category_of_class))
        return -19;
    const int grid = (a.rows + 1023) / 1024;   // a workgroup walks about 1024 rows before it flushes its per-class sums
    if (a.K <= GROUP_CLS_LDS_MAX_K) hipLaunchKernelGGL((group_rows_kernel<true>), dim3(grid), dim3(256), (size_t)3 * a.K * 8, st, a);
    else hipLaunchKernelGGL((group_rows_kernel<false>), dim3(grid), dim3(256), 0, st, a);
    LAUNCH_CHECK();
    return 0;
}

void group_cover_chunks(int64_t n_images, int64_t* per_chunk, int* chunks)
{
    int64_t pc = (n_images + GROUP_COVER_CHUNKS - 1) / GROUP_COVER_CHUNKS;
    pc = pc < 64 ? 64 : pc;
    *per_chunk = pc;
    *chunks = (int)((n_images + pc - 1) / pc);
}

int launch_group_cover(const int32_t* true_cnt, const int32_t* pred_cnt, const int32_t* points, int64_t n_images, int K, double* slab,
                       double* cov, long long* n_used, hipStream_t st)
{
    if (n_images < 1 || K < 1 || !true_cnt || !pred_cnt || !points || !slab || !cov || !n_used) return -19;
    int64_t pc;
    int chunks;
    group_cover_chunks(n_images, &pc, &chunks);
    const dim3 grid(chunks, (K + 63) / 64);
    hipLaunchKernelGGL(cover_pass1_kernel, grid, dim3(64), 0, st, true_cnt, pred_cnt, points, n_images, K, pc, slab);
    hipLaunchKernelGGL(cover_reduce1_kernel, dim3((K + 255) / 256), dim3(256), 0, st, slab, chunks, K, cov, n_used);
    hipLaunchKernelGGL(cover_pass2_kernel, grid, dim3(64), 0, st, true_cnt, points, n_images, K, pc, cov, n_used, slab);
    hipLaunchKernelGGL(cover_reduce2_kernel, dim3((K + 255) / 256), dim3(256), 0, st, slab, chunks, K, cov);
    LAUNCH_CHECK();
    return 0;
}

// the three select levels and the binned sums over keys[n], from the targets a select_init*_kernel has seeded in sel
static int select_levels(const uint32_t* keys, int64_t n, GroupSelect* sel, uint32_t* hist, unsigned long long* raw, hipStream_t st)
{
    static const int level_bits[3] = {11, 10, 10};
    int shift = 31;
    for (int l = 0; l < 3; ++l) {
        const int bits = level_bits[l];
        shift -= bits;
        if (hipMemsetAsync(hist, 0, (size_t)GROUP_HIST_WORDS * 4, st) != hipSuccess) return (int)hipGetLastError();
        hipLaunchKernelGGL(select_hist_kernel, dim3(pass_grid(n)), dim3(256), 0, st, keys, n, shift, bits, sel, hist);
        hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(GROUP_MAX_TARGETS), 0, st, bits, sel, hist);
    }
    if (hipMemsetAsync(raw, 0, (size_t)4 * GROUP_MAX_TARGETS * 8, st) != hipSuccess) return (int)hipGetLastError();
    hipLaunchKernelGGL(bin_sums_kernel, dim3(pass_grid(n)), dim3(256), 0, st, keys, n, sel, raw);
    LAUNCH_CHECK();
    return 0;
}

int launch_group_select(const uint32_t* keys, int64_t n, const long long* totals, int n_bins, GroupSelect* sel, uint32_t* hist,
                        unsigned long long* raw, hipStream_t st)
{
    if (n < 1 || !keys || !totals || n_bins < 1 || n_bins > GROUP_MAX_BINS || !sel || !hist || !raw) return -19;
    hipLaunchKernelGGL(select_init_kernel, dim3(1), dim3(GROUP_MAX_TARGETS), 0, st, totals, n_bins, sel);
    return select_levels(keys, n, sel, hist, raw, st);
}

int launch_group_category_counts(const unsigned long long* support, const int32_t* category_of_class, int K, int n_categories,
                                 long long* cat_rows, int32_t* cat_bins, hipStream_t st)
{
    if (!support || !category_of_class || K < 1 || n_categories < 1 || n_categories > GROUP_MAX_CATEGORIES || !cat_rows || !cat_bins) return -19;
    hipLaunchKernelGGL(category_counts_kernel, dim3(1), dim3(GROUP_MAX_CATEGORIES), 0, st, support, category_of_class, K, n_categories, cat_rows,
                       cat_bins);
    LAUNCH_CHECK();
    return 0;
}

int launch_group_select_category(const uint32_t* keys, const uint8_t* seg, int64_t n, int c, const long long* cat_rows, const int32_t* cat_bins,
                                 uint32_t* ckeys, GroupSelect* sel, uint32_t* hist, unsigned long long* raw, hipStream_t st)
{
    if (n < 1 || !keys || !seg || c < 0 || c >= GROUP_MAX_CATEGORIES || !cat_rows || !cat_bins || !ckeys || !sel || !hist || !raw) return -19;
    hipLaunchKernelGGL(category_mask_kernel, dim3(pass_grid(n)), dim3(256), 0, st, keys, seg, n, c, ckeys);
    hipLaunchKernelGGL(select_init_category_kernel, dim3(1), dim3(GROUP_MAX_TARGETS), 0, st, cat_rows, cat_bins, c, sel);
    return select_levels(ckeys, n, sel, hist, raw, st);
}
