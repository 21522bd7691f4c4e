// targets.hip -- per-row soft targets resident on one device (gfx950): storage of mmc_targetset_* (include/mmc.h, "distillation").
//
// No counterpart in the reference, whose trainer knows hard labels only.  A target set is the N x K matrix a distilled pass reads in
// place (trainer.hip, ce_grad_distill_kernel); it is filled from the host, from device rows, or by mmc_ensemble_predict_set
// (mmc_ensemble.cpp) chunk by chunk without a host round trip.
//
// Storage: P [cap][K] fp32 row-major, grown as featureset.hip grows X: the new buffer is allocated first, so a refused call changes
// nothing.  The commit rule: new rows are written past the committed row count, target_rows_kernel validates them on the device,
// one int32 comes back, and the count moves only if no row is invalid.  Readers never see rows past the count.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <climits>
#include <cmath>
#include <utility>
#include <vector>

#include "../../include/mmc.h"
#include "trainer_internal.h"

namespace {

// One wave per row, four rows per 256-thread workgroup.  A row is valid when every entry is finite and >= 0 and its sum, taken in
// double in class order, is within 1e-3 of 1.  The loads are lane-strided (coalesced); the sum walks each group of 64 classes in lane
// order through a broadcast, so every lane adds the same terms in class order.  The first bad row of the launch is the minimum of
// the bad rows' indices: one integer atomicMin per bad row, so the result does not depend on the order the waves run in.
__global__ __launch_bounds__(256) void target_rows_kernel(const float* __restrict__ P, int64_t n, int K, int32_t* __restrict__ first_bad)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float* p = P + (size_t)row * K;
    bool bad = false;
    double sum = 0.0;
    for (int c0 = 0; c0 < K; c0 += 64) {
        const int c = c0 + lane;
        const float v = c < K ? p[c] : 0.f;
        bad = bad || !(v >= 0.f && v <= 3.402823466e+38f);
        const int cnt = K - c0 < 64 ? K - c0 : 64;
        for (int l = 0; l < cnt; ++l) sum += (double)__shfl(v, l);
    }
    bad = __any(bad) || !(fabs(sum - 1.0) <= 1e-3);
    if (bad && lane == 0) atomicMin(first_bad, (int32_t)row);
}

// why a row is invalid, in the words of the header: the kernel's rule on a host copy of the row
int describe_bad_row(const std::vector<float>& row, long long label)
{
    double sum = 0.0;
    for (size_t c = 0; c < row.size(); ++c) {
        if (!(row[c] >= 0.f && std::isfinite(row[c])))
            return mmc_fail(MMC_ERR_ARG, "row %lld: entry %d = %g is negative or not finite", label, (int)c, (double)row[c]);
        sum += (double)row[c];
    }
    return mmc_fail(MMC_ERR_ARG, "row %lld sums to %.6g, not 1 within 1e-3", label, sum);
}

}  // namespace

int target_rows_check(const float* P_dev, int64_t n, int K, int32_t* verdict_dev, int64_t label_first, hipStream_t st)
{
    // rows go in launches of at most 2^30 so that the row index of a launch fits the int32 the atomic reduces
    const int64_t step = (int64_t)1 << 30;
    for (int64_t off = 0; off < n; off += step) {
        const int64_t cur = (n - off) < step ? (n - off) : step;
        int32_t h = INT_MAX;
        HIP_TRY(hipMemcpyAsync(verdict_dev, &h, 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(target_rows_kernel, dim3((unsigned)((cur + 3) / 4)), dim3(256), 0, st, P_dev + (size_t)off * K, cur, K, verdict_dev);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&h, verdict_dev, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (h != INT_MAX) {
            std::vector<float> row((size_t)K);
            HIP_TRY(hipMemcpy(row.data(), P_dev + (size_t)(off + h) * K, (size_t)K * 4, hipMemcpyDeviceToHost));
            return describe_bad_row(row, (long long)(label_first + off + h));
        }
    }
    return MMC_OK;
}

int targetset_reserve(mmc_targetset* ts, int64_t need, hipStream_t st)
{
    if (need > MMC_TARGETSET_MAX_CELLS / ts->K)
        return mmc_fail(MMC_ERR_ARG, "%lld rows x %d classes: a target set holds at most %lld cells (MMC_TARGETSET_MAX_CELLS)", (long long)need,
                        ts->K, (long long)MMC_TARGETSET_MAX_CELLS);
    if (need <= ts->cap) return MMC_OK;
    int64_t cap = ts->cap * 2 > need ? ts->cap * 2 : need;
    if (cap > MMC_TARGETSET_MAX_CELLS / ts->K) cap = MMC_TARGETSET_MAX_CELLS / ts->K;
    DevBuf<float> P;
    if (!P.alloc(cap * ts->K)) return mmc_fail(MMC_ERR_NOMEM, "hipMalloc of %lld x %d targets failed", (long long)cap, ts->K);
    if (ts->n) {
        hipError_t e = hipMemcpyAsync(P, ts->P, (size_t)ts->n * ts->K * 4, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return mmc_fail(MMC_ERR_HIP, "moving %lld rows to the grown target set: %s", (long long)ts->n, hipGetErrorString(e));
    }
    ts->P = std::move(P);
    ts->cap = cap;
    return MMC_OK;
}

int targetset_commit(mmc_targetset* ts, int64_t n, int64_t label_first, hipStream_t st)
{
    int r = ts->verdict.reserve(4);
    if (r) return r;
    // a refused fill leaves its rows past the count, where nobody reads them
    if ((r = target_rows_check(ts->P + (size_t)ts->n * ts->K, n, ts->K, ts->verdict, label_first, st))) return r;
    ts->n += n;
    return MMC_OK;
}

extern "C" void mmc_targetset_destroy(mmc_targetset* ts)
{
    if (!ts) return;
    hipSetDevice(ts->device);
    delete ts;
}

extern "C" int mmc_targetset_create(int K, int device, int64_t reserve_rows, mmc_targetset** out)
{
    if (!out) return mmc_fail(MMC_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (K < 1) return mmc_fail(MMC_ERR_ARG, "K = %d must be positive", K);
    if (reserve_rows < 0) return mmc_fail(MMC_ERR_ARG, "reserve_rows = %lld is negative", (long long)reserve_rows);
    if (reserve_rows > MMC_TARGETSET_MAX_CELLS / K)
        return mmc_fail(MMC_ERR_ARG, "%lld rows x %d classes: a target set holds at most %lld cells (MMC_TARGETSET_MAX_CELLS)",
                        (long long)reserve_rows, K, (long long)MMC_TARGETSET_MAX_CELLS);
    if (int r = check_device(device)) return r;
    HIP_TRY(hipSetDevice(device));
    mmc_targetset* ts = new mmc_targetset();
    ts->K = K;
    ts->device = device;
    if (reserve_rows) {
        const int r = targetset_reserve(ts, reserve_rows, nullptr);
        if (r) {
            mmc_targetset_destroy(ts);
            return r;
        }
    }
    *out = ts;
    return MMC_OK;
}

extern "C" int64_t mmc_targetset_rows(const mmc_targetset* ts) { return ts ? ts->n : 0; }
extern "C" int mmc_targetset_num_classes(const mmc_targetset* ts) { return ts ? ts->K : 0; }

extern "C" int mmc_targetset_append(mmc_targetset* ts, const float* P, int64_t n, unsigned flags, void* hip_stream)
{
    if (!ts) return mmc_fail(MMC_ERR_ARG, "target set handle is NULL");
    if (n < 0) return mmc_fail(MMC_ERR_ARG, "n = %lld is negative", (long long)n);
    if (flags != MMC_IN_HOST && flags != MMC_IN_DEVICE)
        return mmc_fail(MMC_ERR_ARG, "flags 0x%x: MMC_IN_HOST or MMC_IN_DEVICE", flags);
    if (n == 0) return MMC_OK;
    if (!P) return mmc_fail(MMC_ERR_ARG, "P is NULL");
    if (n > MMC_TARGETSET_MAX_CELLS / ts->K - ts->n)
        return mmc_fail(MMC_ERR_ARG, "%lld + %lld rows x %d classes: a target set holds at most %lld cells (MMC_TARGETSET_MAX_CELLS)",
                        (long long)ts->n, (long long)n, ts->K, (long long)MMC_TARGETSET_MAX_CELLS);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(ts->device));
    int r = targetset_reserve(ts, ts->n + n, st);
    if (r) return r;
    HIP_TRY(hipMemcpyAsync(ts->P + (size_t)ts->n * ts->K, P, (size_t)n * ts->K * 4,
                           flags == MMC_IN_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
    return targetset_commit(ts, n, 0, st);
}

extern "C" int mmc_targetset_read(mmc_targetset* ts, int64_t first, int64_t n, float* P, void* hip_stream)
{
    if (!ts) return mmc_fail(MMC_ERR_ARG, "target set handle is NULL");
    if (first < 0 || n < 0 || first > ts->n || n > ts->n - first)
        return mmc_fail(MMC_ERR_ARG, "rows [%lld, %lld + %lld) outside the set's %lld rows", (long long)first, (long long)first, (long long)n,
                        (long long)ts->n);
    if (n == 0) return MMC_OK;
    if (!P) return mmc_fail(MMC_ERR_ARG, "P is NULL");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(ts->device));
    HIP_TRY(hipMemcpyAsync(P, ts->P + (size_t)first * ts->K, (size_t)n * ts->K * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MMC_OK;
}
