// featureset.hip -- a labelled feature split resident on one device (gfx950): storage of mmc_featureset_*.
//
// Replaces the role of ImageLabels.load_data_in_batches in the reference's epoch loop (mermaid_classifier/pyspacer/trainer.py:141-145,
// and the ref / val streams of :295-342, :344-396): there every epoch re-reads every split from disk in RAM-sized batches; here a split
// is uploaded (or written by the backbone) once and every later pass, evaluation and calibration reads it in place.
// Its readers are mmc_trainer_partial_fit_set (trainer.hip), mmc_trainer_evaluate_set_q32 and mmc_calibrator_add_set (calib.hip).
//
// Storage: X [cap][dim] fp32 row-major and y [cap] int32 on the device, plus a host mirror of the labels.  An append that does not fit
// allocates max(2 cap, rows needed) rows, moves the old rows with one device-to-device copy and frees the old
// buffers; both new buffers are allocated before anything is touched, so a failed allocation leaves the set as it was.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>
#include <utility>
#include <vector>

#include "../../include/mmc.h"
#include "trainer_internal.h"

// room for `need` rows; the rows stored so far move on `st` (also features.hip's way to grow a set)
int featureset_reserve(mmc_featureset* fs, int64_t need, hipStream_t st)
{
    if (need <= fs->cap) return MMC_OK;
    const int64_t cap = fs->cap * 2 > need ? fs->cap * 2 : need;
    DevBuf<float> X;
    DevBuf<int32_t> y;
    if (!X.alloc(cap * fs->dim)) return mmc_fail(MMC_ERR_NOMEM, "hipMalloc of %lld x %d features failed", (long long)cap, fs->dim);
    if (!y.alloc(cap)) return mmc_fail(MMC_ERR_NOMEM, "hipMalloc of %lld labels failed", (long long)cap);
    if (fs->n) {
        hipError_t e = hipMemcpyAsync(X, fs->X, (size_t)fs->n * fs->dim * 4, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(y, fs->y, (size_t)fs->n * 4, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess)
            return mmc_fail(MMC_ERR_HIP, "moving %lld rows to the grown feature set: %s", (long long)fs->n, hipGetErrorString(e));
    }
    fs->X = std::move(X);
    fs->y = std::move(y);
    fs->cap = cap;
    return MMC_OK;
}

extern "C" void mmc_featureset_destroy(mmc_featureset* fs)
{
    if (!fs) return;
    hipSetDevice(fs->device);
    delete fs;
}

extern "C" int mmc_featureset_create(int dim, int n_classes, int device, int64_t reserve_rows, mmc_featureset** out)
{
    if (!out) return mmc_fail(MMC_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (dim < 1) return mmc_fail(MMC_ERR_ARG, "dim = %d must be positive", dim);
    if (n_classes < 1) return mmc_fail(MMC_ERR_ARG, "n_classes = %d must be positive", n_classes);
    if (reserve_rows < 0) return mmc_fail(MMC_ERR_ARG, "reserve_rows = %lld is negative", (long long)reserve_rows);
    if (int r = check_device(device)) return r;
    HIP_TRY(hipSetDevice(device));
    mmc_featureset* fs = new mmc_featureset();
    fs->dim = dim;
    fs->K = n_classes;
    fs->device = device;
    if (reserve_rows) {
        const int r = featureset_reserve(fs, reserve_rows, nullptr);
        if (r) {
            mmc_featureset_destroy(fs);
            return r;
        }
    }
    *out = fs;
    return MMC_OK;
}

extern "C" int64_t mmc_featureset_rows(const mmc_featureset* fs) { return fs ? fs->n : 0; }
extern "C" int mmc_featureset_dim(const mmc_featureset* fs) { return fs ? fs->dim : 0; }

extern "C" int mmc_featureset_append(mmc_featureset* fs, const float* X, const int32_t* y, int64_t n, unsigned flags, void* hip_stream)
{
    if (!fs) return mmc_fail(MMC_ERR_ARG, "feature set handle is NULL");
    if (n < 0) return mmc_fail(MMC_ERR_ARG, "n = %lld is negative", (long long)n);
    if (flags & ~MMC_IN_HOST) return mmc_fail(MMC_ERR_ARG, "flags 0x%x: only MMC_IN_HOST is defined here", flags);
    if (n == 0) return MMC_OK;
    if (!X || !y) return mmc_fail(MMC_ERR_ARG, "X/y is NULL");
    for (int64_t i = 0; i < n; ++i)
        if (y[i] < 0 || y[i] >= fs->K) return mmc_fail(MMC_ERR_ARG, "label index y[%lld] = %d outside [0, %d)", (long long)i, y[i], fs->K);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(fs->device));
    try {
        fs->y_host.reserve((size_t)(fs->n + n));
    } catch (const std::bad_alloc&) {
        return mmc_fail(MMC_ERR_NOMEM, "no host memory for %lld labels", (long long)(fs->n + n));
    }
    const int r = featureset_reserve(fs, fs->n + n, st);
    if (r) return r;
    HIP_TRY(hipMemcpyAsync(fs->X + (size_t)fs->n * fs->dim, X, (size_t)n * fs->dim * 4,
                         (flags & MMC_IN_HOST) ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(fs->y + fs->n, y, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    fs->y_host.insert(fs->y_host.end(), y, y + n);   // the row count moves only once the rows are there
    fs->n += n;
    return MMC_OK;
}

extern "C" int mmc_featureset_read(mmc_featureset* fs, int64_t first, int64_t n, float* X, int32_t* y, void* hip_stream)
{
    if (!fs) return mmc_fail(MMC_ERR_ARG, "feature set handle is NULL");
    if (first < 0 || n < 0 || first > fs->n || n > fs->n - first)
        return mmc_fail(MMC_ERR_ARG, "rows [%lld, %lld + %lld) outside the set's %lld rows", (long long)first, (long long)first, (long long)n,
                        (long long)fs->n);
    if (n == 0) return MMC_OK;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(fs->device));
    if (X) HIP_TRY(hipMemcpyAsync(X, fs->X + (size_t)first * fs->dim, (size_t)n * fs->dim * 4, hipMemcpyDeviceToHost, st));
    if (y) HIP_TRY(hipMemcpyAsync(y, fs->y + first, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MMC_OK;
}
