// trainer_internal.h -- what calib.hip takes from the trainer: the eval-mode forward of a trainer's current parameters (trainer.hip)
// and its scratch and shape (trainer_options.cpp); and the device-resident feature set (featureset.hip) that the trainer's passes
// and calib.hip read rows and labels from.  The trainer's own units share trainer_state.h.
// Library-internal; not part of the C ABI (include/mmc.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "device_mem.h"

struct mmc_trainer;

// mmc_featureset_*: n labelled rows resident on one device.  X / y hold `cap` rows; growth is geometric (featureset.hip).
struct mmc_featureset {
    int dim = 0, K = 0, device = 0;
    int64_t n = 0, cap = 0;
    DevBuf<float> X;                  // [cap][dim] fp32, row-major
    DevBuf<int32_t> y;                // [cap] class indices
    std::vector<int32_t> y_host;      // host mirror of y[0..n): argument checks and per-mini-batch class-weight sums
};

// room for `need` rows in all (featureset.hip): both new buffers are allocated before anything is touched, the stored rows move on `st`
int featureset_reserve(mmc_featureset* fs, int64_t need, hipStream_t st);

// mmc_targetset_*: n rows of per-row class distributions resident on one device (targets.hip); row i belongs to row i of a feature
// set.  P holds `cap` rows and grows as a feature set does.  Rows [0, n) are valid distributions (include/mmc.h, "distillation").
struct mmc_targetset {
    int K = 0, device = 0;
    int64_t n = 0, cap = 0;
    DevBuf<float> P;                  // [cap][K] fp32, row-major
    DevBuf<int32_t> verdict;          // the validation kernel's result: the first bad row of a launch
};

// room for `need` rows in all (targets.hip): the new buffer is allocated before anything is touched, the stored rows move on `st`;
// more than MMC_TARGETSET_MAX_CELLS cells is refused before anything is allocated
int targetset_reserve(mmc_targetset* ts, int64_t need, hipStream_t st);
// the commit rule: rows [ts->n, ts->n + n) have been written on `st`; validates them on the device, reads one result back and moves
// the row count only if every row is a distribution, else MMC_ERR_ARG naming the first bad row (numbered from `label_first`)
int targetset_commit(mmc_targetset* ts, int64_t n, int64_t label_first, hipStream_t st);
// the same rule for n rows x K of P that belong to no set (the distillation probe): `verdict_dev` is one int32 on the device; bad rows are numbered from `label_first`
int target_rows_check(const float* P_dev, int64_t n, int K, int32_t* verdict_dev, int64_t label_first, hipStream_t st);

// rows per trainer_forward call (the trainer's activation buffers are sized for at most this many)
constexpr int kTrainerForwardRows = 16384;

int trainer_classes(const mmc_trainer* t);     // K = dims[n_layers]
int trainer_input_dim(const mmc_trainer* t);   // dims[0]
int trainer_device(const mmc_trainer* t);

// *out = a device buffer of at least `bytes` owned by the trainer (grown on demand, freed with it), for work that runs on the
// trainer's stream: calib.hip's evaluation labels and partial sums, so that an evaluation per batch allocates nothing.
int trainer_scratch(mmc_trainer* t, size_t bytes, void** out);

// Uploads n (1..kTrainerForwardRows) host rows X[n][dims[0]] and runs Linear/ReLU ... Linear on `st` with the exact kernels of
// a training step's forward; *logits = device [n][K] fp32, valid until the next call on `t` (stream-ordered, no sync).
int trainer_forward(mmc_trainer* t, const float* X, int n, hipStream_t st, const float** logits);
// The same on rows that are already on the trainer's device (a feature set's): nothing is uploaded, the first layer reads X.
int trainer_forward_device(mmc_trainer* t, const float* X_dev, int n, hipStream_t st, const float** logits);

// argument checks shared by calib.hip and logit_scaling.hip (defined in calib.hip); each sets the error message and returns MMC_ERR_ARG
int check_labels(const int32_t* y, int64_t n, int K);                        // every y[i] in [0, K)
int check_set_range(const mmc_featureset* fs, int64_t first, int64_t n);     // rows [first, first + n) inside the set
int check_set_matches(const mmc_featureset* fs, mmc_trainer* t);             // width, classes and device of set and trainer agree
