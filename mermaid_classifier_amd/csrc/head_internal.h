// head_internal.h -- the calibrated head's handle, shared by its own unit (mmc_head.cpp) and the ensemble (mmc_ensemble.cpp), which
// borrows its members' device weights and Platt parameters.  Library-internal; not part of the C ABI (include/mmc.h).
#pragma once
#include <stdint.h>

#include <vector>

#include "device_mem.h"

// rows per chunk of every pass over a head
static const int64_t HEAD_CHUNK = 65536;
// rows of features mmc_classify_patches keeps between backbone and head: a larger call works through chunks of exactly this size
// (and one remainder), so the (patches chunk, feature buffer, n) combinations of a repeated call recur and keep their graphs
static const int64_t CLASSIFY_CHUNK = 4096;

// what a cover call keeps between calls: the resident n x K probabilities, the stage's device state (tables, offsets, slab list,
// priors, slab sums, top-k staging: cover_layout) and the host side of the slab list
struct CoverScratch {
    DevBuf<float> proba;
    DevBuf<char> dev;
    std::vector<int64_t> slab_row0, group_slab0;
    std::vector<int32_t> slab_group;
    std::vector<double> prior;
};

struct mmc_head {
    int device = 0, n_layers = 0, K = 0, input_dim = 0, in_pad = 0;
    std::vector<int> dims_pad;        // padded widths (multiples of 4), last = K (unpadded)
    std::vector<DevBuf<float>> W, b;  // device
    DevBuf<float> a, bc;
    // one chunk's activations (ping-pong, as wide as the widest layer), padded input rows, probabilities and arg-max
    DevBuf<float> buf0, buf1, in_stage, proba_stage;
    DevBuf<int32_t> arg_stage;
    // mmc_head_topk: device staging of one chunk's (rows, k) outputs for MMC_OUT_HOST
    DevBuf<int32_t> topk_idx_stage;
    DevBuf<float> topk_score_stage;
    // mmc_classify_patches: the features between backbone and head, up to CLASSIFY_CHUNK rows
    DevBuf<float> cls_feats;
    // mmc_head_evaluate*: one chunk's labels and per-row outputs ([6][rows] dwords), the label map, and the int64 totals / rank
    // histogram / confusion table
    DevBuf<int32_t> eval_rows, eval_map;
    DevBuf<long long> eval_tot;
    // mmc_head_evaluate_grouped*: offsets, per-image counts, per-class and per-source tables, reliability keys, select state, slabs
    DevBuf<char> grp;
    // mmc_head_evaluate_ranked*: the int64 class_rank_hist and hier_hist tables, then the uploaded similarity levels
    DevBuf<char> rnk;
    // mmc_head_cover*: the resident probabilities of the call's points and the cover stage's state
    CoverScratch cover;
};
