// trainer_state.h -- the trainer's state and what its three translation units take from each other: trainer.hip (the kernels and
// every launch of them), trainer_options.cpp (handle, option setters, state up and down) and trainer_pass.cpp (the passes).
// Host-only and library-internal; the other units of the library see a trainer through trainer_internal.h alone.
#pragma once
#include <vector>

#include "trainer_internal.h"

struct mmc_trainer {
    int device = 0, L = 0, K = 0;
    std::vector<int> dims;
    std::vector<DevBuf<float>> W, b, gW, gb, mW, vW, mb, vb;
    std::vector<DevBuf<float>> Hbuf, dZbuf;             // the activations and their gradients of layers 1..L ([0] stays empty)
    std::vector<float*> H;                              // views: H[0] = mini-batch input, H[l+1] = layer l's output; size L+1
    std::vector<float*> dZ;                             // views: dZ[l] = gradient w.r.t. layer l-1's pre-activation (size L+1, [0] unused)
    DevBuf<float> cw;                                   // class weights or empty
    DevBuf<float> X, row_loss, partials, losses;
    DevBuf<int32_t> y;
    DevBuf<float> Xn;               // natural-order staging of a pass (device-side shuffle)
    DevBuf<int32_t> yn;
    DevBuf<int64_t> order;
    DevBuf<int64_t> visit;          // visiting order of a pass over a resident feature set
    double lr = 1e-3, beta1 = 0.9, beta2 = 0.999, eps = 1e-8, alpha = 1e-4;   // kept in double: torch derives its fp32 scalars from python floats
    long long t = 0;                                    // Adam step count
    std::vector<float> cw_host;
    // loss formulation (mmc_trainer_set_loss); all defaults = the plain weighted cross-entropy and its instantiation of the kernel
    double label_smoothing = 0.0, focal_gamma = 0.0;
    DevBuf<float> prior;                                // logit prior [K] or empty
    bool general = false;
    float w_total = 0.f;                                // the float of the double sum of the class weights in class order; K without
    DevBuf<char> scratch;                               // trainer_scratch (calib.hip's evaluation buffers)
    // regularisers (mmc_trainer_set_dropout; the plan of a mixed pass): all off = today's launches
    double p_input = 0.0, p_hidden = 0.0;
    uint64_t drop_seed = 0;
    uint32_t thresh_input = 0, thresh_hidden = 0;       // (uint32)floor(p 2^32); 0 = off
    float scale_input = 1.f, scale_hidden = 1.f;        // (float)(1.0 / (1.0 - p))
    DevBuf<int32_t> y2;                                 // the partner's label of every staged row of a mixed pass
    DevBuf<int64_t> partner;                            // device copy of a mixed pass's partner rows
    DevBuf<float> lam;                                  // device copy of its per-mini-batch lam
    // optimiser options (mmc_trainer_set_lr_schedule / _set_grad_clip / _set_ema): all off = today's launches
    int lr_kind = MMC_LR_CONSTANT;
    long long warmup_steps = 0, total_steps = 0;
    double final_ratio = 0.0;
    double max_norm = 0.0;                              // 0 = no clipping
    DevBuf<float> gpartials;                            // [2 * 16 + 1][256] partial sums of squares of gW[l] (2l), gb[l] (2l + 1), bn_g (2L)
    DevBuf<float> coef;                                 // the step's clipping coefficient
    DevBuf<float> gnorm;                                // pre-clip norm of every step of a pass, beside losses
    int gnorm_steps = 0;                                // steps of the last pass that wrote gnorm
    double ema_decay = 0.0;                             // 0 = no averaged weights
    std::vector<DevBuf<float>> sW, sb;                  // the shadow: averaged weights (empty without)
    int eval_which = MMC_WEIGHTS_RAW;                   // what the eval-mode forward reads
    // group-robust training (mmc_trainer_set_group_dro; the arrays of a weighted pass): all off = today's launches
    int n_groups = 0;                                   // 0 = no group DRO
    double dro_eta = 0.0;
    DevBuf<double> logq;                                // [n_groups] log q, normalised; lives across steps and passes
    DevBuf<float> row_w;                                // device copy of a weighted pass's row weights, by position
    DevBuf<int32_t> row_g;                              // and of its groups
    DevBuf<double> group_mass;                          // [steps][n_groups] V_a of every mini-batch of the pass
    DevBuf<float> row_scale;                            // [mb] c_i of the step
    // taxonomy-aware loss (mmc_trainer_set_hierarchy): nothing set = today's launches
    int hier_levels = 0;
    float hier_lam[MMC_HIER_MAX_LEVELS] = {0.f, 0.f, 0.f, 0.f};
    DevBuf<int32_t> hier_ids;                           // [hier_levels][K] node ids or empty
    DevBuf<float> hier_T;                               // [K][K] soft targets or empty
    bool hier = false;                                  // hier_levels > 0 or soft targets: the member takes ce_grad_hier_kernel
    // distillation (mmc_trainer_set_distillation; the target set of a distilled pass): alpha = 0 = today's launches
    double distill_alpha = 0.0, distill_tau = 1.0;
    // batch normalisation (mmc_trainer_set_batch_norm): off = today's launches.  Hidden layer h (0 .. L-2) owns [bn_off[h],
    // bn_off[h] + 2 dims[h+1]) of every bn_* array: gamma then beta in bn_p (bn_g, bn_m, bn_v alike, so Adam and the clipping norm
    // take all of them in one launch each), running mean then variance in bn_run, the step's mean then rstd in bn_stat.
    bool bn = false;
    double bn_eps = 1e-5, bn_mom = 0.1;
    std::vector<int64_t> bn_off;
    int64_t bn_total = 0;                               // 2 x the sum of the hidden widths
    DevBuf<float> bn_p, bn_g, bn_m, bn_v, bn_run, bn_stat;
    std::vector<DevBuf<float>> Zbuf;                    // [l + 1]: Z of hidden layer l, [mb][dims[l + 1]] (the backward reads it)
    std::vector<DevBuf<float>> fW, fb;                  // the folded hidden layers, what the eval-mode forward reads
    bool fold_stale = true;                             // a step or a state upload since the last fold
    float* bn_ptr(const DevBuf<float>& a, int h, int second) const { return a.p + bn_off[h] + (second ? dims[h + 1] : 0); }
};

// one trainer's part in a step: its mini-batch is rows [off, off + cur) of its staging X / y, its loss goes to losses[slot]
struct StepMember {
    mmc_trainer* t;
    int64_t off;
    int cur;
    float inv_wsum;   // 1 / sum of the mini-batch's class weights (of a mixed one: of lam w[ya] + oml w[yb])
    int slot;
    bool mixed;       // the rows were mixed: t->y2 holds the partners' labels, the loss stage takes two targets
    float lam;
    // group-robust training: a weighted member takes ce_grad_weighted_kernel; inv_wsum is then 1 / sum of the row masses, or 1.0f
    // with groups, whose rows dro_update_kernel and row_scale_kernel normalise
    bool weighted = false;
    const float* rw = nullptr;      // device: the weights of the mini-batch's positions, or null (all 1)
    const int32_t* rg = nullptr;    // device: their groups, or null (row weights only)
    const double* V = nullptr;      // device: [n_groups] the groups' masses in this mini-batch
    // distillation: a member with targets takes ce_grad_distill_kernel (row weights ride it); position i of the mini-batch reads
    // row (q_visit ? q_visit[q_start + i] : q_start + i) of q in place
    const float* q = nullptr;           // device: the target set's rows [.][K], or null (no targets)
    const int64_t* q_visit = nullptr;   // device: the pass's visiting order (t->visit), or null
    int64_t q_start = 0;                // the mini-batch's start in the pass
};

// rows of the mini-batch that starts at row `start` of a pass over n rows
inline int batch_rows(int64_t n, int64_t start, int mb) { return (int)((n - start) < mb ? (n - start) : mb); }

// trainer.hip, each described where it is defined
int trainer_group_step(const StepMember* act, int cnt, hipStream_t st);   // cnt in [1, MMC_TRAINER_GROUP_MAX]
int trainer_reserve(mmc_trainer* t, int64_t n, int mb, int steps);
int trainer_refresh_fold(mmc_trainer* t, hipStream_t st);
void gather_ordered(mmc_trainer* t, int64_t n, hipStream_t st);
int gather_chunk(mmc_trainer* t, const mmc_featureset* fs, bool visited, bool mixed, int mb, int64_t c0, int rows, hipStream_t st);
// trainer_pass.cpp: the weighted loss probe of trainer.hip is a weighted pass of one mini-batch
int minibatch_masses(const char* who, const mmc_trainer* t, const int32_t* y, const int64_t* idx, const float* rw, const int32_t* rg, int G,
                     int64_t n, int mb, std::vector<double>* wsums, std::vector<double>* vmass);
