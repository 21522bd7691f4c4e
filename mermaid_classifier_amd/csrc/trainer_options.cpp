// trainer_options.cpp -- the life of a trainer handle, its option setters and its state up and down (include/mmc.h, mmc_trainer_*).
// HIP runtime API only: nothing is launched from here.  What an option means to a step is in trainer.hip's header comment.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "trainer_state.h"

extern "C" void mmc_trainer_destroy(mmc_trainer* t)
{
    if (!t) return;
    hipSetDevice(t->device);
    delete t;
}

extern "C" int mmc_trainer_create(const float* const* W, const float* const* b, const int* dims, int n_layers, double lr, double beta1,
                                  double beta2, double eps, double alpha, const float* class_weight, int device, mmc_trainer** out)
{
    if (!out) return mmc_fail(MMC_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!W || !b || !dims) return mmc_fail(MMC_ERR_ARG, "NULL argument");
    if (n_layers < 1 || n_layers > 16) return mmc_fail(MMC_ERR_ARG, "n_layers %d out of range [1,16]", n_layers);
    for (int l = 0; l <= n_layers; ++l)
        if (dims[l] < 1) return mmc_fail(MMC_ERR_ARG, "dims[%d]=%d must be positive", l, dims[l]);
    if (!(lr > 0.) || !(beta1 >= 0. && beta1 < 1.) || !(beta2 >= 0. && beta2 < 1.) || !(eps >= 0.) || !(alpha >= 0.))
        return mmc_fail(MMC_ERR_ARG, "bad optimizer hyper-parameter (lr %g, betas %g %g, eps %g, alpha %g)", lr, beta1, beta2, eps, alpha);
    const int K = dims[n_layers];
    if (class_weight)
        for (int c = 0; c < K; ++c)
            if (!(class_weight[c] >= 0.f)) return mmc_fail(MMC_ERR_ARG, "class_weight[%d] = %g is negative", c, class_weight[c]);
    if (int r = check_device(device)) return r;
    HIP_TRY(hipSetDevice(device));
    mmc_trainer* t = new mmc_trainer();
    t->device = device; t->L = n_layers; t->K = K;
    t->dims.assign(dims, dims + n_layers + 1);
    t->lr = lr; t->beta1 = beta1; t->beta2 = beta2; t->eps = eps; t->alpha = alpha;
    auto up = [&](std::vector<DevBuf<float>>& dst, const float* src, size_t n, bool zero) -> bool {
        DevBuf<float> d;
        if (!d.alloc((int64_t)n)) return false;
        if ((zero ? hipMemset(d, 0, n * 4) : hipMemcpy(d, src, n * 4, hipMemcpyHostToDevice)) != hipSuccess) return false;
        dst.push_back(std::move(d));
        return true;
    };
    bool ok = true;
    for (int l = 0; l < n_layers && ok; ++l) {
        const size_t nw = (size_t)dims[l + 1] * dims[l], nb = (size_t)dims[l + 1];
        ok = up(t->W, W[l], nw, false) && up(t->b, b[l], nb, false) && up(t->gW, nullptr, nw, true) && up(t->gb, nullptr, nb, true) &&
             up(t->mW, nullptr, nw, true) && up(t->vW, nullptr, nw, true) && up(t->mb, nullptr, nb, true) && up(t->vb, nullptr, nb, true);
    }
    if (ok && class_weight) {
        ok = t->cw.alloc(K) && hipMemcpy(t->cw, class_weight, (size_t)K * 4, hipMemcpyHostToDevice) == hipSuccess;
        t->cw_host.assign(class_weight, class_weight + K);
    }
    double wtot = (double)K;
    if (class_weight) {
        wtot = 0.0;
        for (int c = 0; c < K; ++c) wtot += (double)class_weight[c];
    }
    t->w_total = (float)wtot;
    if (ok) ok = t->partials.alloc(256 * 16);
    if (!ok) {
        mmc_trainer_destroy(t);
        return mmc_fail(MMC_ERR_NOMEM, "hipMalloc/hipMemcpy failed while creating the trainer");
    }
    t->Hbuf.resize(n_layers + 1);
    t->dZbuf.resize(n_layers + 1);
    t->H.assign(n_layers + 1, nullptr);
    t->dZ.assign(n_layers + 1, nullptr);
    *out = t;
    return MMC_OK;
}

int trainer_scratch(mmc_trainer* t, size_t bytes, void** out)
{
    if ((int64_t)bytes > t->scratch.cap) {   // only on growth: the buffer is kept for the trainer's lifetime
        HIP_TRY(hipSetDevice(t->device));
        if (int r = t->scratch.reserve((int64_t)bytes)) return r;
    }
    *out = t->scratch.p;
    return MMC_OK;
}

int trainer_classes(const mmc_trainer* t) { return t->K; }
int trainer_input_dim(const mmc_trainer* t) { return t->dims[0]; }
int trainer_device(const mmc_trainer* t) { return t->device; }

// every layer's tensor pair between the host arrays W / b and the device tensors dW / db, once the device is idle: down, or up
// when `set`
static int copy_layers(const mmc_trainer* t, bool set, const std::vector<DevBuf<float>>& dW, const std::vector<DevBuf<float>>& db,
                       float* const* W, float* const* b)
{
    HIP_TRY(hipSetDevice(t->device));
    HIP_TRY(hipDeviceSynchronize());
    for (int l = 0; l < t->L; ++l) {
        const size_t nw = (size_t)t->dims[l + 1] * t->dims[l] * 4, nb = (size_t)t->dims[l + 1] * 4;
        if (set) { HIP_TRY(hipMemcpy(dW[l], W[l], nw, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(db[l], b[l], nb, hipMemcpyHostToDevice)); }
        else { HIP_TRY(hipMemcpy(W[l], dW[l], nw, hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(b[l], db[l], nb, hipMemcpyDeviceToHost)); }
    }
    return MMC_OK;
}

extern "C" int mmc_trainer_get_params(mmc_trainer* t, float* const* W, float* const* b)
{
    if (!t || !W || !b) return mmc_fail(MMC_ERR_ARG, "NULL argument");
    return copy_layers(t, false, t->W, t->b, W, b);
}

// Optimizer state for pickling (torch_classifier.py:404-415 serialises module + optimizer state dicts):
// which = 0: exp_avg, 1: exp_avg_sq.  `set` != 0 uploads instead.  *step is read / written alike.
extern "C" int mmc_trainer_adam_state(mmc_trainer* t, int which, int set, float* const* W, float* const* b, long long* step)
{
    if (!t || !W || !b || !step) return mmc_fail(MMC_ERR_ARG, "NULL argument");
    if (which != 0 && which != 1) return mmc_fail(MMC_ERR_ARG, "which must be 0 (exp_avg) or 1 (exp_avg_sq)");
    if (int r = copy_layers(t, set != 0, which == 0 ? t->mW : t->vW, which == 0 ? t->mb : t->vb, W, b)) return r;
    if (set) t->t = *step; else *step = t->t;
    return MMC_OK;
}

extern "C" int mmc_trainer_set_loss(mmc_trainer* t, double label_smoothing, double focal_gamma, const float* logit_prior)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!(label_smoothing >= 0.0 && label_smoothing < 1.0))
        return mmc_fail(MMC_ERR_ARG, "label_smoothing = %g outside [0, 1)", label_smoothing);
    if (!(focal_gamma == 0.0 || (focal_gamma >= 1.0 && focal_gamma <= 8.0)))
        return mmc_fail(MMC_ERR_ARG, "focal_gamma = %g is neither 0 nor in [1, 8]", focal_gamma);
    if (logit_prior)
        for (int c = 0; c < t->K; ++c)
            if (!std::isfinite(logit_prior[c])) return mmc_fail(MMC_ERR_ARG, "logit_prior[%d] = %g is not finite", c, logit_prior[c]);
    if (t->hier_T.p && (label_smoothing != 0.0 || focal_gamma != 0.0))
        return mmc_fail(MMC_ERR_ARG, "label_smoothing = %g / focal_gamma = %g on a trainer with soft targets (mmc_trainer_set_hierarchy)",
                        label_smoothing, focal_gamma);
    HIP_TRY(hipSetDevice(t->device));
    // passes synchronise their stream before they return, so nothing in flight reads the prior that is replaced here
    DevBuf<float> prior;
    if (logit_prior) {
        if (!prior.alloc(t->K)) return mmc_fail(MMC_ERR_NOMEM, "hipMalloc failed for the logit prior (%d classes)", t->K);
        hipError_t e = hipMemcpy(prior, logit_prior, (size_t)t->K * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return mmc_fail(MMC_ERR_HIP, "uploading the logit prior: %s", hipGetErrorString(e));
    }
    t->prior = std::move(prior);
    t->label_smoothing = label_smoothing;
    t->focal_gamma = focal_gamma;
    t->general = label_smoothing != 0.0 || focal_gamma != 0.0 || t->prior.p != nullptr;
    return MMC_OK;
}

// ---- taxonomy-aware loss (include/mmc.h) ------------------------------------------------------------------------------------
extern "C" int mmc_trainer_set_hierarchy(mmc_trainer* t, int n_levels, const int32_t* level_of_class, const double* level_weight,
                                         const float* soft_targets)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (n_levels < 0 || n_levels > MMC_HIER_MAX_LEVELS) return mmc_fail(MMC_ERR_ARG, "n_levels = %d outside [0, %d]", n_levels, MMC_HIER_MAX_LEVELS);
    if (n_levels > 0 && (!level_of_class || !level_weight)) return mmc_fail(MMC_ERR_ARG, "n_levels = %d needs level_of_class and level_weight", n_levels);
    const int K = t->K;
    float lam[MMC_HIER_MAX_LEVELS] = {0.f, 0.f, 0.f, 0.f};
    for (int l = 0; l < n_levels; ++l) {
        if (!(level_weight[l] >= 0.0 && std::isfinite(level_weight[l]) && std::isfinite((float)level_weight[l])))
            return mmc_fail(MMC_ERR_ARG, "level_weight[%d] = %g is negative or not finite", l, level_weight[l]);
        lam[l] = (float)level_weight[l];
    }
    if (soft_targets) {
        for (int r = 0; r < K; ++r) {
            double sum = 0.0;
            for (int c = 0; c < K; ++c) {
                const float v = soft_targets[(size_t)r * K + c];
                if (!(v >= 0.f && std::isfinite(v)))
                    return mmc_fail(MMC_ERR_ARG, "soft_targets[%d][%d] = %g is negative or not finite", r, c, (double)v);
                sum += (double)v;
            }
            if (!(std::fabs(sum - 1.0) <= 1e-5)) return mmc_fail(MMC_ERR_ARG, "row %d of soft_targets sums to %.9g, not 1", r, sum);
        }
        if (t->label_smoothing != 0.0 || t->focal_gamma != 0.0)
            return mmc_fail(MMC_ERR_ARG, "soft_targets on a trainer with label_smoothing = %g / focal_gamma = %g (mmc_trainer_set_loss)",
                            t->label_smoothing, t->focal_gamma);
    }
    if ((n_levels > 0 || soft_targets) && t->distill_alpha != 0.0)
        return mmc_fail(MMC_ERR_ARG, "a hierarchy on a trainer with distillation (mmc_trainer_set_distillation, alpha = %g)", t->distill_alpha);
    HIP_TRY(hipSetDevice(t->device));
    // passes synchronise their stream before they return, so nothing in flight reads what is replaced here
    DevBuf<int32_t> ids;
    DevBuf<float> T;
    if (n_levels) {
        if (!ids.alloc((int64_t)n_levels * K)) return mmc_fail(MMC_ERR_NOMEM, "hipMalloc failed for the level ids (%d levels, %d classes)", n_levels, K);
        hipError_t e = hipMemcpy(ids, level_of_class, (size_t)n_levels * K * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return mmc_fail(MMC_ERR_HIP, "uploading the level ids: %s", hipGetErrorString(e));
    }
    if (soft_targets) {
        if (!T.alloc((int64_t)K * K)) return mmc_fail(MMC_ERR_NOMEM, "hipMalloc failed for the soft targets (%d classes)", K);
        hipError_t e = hipMemcpy(T, soft_targets, (size_t)K * K * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return mmc_fail(MMC_ERR_HIP, "uploading the soft targets: %s", hipGetErrorString(e));
    }
    t->hier_ids = std::move(ids);
    t->hier_T = std::move(T);
    t->hier_levels = n_levels;
    std::copy(lam, lam + MMC_HIER_MAX_LEVELS, t->hier_lam);
    t->hier = n_levels > 0 || t->hier_T.p != nullptr;
    return MMC_OK;
}

// ---- distillation (include/mmc.h) ---------------------------------------------------------------------------------------------
extern "C" int mmc_trainer_set_distillation(mmc_trainer* t, double alpha, double temperature)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!(alpha >= 0.0 && alpha <= 1.0)) return mmc_fail(MMC_ERR_ARG, "alpha = %g outside [0, 1]", alpha);
    if (!(temperature >= 0.25 && temperature <= 64.0)) return mmc_fail(MMC_ERR_ARG, "temperature = %g outside [0.25, 64]", temperature);
    if (alpha != 0.0 && t->hier)
        return mmc_fail(MMC_ERR_ARG, "distillation on a trainer with a hierarchy (mmc_trainer_set_hierarchy)");
    t->distill_alpha = alpha;
    t->distill_tau = alpha != 0.0 ? temperature : 1.0;
    return MMC_OK;
}

extern "C" int mmc_trainer_set_dropout(mmc_trainer* t, double p_input, double p_hidden, uint64_t seed)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!(std::isfinite(p_input) && p_input >= 0.0 && p_input <= 0.9)) return mmc_fail(MMC_ERR_ARG, "p_input = %g outside [0, 0.9]", p_input);
    if (!(std::isfinite(p_hidden) && p_hidden >= 0.0 && p_hidden <= 0.9)) return mmc_fail(MMC_ERR_ARG, "p_hidden = %g outside [0, 0.9]", p_hidden);
    if (t->bn && p_hidden > 0.0)
        return mmc_fail(MMC_ERR_ARG, "p_hidden = %g on a trainer with batch normalisation (mmc_trainer_set_batch_norm)", p_hidden);
    t->p_input = p_input;
    t->p_hidden = p_hidden;
    t->drop_seed = seed;
    t->thresh_input = (uint32_t)std::floor(p_input * 4294967296.0);
    t->thresh_hidden = (uint32_t)std::floor(p_hidden * 4294967296.0);
    t->scale_input = (float)(1.0 / (1.0 - p_input));
    t->scale_hidden = (float)(1.0 / (1.0 - p_hidden));
    return MMC_OK;
}

// ---- optimiser options (include/mmc.h) ----------------------------------------------------------------------------------
// lr_s of the 1-based step s: a pure function of the step count, all in double
extern "C" int mmc_lr_schedule_at(double lr, int kind, long long warmup_steps, long long total_steps, double final_ratio, long long step,
                                  double* out)
{
    if (!out) return mmc_fail(MMC_ERR_ARG, "out is NULL");
    if (kind != MMC_LR_CONSTANT && kind != MMC_LR_LINEAR && kind != MMC_LR_COSINE)
        return mmc_fail(MMC_ERR_ARG, "kind = %d is not MMC_LR_CONSTANT, MMC_LR_LINEAR or MMC_LR_COSINE", kind);
    if (warmup_steps < 0) return mmc_fail(MMC_ERR_ARG, "warmup_steps = %lld is negative", warmup_steps);
    if (kind != MMC_LR_CONSTANT && !(total_steps > warmup_steps))
        return mmc_fail(MMC_ERR_ARG, "a decaying schedule needs total_steps > warmup_steps (got %lld, %lld)", total_steps, warmup_steps);
    if (!(final_ratio >= 0.0 && final_ratio <= 1.0)) return mmc_fail(MMC_ERR_ARG, "final_ratio = %g outside [0, 1]", final_ratio);
    const double s = (double)step, wu = (double)warmup_steps;
    const double w = warmup_steps > 0 ? std::min(1.0, s / wu) : 1.0;
    const double u = std::min(1.0, std::max(0.0, (s - wu) / (double)std::max(1LL, total_steps - warmup_steps)));
    const double r = final_ratio;
    double d = 1.0;
    if (kind == MMC_LR_LINEAR) d = 1.0 - (1.0 - r) * u;
    if (kind == MMC_LR_COSINE) d = r + (1.0 - r) * 0.5 * (1.0 + std::cos(3.14159265358979323846 * u));   // the double nearest pi
    *out = lr * w * d;
    return MMC_OK;
}

extern "C" int mmc_trainer_set_lr_schedule(mmc_trainer* t, int kind, long long warmup_steps, long long total_steps, double final_ratio)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    double probe = 0.0;
    int r = mmc_lr_schedule_at(t->lr, kind, warmup_steps, total_steps, final_ratio, 1, &probe);
    if (r) return r;
    t->lr_kind = kind;
    t->warmup_steps = warmup_steps;
    t->total_steps = total_steps;
    t->final_ratio = final_ratio;
    return MMC_OK;
}

extern "C" int mmc_trainer_lr_at(mmc_trainer* t, long long step, double* lr)
{
    if (!t || !lr) return mmc_fail(MMC_ERR_ARG, "NULL argument");
    return mmc_lr_schedule_at(t->lr, t->lr_kind, t->warmup_steps, t->total_steps, t->final_ratio, step, lr);
}

extern "C" int mmc_trainer_set_grad_clip(mmc_trainer* t, double max_norm)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!(max_norm == 0.0 || (max_norm > 0.0 && std::isfinite(max_norm) && std::isfinite((float)max_norm) && (float)max_norm > 0.f)))
        return mmc_fail(MMC_ERR_ARG, "max_norm = %g is neither 0 nor a positive finite fp32 value", max_norm);
    if (max_norm != 0.0 && !t->gpartials) {
        HIP_TRY(hipSetDevice(t->device));
        DevBuf<float> gp, cf;
        if (!gp.alloc((2 * 16 + 1) * 256) || !cf.alloc(1)) return mmc_fail(MMC_ERR_NOMEM, "hipMalloc failed for the gradient-norm partials");
        t->gpartials = std::move(gp);
        t->coef = std::move(cf);
    }
    t->max_norm = max_norm;
    t->gnorm_steps = 0;
    return MMC_OK;
}

extern "C" int mmc_trainer_grad_norms(mmc_trainer* t, float* out, int capacity, int* steps)
{
    if (!t || !steps) return mmc_fail(MMC_ERR_ARG, "NULL argument");
    if (capacity < 0 || (capacity > 0 && !out)) return mmc_fail(MMC_ERR_ARG, "capacity = %d with out %s", capacity, out ? "set" : "NULL");
    *steps = t->gnorm_steps;
    const int n = std::min(capacity, t->gnorm_steps);
    if (n > 0) {
        HIP_TRY(hipSetDevice(t->device));
        HIP_TRY(hipMemcpy(out, t->gnorm, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    return MMC_OK;
}

extern "C" int mmc_trainer_set_ema(mmc_trainer* t, double decay)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!(decay == 0.0 || (decay > 0.0 && decay < 1.0))) return mmc_fail(MMC_ERR_ARG, "decay = %g is neither 0 nor in (0, 1)", decay);
    if (t->bn && decay != 0.0)
        return mmc_fail(MMC_ERR_ARG, "decay = %g on a trainer with batch normalisation (mmc_trainer_set_batch_norm)", decay);
    HIP_TRY(hipSetDevice(t->device));
    if (decay == 0.0) {
        t->sW.clear();
        t->sb.clear();
        t->eval_which = MMC_WEIGHTS_RAW;
    } else if (t->sW.empty()) {   // passes synchronise their stream before they return: the parameters copied here are settled
        std::vector<DevBuf<float>> sW(t->L), sb(t->L);
        bool ok = true;
        auto dup = [&](DevBuf<float>& dst, const float* src, size_t n) -> bool {
            return dst.alloc((int64_t)n) && hipMemcpy(dst, src, n * 4, hipMemcpyDeviceToDevice) == hipSuccess;
        };
        for (int l = 0; l < t->L && ok; ++l)
            ok = dup(sW[l], t->W[l], (size_t)t->dims[l + 1] * t->dims[l]) && dup(sb[l], t->b[l], (size_t)t->dims[l + 1]);
        if (!ok) {
            (void)hipGetLastError();
            return mmc_fail(MMC_ERR_NOMEM, "hipMalloc/hipMemcpy failed for the averaged weights");
        }
        t->sW = std::move(sW);
        t->sb = std::move(sb);
    }
    t->ema_decay = decay;
    return MMC_OK;
}

extern "C" int mmc_trainer_ema_state(mmc_trainer* t, int set, float* const* W, float* const* b)
{
    if (!t || !W || !b) return mmc_fail(MMC_ERR_ARG, "NULL argument");
    if (t->sW.empty()) return mmc_fail(MMC_ERR_ARG, "the trainer keeps no averaged weights (mmc_trainer_set_ema)");
    return copy_layers(t, set != 0, t->sW, t->sb, W, b);
}

extern "C" int mmc_trainer_eval_weights(mmc_trainer* t, int which)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (which != MMC_WEIGHTS_RAW && which != MMC_WEIGHTS_AVERAGED)
        return mmc_fail(MMC_ERR_ARG, "which = %d is neither MMC_WEIGHTS_RAW nor MMC_WEIGHTS_AVERAGED", which);
    if (which == MMC_WEIGHTS_AVERAGED && t->sW.empty())
        return mmc_fail(MMC_ERR_ARG, "the trainer keeps no averaged weights (mmc_trainer_set_ema)");
    t->eval_which = which;
    return MMC_OK;
}

extern "C" int mmc_trainer_optimizer_options(mmc_trainer* t, int* lr_kind, long long* warmup_steps, long long* total_steps,
                                             double* final_ratio, double* max_norm, double* ema_decay, int* eval_which)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (lr_kind) *lr_kind = t->lr_kind;
    if (warmup_steps) *warmup_steps = t->warmup_steps;
    if (total_steps) *total_steps = t->total_steps;
    if (final_ratio) *final_ratio = t->final_ratio;
    if (max_norm) *max_norm = t->max_norm;
    if (ema_decay) *ema_decay = t->ema_decay;
    if (eval_which) *eval_which = t->eval_which;
    return MMC_OK;
}

// ---- group-robust training (include/mmc.h) -------------------------------------------------------------------------------
// lse = mx + log(sum_b exp(logq_b - mx)), the sum in index order: the host form of dro_update_kernel's normaliser
static double logq_lse(const double* logq, int G)
{
    double mx = logq[0];
    for (int a = 1; a < G; ++a) mx = std::max(mx, logq[a]);
    double s = 0.0;
    for (int a = 0; a < G; ++a) s += std::exp(logq[a] - mx);
    return mx + std::log(s);
}

extern "C" int mmc_trainer_set_group_dro(mmc_trainer* t, int n_groups, double eta)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (n_groups < 0 || n_groups > MMC_DRO_MAX_GROUPS) return mmc_fail(MMC_ERR_ARG, "n_groups = %d outside [0, %d]", n_groups, MMC_DRO_MAX_GROUPS);
    if (!(eta >= 0.0 && eta <= 10.0)) return mmc_fail(MMC_ERR_ARG, "eta = %g outside [0, 10]", eta);
    HIP_TRY(hipSetDevice(t->device));
    DevBuf<double> logq;
    if (n_groups) {   // passes synchronise their stream before they return, so nothing in flight reads the state that is replaced here
        if (!logq.alloc(n_groups)) return mmc_fail(MMC_ERR_NOMEM, "hipMalloc failed for the group distribution (%d groups)", n_groups);
        const std::vector<double> uniform((size_t)n_groups, -std::log((double)n_groups));
        hipError_t e = hipMemcpy(logq, uniform.data(), (size_t)n_groups * 8, hipMemcpyHostToDevice);
        if (e != hipSuccess) return mmc_fail(MMC_ERR_HIP, "uploading the group distribution: %s", hipGetErrorString(e));
    }
    t->logq = std::move(logq);
    t->n_groups = n_groups;
    t->dro_eta = eta;
    return MMC_OK;
}

extern "C" int mmc_trainer_group_dro_state(mmc_trainer* t, int set, double* log_q)
{
    if (!t || !log_q) return mmc_fail(MMC_ERR_ARG, "NULL argument");
    if (!t->n_groups) return mmc_fail(MMC_ERR_ARG, "the trainer keeps no group distribution (mmc_trainer_set_group_dro)");
    const int G = t->n_groups;
    HIP_TRY(hipSetDevice(t->device));
    if (!set) {
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(log_q, t->logq, (size_t)G * 8, hipMemcpyDeviceToHost));
        return MMC_OK;
    }
    for (int a = 0; a < G; ++a)
        if (!std::isfinite(log_q[a])) return mmc_fail(MMC_ERR_ARG, "log_q[%d] = %g is not finite", a, log_q[a]);
    // a state that is normalised already (what a read returns: |lse| at rounding level) goes back as it is, so a resume continues
    // on the bits it left; anything else is renormalised
    std::vector<double> q(log_q, log_q + G);
    const double lse = logq_lse(q.data(), G);
    if (std::fabs(lse) > 0x1p-40)
        for (int a = 0; a < G; ++a) q[a] = q[a] - lse;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(t->logq, q.data(), (size_t)G * 8, hipMemcpyHostToDevice));
    return MMC_OK;
}

// ---- batch normalisation (include/mmc.h) -----------------------------------------------------------------------------------
extern "C" int mmc_trainer_set_batch_norm(mmc_trainer* t, int enable, double eps, double momentum)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    HIP_TRY(hipSetDevice(t->device));
    if (!enable) {   // passes synchronise their stream before they return: nothing in flight reads what is freed here
        t->bn = false;
        t->bn_p.reset(); t->bn_g.reset(); t->bn_m.reset(); t->bn_v.reset(); t->bn_run.reset(); t->bn_stat.reset();
        t->Zbuf.clear(); t->fW.clear(); t->fb.clear();
        t->bn_off.clear();
        t->bn_total = 0;
        return MMC_OK;
    }
    if (!(eps > 0.0 && std::isfinite(eps) && (float)eps > 0.f)) return mmc_fail(MMC_ERR_ARG, "eps = %g is not a positive finite fp32 value", eps);
    if (!(momentum > 0.0 && momentum <= 1.0)) return mmc_fail(MMC_ERR_ARG, "momentum = %g outside (0, 1]", momentum);
    if (t->p_hidden > 0.0)
        return mmc_fail(MMC_ERR_ARG, "batch normalisation on a trainer with hidden dropout p_hidden = %g (mmc_trainer_set_dropout)", t->p_hidden);
    if (!t->sW.empty())
        return mmc_fail(MMC_ERR_ARG, "batch normalisation on a trainer with averaged weights, decay = %g (mmc_trainer_set_ema)", t->ema_decay);
    if (!(t->eps > 0.0))
        return mmc_fail(MMC_ERR_ARG, "batch normalisation freezes the hidden biases at a zero gradient, which needs Adam's eps > 0 (got %g)", t->eps);
    if (t->bn) {   // already on: the state stays, the two scalars move
        t->bn_eps = eps;
        t->bn_mom = momentum;
        t->fold_stale = true;
        return MMC_OK;
    }
    const int H = t->L - 1;
    std::vector<int64_t> off(H);
    int64_t total = 0;
    for (int h = 0; h < H; ++h) {
        off[h] = total;
        total += 2 * (int64_t)t->dims[h + 1];
    }
    DevBuf<float> p, g, m, v, run, stat;
    std::vector<DevBuf<float>> fW(H), fb(H);
    if (total) {
        bool ok = p.alloc(total) && g.alloc(total) && m.alloc(total) && v.alloc(total) && run.alloc(total) && stat.alloc(total);
        for (int h = 0; h < H && ok; ++h) ok = fW[h].alloc((int64_t)t->dims[h + 1] * t->dims[h]) && fb[h].alloc(t->dims[h + 1]);
        if (!ok) return mmc_fail(MMC_ERR_NOMEM, "hipMalloc failed for the batch-normalisation state (%lld values)", (long long)total);
        // gamma = 1 then beta = 0; running mean 0 then running variance 1
        std::vector<float> init((size_t)total, 0.f), stats((size_t)total, 0.f);
        for (int h = 0; h < H; ++h) {
            std::fill(init.begin() + off[h], init.begin() + off[h] + t->dims[h + 1], 1.f);
            std::fill(stats.begin() + off[h] + t->dims[h + 1], stats.begin() + off[h] + 2 * t->dims[h + 1], 1.f);
        }
        HIP_TRY(hipMemcpy(p, init.data(), (size_t)total * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(run, stats.data(), (size_t)total * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(g, 0, (size_t)total * 4));
        HIP_TRY(hipMemset(m, 0, (size_t)total * 4));
        HIP_TRY(hipMemset(v, 0, (size_t)total * 4));
        HIP_TRY(hipMemset(stat, 0, (size_t)total * 4));
        // the bias of a normalised layer cancels: its gradient is zero from here on (no colsum launch writes it)
        for (int h = 0; h < H; ++h) HIP_TRY(hipMemset(t->gb[h], 0, (size_t)t->dims[h + 1] * 4));
    }
    t->bn_p = std::move(p); t->bn_g = std::move(g); t->bn_m = std::move(m); t->bn_v = std::move(v);
    t->bn_run = std::move(run); t->bn_stat = std::move(stat);
    t->fW = std::move(fW); t->fb = std::move(fb);
    t->Zbuf.clear();
    t->Zbuf.resize(t->L + 1);
    t->bn_off = std::move(off);
    t->bn_total = total;
    t->bn_eps = eps;
    t->bn_mom = momentum;
    t->bn = true;
    t->fold_stale = true;
    return MMC_OK;
}

extern "C" int mmc_trainer_batch_norm_state(mmc_trainer* t, int set, float* const* gamma, float* const* beta, float* const* running_mean,
                                            float* const* running_var, float* const* adam_m_gamma, float* const* adam_v_gamma,
                                            float* const* adam_m_beta, float* const* adam_v_beta)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!gamma || !beta || !running_mean || !running_var || !adam_m_gamma || !adam_v_gamma || !adam_m_beta || !adam_v_beta)
        return mmc_fail(MMC_ERR_ARG, "NULL argument");
    if (!t->bn) return mmc_fail(MMC_ERR_ARG, "the trainer has no batch normalisation (mmc_trainer_set_batch_norm)");
    HIP_TRY(hipSetDevice(t->device));
    HIP_TRY(hipDeviceSynchronize());
    for (int h = 0; h < t->L - 1; ++h) {
        const size_t nb = (size_t)t->dims[h + 1] * 4;
        float* host[8] = {gamma[h], beta[h], running_mean[h], running_var[h], adam_m_gamma[h], adam_m_beta[h], adam_v_gamma[h], adam_v_beta[h]};
        float* dev[8] = {t->bn_ptr(t->bn_p, h, 0), t->bn_ptr(t->bn_p, h, 1), t->bn_ptr(t->bn_run, h, 0), t->bn_ptr(t->bn_run, h, 1),
                         t->bn_ptr(t->bn_m, h, 0), t->bn_ptr(t->bn_m, h, 1), t->bn_ptr(t->bn_v, h, 0), t->bn_ptr(t->bn_v, h, 1)};
        for (int a = 0; a < 8; ++a) {
            if (!host[a]) return mmc_fail(MMC_ERR_ARG, "NULL array for hidden layer %d", h);
            if (set) HIP_TRY(hipMemcpy(dev[a], host[a], nb, hipMemcpyHostToDevice));
            else HIP_TRY(hipMemcpy(host[a], dev[a], nb, hipMemcpyDeviceToHost));
        }
    }
    if (set) t->fold_stale = true;
    return MMC_OK;
}

extern "C" int mmc_trainer_folded_params(mmc_trainer* t, float* const* W, float* const* b)
{
    if (!t || !W || !b) return mmc_fail(MMC_ERR_ARG, "NULL argument");
    if (!t->bn) return mmc_trainer_get_params(t, W, b);
    HIP_TRY(hipSetDevice(t->device));
    HIP_TRY(hipDeviceSynchronize());
    if (int r = trainer_refresh_fold(t, nullptr)) return r;
    HIP_TRY(hipDeviceSynchronize());
    for (int l = 0; l < t->L; ++l) {
        const bool folded = l < t->L - 1;
        HIP_TRY(hipMemcpy(W[l], folded ? t->fW[l].p : t->W[l].p, (size_t)t->dims[l + 1] * t->dims[l] * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(b[l], folded ? t->fb[l].p : t->b[l].p, (size_t)t->dims[l + 1] * 4, hipMemcpyDeviceToHost));
    }
    return MMC_OK;
}
