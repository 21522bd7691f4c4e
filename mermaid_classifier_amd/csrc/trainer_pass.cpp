// trainer_pass.cpp -- the passes of a trainer (include/mmc.h, mmc_trainer_partial_fit*) over host rows or rows of a device-resident
// feature set, one trainer or a group.  A pass checks its arguments and sums every mini-batch's weights on the host before anything is
// uploaded or launched, stages the rows and issues its steps.  HIP runtime API only: the gathers and the step are trainer.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "trainer_state.h"

// wsums[s] = the class-weight sum of mini-batch s (the mean reduction of the weighted CE), whose i-th row carries the label
// ya = y[visit ? visit[i] : i], summed in double in row order (without class weights: the row count, exactly); a mini-batch without
// weight is rejected.  A mixed pass (partner and lam given): position i carries lam w[ya] + oml w[yb] with yb = y[partner[i]] and
// oml = 1.0f - lam[s].  Every pass calls this before it uploads or launches anything, so a rejected pass leaves the weights, the Adam
// moments and the step counter exactly as they were.
static int minibatch_wsums(const char* who, const mmc_trainer* t, const int32_t* y, const int64_t* visit, const int64_t* partner,
                           const float* lam, int64_t n, int mb, std::vector<double>* wsums)
{
    const int steps = (int)((n + mb - 1) / mb);
    wsums->resize(steps);
    for (int s = 0; s < steps; ++s) {
        const int64_t start = (int64_t)s * mb;
        const int cur = batch_rows(n, start, mb);
        const double la = partner ? (double)lam[s] : 1.0, lb = partner ? (double)(1.0f - lam[s]) : 0.0;
        double wsum = 0.0;
        for (int i = 0; i < cur; ++i) {
            const double wa = t->cw ? (double)t->cw_host[y[visit ? visit[start + i] : start + i]] : 1.0;
            if (!partner) { wsum += wa; continue; }
            const double wb = t->cw ? (double)t->cw_host[y[partner[start + i]]] : 1.0;
            wsum += la * wa + lb * wb;
        }
        if (!(wsum > 0.0)) return mmc_fail(MMC_ERR_ARG, "%smini-batch %d has zero total %sclass weight", who, s, partner ? "mixed " : "");
        (*wsums)[s] = wsum;
    }
    return 0;
}

// minibatch_wsums of a weighted pass (include/mmc.h, "group-robust training"): position i carries the mass
// v_i = (double)rw[i] (double)w[y_i] (rw null: 1), summed in double in position order -- into wsums[s] without groups, into
// vmass[s G + rg[i]] with them (wsums[s] is then 1: the loss stage runs with g = 1).  Rejects a weight that is negative or not
// finite, a group outside [0, G), a mini-batch without mass or in which no group has mass.
int minibatch_masses(const char* who, const mmc_trainer* t, const int32_t* y, const int64_t* idx, const float* rw, const int32_t* rg, int G,
                     int64_t n, int mb, std::vector<double>* wsums, std::vector<double>* vmass)
{
    const int steps = (int)((n + mb - 1) / mb);
    for (int64_t i = 0; i < n; ++i) {
        if (rw && !(rw[i] >= 0.f && std::isfinite(rw[i])))
            return mmc_fail(MMC_ERR_ARG, "%srow_weight[%lld] = %g is negative or not finite", who, (long long)i, (double)rw[i]);
        if (rg && (rg[i] < 0 || rg[i] >= G))
            return mmc_fail(MMC_ERR_ARG, "%srow_group[%lld] = %d outside [0, %d)", who, (long long)i, rg[i], G);
    }
    wsums->assign(steps, 1.0);
    if (rg) vmass->assign((size_t)steps * G, 0.0);
    for (int s = 0; s < steps; ++s) {
        const int64_t start = (int64_t)s * mb;
        const int cur = batch_rows(n, start, mb);
        double wsum = 0.0;
        double* V = rg ? vmass->data() + (size_t)s * G : nullptr;
        for (int i = 0; i < cur; ++i) {
            const double w = t->cw ? (double)t->cw_host[y[idx ? idx[start + i] : start + i]] : 1.0;
            const double v = (rw ? (double)rw[start + i] : 1.0) * w;
            if (rg) V[rg[start + i]] += v; else wsum += v;
        }
        if (rg) {
            bool any = false;
            for (int a = 0; a < G; ++a) any = any || V[a] > 0.0;
            if (!any) return mmc_fail(MMC_ERR_ARG, "%sno group of mini-batch %d has mass", who, s);
        } else {
            if (!(wsum > 0.0)) return mmc_fail(MMC_ERR_ARG, "%smini-batch %d has zero total mass", who, s);
            (*wsums)[s] = wsum;
        }
    }
    return 0;
}

// A mini-batch of one row has no variance: a pass of a normalised trainer whose mini-batch, or whose last one, holds fewer than two
// rows is refused where minibatch_wsums refuses, before anything is uploaded or launched.
static int check_bn_minibatches(const char* who, const mmc_trainer* t, int64_t n, int mb)
{
    if (!t->bn) return 0;
    const int64_t last = n - (n - 1) / mb * mb;
    if (mb < 2 || last < 2)
        return mmc_fail(MMC_ERR_ARG, "%sbatch normalisation needs at least 2 rows in every mini-batch: %lld rows in mini-batches of %d leave one of %lld",
                        who, (long long)n, mb, (long long)(mb < 2 ? mb : last));
    return 0;
}

// torch_classifier.py:293-298: sum of loss.item() * mb_size over the steps, over n
static double pass_avg_loss(const std::vector<float>& h, int mb, int64_t n)
{
    double tot = 0.0;
    for (size_t s = 0; s < h.size(); ++s) tot += (double)h[s] * (double)batch_rows(n, (int64_t)s * mb, mb);
    return tot / (double)n;
}

// The pass over host rows.  `order` (n int64 row indices, or NULL = rows are already in visiting order): the shuffle of torch_classifier.py:251-257 applied
// on the device -- the natural-order matrix is uploaded as it is and a gather kernel builds the visiting order (when the
// feature width is a multiple of 4; otherwise, and without `order`, the rows are taken as given).
extern "C" int mmc_trainer_partial_fit_ordered(mmc_trainer* t, const float* X, const int32_t* y, const int64_t* order, int64_t n,
                                               int batch_size, double* avg_loss, void* hip_stream)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!X || !y) return mmc_fail(MMC_ERR_ARG, "X/y is NULL");
    if (n < 1) return mmc_fail(MMC_ERR_ARG, "n = %lld must be positive", (long long)n);
    if (batch_size < 1) return mmc_fail(MMC_ERR_ARG, "batch_size = %d must be positive", batch_size);
    if (order && (t->dims[0] & 3)) return mmc_fail(MMC_ERR_ARG, "device-side ordering needs a feature width that is a multiple of 4 (got %d)", t->dims[0]);
    for (int64_t i = 0; i < n; ++i) {
        if (y[i] < 0 || y[i] >= t->K) return mmc_fail(MMC_ERR_ARG, "label index y[%lld] = %d outside [0, %d)", (long long)i, y[i], t->K);
        if (order && (order[i] < 0 || order[i] >= n)) return mmc_fail(MMC_ERR_ARG, "order[%lld] = %lld outside [0, %lld)", (long long)i, (long long)order[i], (long long)n);
    }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(t->device));
    const int mb = (int)(batch_size < n ? batch_size : n);
    std::vector<double> wsums;
    int r = check_bn_minibatches("", t, n, mb);
    if (r) return r;
    if ((r = minibatch_wsums("", t, y, order, nullptr, nullptr, n, mb, &wsums))) return r;
    const int steps = (int)wsums.size();
    if ((r = trainer_reserve(t, n, mb, steps))) return r;
    if (order) {
        if ((r = t->Xn.reserve(n * t->dims[0])) || (r = t->yn.reserve(n)) || (r = t->order.reserve(n))) return r;
        HIP_TRY(hipMemcpyAsync(t->Xn, X, (size_t)n * t->dims[0] * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(t->yn, y, (size_t)n * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(t->order, order, (size_t)n * 8, hipMemcpyHostToDevice, st));
        gather_ordered(t, n, st);
    } else {
        HIP_TRY(hipMemcpyAsync(t->X, X, (size_t)n * t->dims[0] * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(t->y, y, (size_t)n * 4, hipMemcpyHostToDevice, st));
    }
    for (int s = 0; s < steps; ++s) {
        const int64_t start = (int64_t)s * mb;
        const StepMember one{t, start, batch_rows(n, start, mb), (float)(1.0 / wsums[s]), s, false, 0.f};
        if ((r = trainer_group_step(&one, 1, st))) return r;
    }
    t->gnorm_steps = t->max_norm > 0.0 ? steps : 0;
    std::vector<float> h(steps);
    HIP_TRY(hipMemcpyAsync(h.data(), t->losses, (size_t)steps * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (avg_loss) *avg_loss = pass_avg_loss(h, mb, n);
    return MMC_OK;
}

extern "C" int mmc_trainer_partial_fit(mmc_trainer* t, const float* X, const int32_t* y, int64_t n, int batch_size, double* avg_loss,
                                       void* hip_stream)
{
    return mmc_trainer_partial_fit_ordered(t, X, y, nullptr, n, batch_size, avg_loss, hip_stream);
}

// ---- passes over a resident feature set -----------------------------------------------------------------------------------
namespace {

// how one trainer takes one pass over rows of a set: mini-batch, steps, its chunks of whole mini-batches, every step's weight sum
struct SetPass {
    mmc_trainer* t = nullptr;
    const int64_t* visit = nullptr;
    const int64_t* partner = nullptr;   // a mixed pass: partner rows and one lam per mini-batch (both or neither)
    const float* lam = nullptr;
    const float* row_weight = nullptr;  // a weighted pass: either or both, by position
    const int32_t* row_group = nullptr;
    const mmc_targetset* targets = nullptr;   // a distilled pass: position i reads target row visit ? visit[i] : i in place
    int64_t n = 0;
    int mb = 0, steps = 0;
    int64_t chunk = 0, steps_per_chunk = 0, stage_rows = 0;
    std::vector<double> wsums;
    std::vector<double> vmass;          // [steps][n_groups] of a pass with groups
};

// `who` prefixes the message: "" for the solo call, "member 3: " for a member of a group
int check_set_pass(const char* who, const mmc_trainer* t, const mmc_featureset* fs, const int64_t* visit, int64_t n, int batch_size)
{
    if (fs->dim != t->dims[0]) return mmc_fail(MMC_ERR_ARG, "%sfeature set has %d columns, trainer expects %d", who, fs->dim, t->dims[0]);
    if (fs->K != t->K) return mmc_fail(MMC_ERR_ARG, "%sfeature set has %d classes, trainer %d", who, fs->K, t->K);
    if (fs->device != t->device) return mmc_fail(MMC_ERR_ARG, "%sfeature set is on device %d, trainer on device %d", who, fs->device, t->device);
    if (n < 1) return mmc_fail(MMC_ERR_ARG, "%sn = %lld must be positive", who, (long long)n);
    if (batch_size < 1) return mmc_fail(MMC_ERR_ARG, "%sbatch_size = %d must be positive", who, batch_size);
    if (!visit && n != fs->n) return mmc_fail(MMC_ERR_ARG, "%swithout a visiting order n must be the set's %lld rows (got %lld)", who, (long long)fs->n, (long long)n);
    if (visit)
        for (int64_t i = 0; i < n; ++i)
            if (visit[i] < 0 || visit[i] >= fs->n)
                return mmc_fail(MMC_ERR_ARG, "%svisit[%lld] = %lld outside [0, %lld)", who, (long long)i, (long long)visit[i], (long long)fs->n);
    return 0;
}

// the targets of a distilled pass against its trainer and its feature set (include/mmc.h, "distillation"); no entry point takes
// targets and a mixing plan, so mixup with targets needs no check here
int check_targets(const char* who, const mmc_trainer* t, const mmc_featureset* fs, const mmc_targetset* ts)
{
    if (!ts) return 0;
    if (t->distill_alpha == 0.0) return mmc_fail(MMC_ERR_ARG, "%stargets: the trainer needs mmc_trainer_set_distillation(alpha > 0)", who);
    if (t->hier) return mmc_fail(MMC_ERR_ARG, "%sa distilled pass takes no hierarchy (mmc_trainer_set_hierarchy)", who);
    if (ts->K != t->K) return mmc_fail(MMC_ERR_ARG, "%starget set has %d classes, trainer %d", who, ts->K, t->K);
    if (ts->n != fs->n) return mmc_fail(MMC_ERR_ARG, "%starget set has %lld rows, feature set %lld", who, (long long)ts->n, (long long)fs->n);
    if (ts->device != t->device) return mmc_fail(MMC_ERR_ARG, "%starget set is on device %d, trainer on device %d", who, ts->device, t->device);
    return 0;
}

// the plan of a mixed pass: both arrays or neither, every partner a row of the set, every lam in [0, 1]
int check_mix_plan(const char* who, const mmc_featureset* fs, const int64_t* partner, const float* lam, int64_t n, int batch_size)
{
    if (!partner && !lam) return 0;
    if (!partner || !lam) return mmc_fail(MMC_ERR_ARG, "%spartner and lam go together: only %s was given", who, partner ? "partner" : "lam");
    for (int64_t i = 0; i < n; ++i)
        if (partner[i] < 0 || partner[i] >= fs->n)
            return mmc_fail(MMC_ERR_ARG, "%spartner[%lld] = %lld outside [0, %lld)", who, (long long)i, (long long)partner[i], (long long)fs->n);
    const int64_t mb = batch_size < n ? batch_size : n, steps = (n + mb - 1) / mb;
    for (int64_t s = 0; s < steps; ++s)
        if (!(lam[s] >= 0.f && lam[s] <= 1.f)) return mmc_fail(MMC_ERR_ARG, "%slam[%lld] = %g outside [0, 1]", who, (long long)s, (double)lam[s]);
    return 0;
}

int train_chunk_bound(int64_t* bound)
{
    *bound = MMC_TRAIN_CHUNK_ROWS_DEFAULT;
    if (const char* env = std::getenv("MMC_TRAIN_CHUNK_ROWS")) {
        char* end = nullptr;
        const long long v = std::strtoll(env, &end, 10);
        if (end == env || *end || v < 1) return mmc_fail(MMC_ERR_ARG, "MMC_TRAIN_CHUNK_ROWS = '%s' is not a positive integer", env);
        *bound = v;
    }
    return 0;
}

int plan_set_pass(const char* who, mmc_trainer* t, const mmc_featureset* fs, const int64_t* visit, const int64_t* partner,
                  const float* lam, const float* row_weight, const int32_t* row_group, int64_t n, int batch_size, int64_t bound, SetPass* p)
{
    const int mb = (int)(batch_size < n ? batch_size : n);
    if ((n + mb - 1) / mb > (int64_t)1 << 30) return mmc_fail(MMC_ERR_ARG, "%s%lld rows in mini-batches of %d: too many steps for one pass", who, (long long)n, mb);
    p->t = t; p->visit = visit; p->partner = partner; p->lam = lam; p->n = n;
    p->row_weight = row_weight; p->row_group = row_group;
    p->mb = mb;
    p->steps = (int)((n + mb - 1) / mb);
    // the largest multiple of the mini-batch not above the bound, at least one mini-batch, and no more than a gather's grid / `rows` hold
    int64_t chunk = bound / mb * mb;
    if (chunk < mb) chunk = mb;
    const int64_t chunk_max = ((int64_t)1 << 30) / mb * mb;
    if (chunk > chunk_max) chunk = chunk_max;
    p->chunk = chunk;
    p->steps_per_chunk = chunk / mb;
    p->stage_rows = chunk < n ? chunk : n;
    if (row_weight || row_group)   // (never with a partner: set_pass has refused that)
        return minibatch_masses(who, t, fs->y_host.data(), visit, row_weight, row_group, t->n_groups, n, mb, &p->wsums, &p->vmass);
    return minibatch_wsums(who, t, fs->y_host.data(), visit, partner, lam, n, mb, &p->wsums);
}

// the trainer's staging, activations and loss slots for the pass, and its device copy of the visiting order (not yet uploaded)
int reserve_set_pass(const SetPass& p)
{
    mmc_trainer* t = p.t;
    int r = trainer_reserve(t, p.stage_rows, p.mb, p.steps);
    if (r) return r;
    if (p.visit && (r = t->visit.reserve(p.n))) return r;
    if (p.partner && ((r = t->y2.reserve(p.stage_rows)) || (r = t->partner.reserve(p.n)) || (r = t->lam.reserve(p.steps)))) return r;
    if (p.row_weight && (r = t->row_w.reserve(p.n))) return r;
    if (p.row_group && ((r = t->row_g.reserve(p.n)) || (r = t->group_mass.reserve((int64_t)p.steps * t->n_groups)) || (r = t->row_scale.reserve(p.mb))))
        return r;
    return 0;
}

// One pass of `count` trainers over rows of `fs`, step s of every member's pass issued together: position i of member m visits row
// visit[m][i].  Nothing but the visiting orders is uploaded.  A member's visited rows and labels are gathered into its mini-batch
// staging (t->X / t->y) a chunk of whole mini-batches at a time, and that chunk's steps follow on the same stream, so the steps
// run the kernels of the host-fed pass on the same values: same bits.  `grouped` is the entry point's way of naming a member and of
// reporting a failed reservation; the solo entry is a group of one that names nobody.
int set_pass(bool grouped, mmc_trainer* const* trainers, int count, mmc_featureset* fs, const int64_t* const* visit,
             const int64_t* const* partner, const float* const* lam, const float* const* row_weight, const int32_t* const* row_group,
             const mmc_targetset* const* targets, const int64_t* n, const int* batch_size, double* avg_loss, hipStream_t st)
{
    std::vector<SetPass> mem(count);
    char who[MMC_TRAINER_GROUP_MAX][32];
    int r = 0;
    for (int m = 0; m < count; ++m) {
        who[m][0] = 0;
        if (grouped) std::snprintf(who[m], sizeof who[m], "member %d: ", m);
        if ((r = check_set_pass(who[m], trainers[m], fs, visit[m], n[m], batch_size[m]))) return r;
        if ((r = check_mix_plan(who[m], fs, partner ? partner[m] : nullptr, lam ? lam[m] : nullptr, n[m], batch_size[m]))) return r;
        if ((r = check_bn_minibatches(who[m], trainers[m], n[m], (int)(batch_size[m] < n[m] ? batch_size[m] : n[m])))) return r;
        const bool weighted = (row_weight && row_weight[m]) || (row_group && row_group[m]);
        if (weighted && partner && partner[m]) return mmc_fail(MMC_ERR_ARG, "%sa mixed pass takes no row weights or groups", who[m]);
        if (partner && partner[m] && trainers[m]->hier)
            return mmc_fail(MMC_ERR_ARG, "%sa mixed pass takes no hierarchy (mmc_trainer_set_hierarchy)", who[m]);
        if (row_group && row_group[m] && !trainers[m]->n_groups)
            return mmc_fail(MMC_ERR_ARG, "%srow_group needs mmc_trainer_set_group_dro(n_groups > 0) on the trainer", who[m]);
        if ((r = check_targets(who[m], trainers[m], fs, targets ? targets[m] : nullptr))) return r;
    }
    int64_t bound = 0;
    if ((r = train_chunk_bound(&bound))) return r;
    int max_steps = 0;
    for (int m = 0; m < count; ++m) {
        if ((r = plan_set_pass(who[m], trainers[m], fs, visit[m], partner ? partner[m] : nullptr, lam ? lam[m] : nullptr,
                               row_weight ? row_weight[m] : nullptr, row_group ? row_group[m] : nullptr, n[m], batch_size[m], bound, &mem[m])))
            return r;
        mem[m].targets = targets ? targets[m] : nullptr;
        max_steps = std::max(max_steps, mem[m].steps);
    }
    HIP_TRY(hipSetDevice(fs->device));
    // every member's buffers before the first launch: a pass that cannot be staged changes no member
    for (int m = 0; m < count; ++m)
        if ((r = reserve_set_pass(mem[m]))) {
            if (!grouped) return r;
            (void)hipGetLastError();
            return mmc_fail(MMC_ERR_NOMEM, "member %d: could not allocate the buffers of its pass (%lld staged rows, mini-batch %d)", m,
                            (long long)mem[m].stage_rows, mem[m].mb);
        }
    for (int m = 0; m < count; ++m)
        if (mem[m].visit) HIP_TRY(hipMemcpyAsync(mem[m].t->visit, mem[m].visit, (size_t)mem[m].n * 8, hipMemcpyHostToDevice, st));
    for (int m = 0; m < count; ++m)
        if (mem[m].partner) {
            HIP_TRY(hipMemcpyAsync(mem[m].t->partner, mem[m].partner, (size_t)mem[m].n * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(mem[m].t->lam, mem[m].lam, (size_t)mem[m].steps * 4, hipMemcpyHostToDevice, st));
        }
    for (int m = 0; m < count; ++m) {
        const SetPass& p = mem[m];
        if (p.row_weight) HIP_TRY(hipMemcpyAsync(p.t->row_w, p.row_weight, (size_t)p.n * 4, hipMemcpyHostToDevice, st));
        if (p.row_group) {
            HIP_TRY(hipMemcpyAsync(p.t->row_g, p.row_group, (size_t)p.n * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(p.t->group_mass, p.vmass.data(), p.vmass.size() * 8, hipMemcpyHostToDevice, st));
        }
    }
    StepMember act[MMC_TRAINER_GROUP_MAX];
    for (int s = 0; s < max_steps; ++s) {
        int cnt = 0;
        for (int m = 0; m < count; ++m) {
            const SetPass& p = mem[m];
            if (s >= p.steps) continue;   // this member's pass is over
            const int64_t start = (int64_t)s * p.mb, c0 = s / p.steps_per_chunk * p.chunk;
            if (start == c0) {            // its first step of a chunk: stage the chunk's rows first
                const int rows = (int)((p.n - c0) < p.chunk ? (p.n - c0) : p.chunk);
                if ((r = gather_chunk(p.t, fs, p.visit != nullptr, p.partner != nullptr, p.mb, c0, rows, st))) return r;
            }
            act[cnt] = StepMember{p.t, start - c0, batch_rows(p.n, start, p.mb), (float)(1.0 / p.wsums[s]), s, p.partner != nullptr,
                                  p.partner ? p.lam[s] : 0.f};
            if (p.row_weight || p.row_group) {   // the pass's arrays are indexed by position of the pass, not of the chunk
                act[cnt].weighted = true;
                act[cnt].rw = p.row_weight ? p.t->row_w + start : nullptr;
                act[cnt].rg = p.row_group ? p.t->row_g + start : nullptr;
                act[cnt].V = p.row_group ? p.t->group_mass + (size_t)s * p.t->n_groups : nullptr;
            }
            if (p.targets) {   // read in place by position of the pass, through the order the pass has uploaded
                act[cnt].q = p.targets->P;
                act[cnt].q_visit = p.visit ? p.t->visit.p : nullptr;
                act[cnt].q_start = start;
            }
            ++cnt;
        }
        if ((r = trainer_group_step(act, cnt, st))) return r;
    }
    for (int m = 0; m < count; ++m) mem[m].t->gnorm_steps = mem[m].t->max_norm > 0.0 ? mem[m].steps : 0;
    std::vector<std::vector<float>> h(count);
    for (int m = 0; m < count; ++m) {
        h[m].resize(mem[m].steps);
        HIP_TRY(hipMemcpyAsync(h[m].data(), mem[m].t->losses, (size_t)mem[m].steps * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (avg_loss)
        for (int m = 0; m < count; ++m) avg_loss[m] = pass_avg_loss(h[m], mem[m].mb, mem[m].n);
    return MMC_OK;
}

// what both grouped entry points ask of their arguments before the members are looked at; a refused call reports zero losses
int check_group_args(mmc_trainer* const* trainers, int count, const mmc_featureset* fs, const int64_t* const* visit, const int64_t* n,
                     const int* batch_size, double* avg_loss)
{
    if (avg_loss && count >= 1 && count <= MMC_TRAINER_GROUP_MAX)
        for (int m = 0; m < count; ++m) avg_loss[m] = 0.0;
    if (!trainers || !visit || !n || !batch_size) return mmc_fail(MMC_ERR_ARG, "trainers / visit / n / batch_size is NULL");
    if (count < 1 || count > MMC_TRAINER_GROUP_MAX) return mmc_fail(MMC_ERR_ARG, "count = %d outside [1, %d]", count, MMC_TRAINER_GROUP_MAX);
    for (int m = 0; m < count; ++m) {
        if (!trainers[m]) return mmc_fail(MMC_ERR_ARG, "member %d: trainer handle is NULL", m);
        for (int o = 0; o < m; ++o)
            if (trainers[o] == trainers[m]) return mmc_fail(MMC_ERR_ARG, "member %d is the same trainer as member %d", m, o);
    }
    if (!fs) return mmc_fail(MMC_ERR_ARG, "feature set handle is NULL");
    return 0;
}

// the solo entry points: a group of one; an array a pass does not take is null
int solo_pass(mmc_trainer* t, mmc_featureset* fs, const int64_t* visit, const int64_t* partner, const float* lam, const float* row_weight,
              const int32_t* row_group, int64_t n, int batch_size, double* avg_loss, void* hip_stream, const mmc_targetset* targets = nullptr)
{
    if (!t) return mmc_fail(MMC_ERR_ARG, "trainer handle is NULL");
    if (!fs) return mmc_fail(MMC_ERR_ARG, "feature set handle is NULL");
    return set_pass(false, &t, 1, fs, &visit, &partner, &lam, &row_weight, &row_group, &targets, &n, &batch_size, avg_loss,
                    static_cast<hipStream_t>(hip_stream));
}

}  // namespace

// The pass of mmc_trainer_partial_fit_ordered over rows that are already on the device: a group of one (include/mmc.h).
extern "C" int mmc_trainer_partial_fit_set(mmc_trainer* t, mmc_featureset* fs, const int64_t* visit, int64_t n, int batch_size,
                                           double* avg_loss, void* hip_stream)
{
    return solo_pass(t, fs, visit, nullptr, nullptr, nullptr, nullptr, n, batch_size, avg_loss, hip_stream);
}

// mmc_trainer_partial_fit_set on mixed rows (include/mmc.h, "regularisers"); NULL partner and lam: that call itself.
extern "C" int mmc_trainer_partial_fit_set_mixed(mmc_trainer* t, mmc_featureset* fs, const int64_t* visit, const int64_t* partner,
                                                 const float* lam, int64_t n, int batch_size, double* avg_loss, void* hip_stream)
{
    return solo_pass(t, fs, visit, partner, lam, nullptr, nullptr, n, batch_size, avg_loss, hip_stream);
}

// mmc_trainer_partial_fit_set for `count` trainers over one set in the launches of one pass (include/mmc.h).
extern "C" int mmc_trainer_group_partial_fit_set(mmc_trainer* const* trainers, int count, mmc_featureset* fs, const int64_t* const* visit,
                                                 const int64_t* n, const int* batch_size, double* avg_loss, void* hip_stream)
{
    return mmc_trainer_group_partial_fit_set_mixed(trainers, count, fs, visit, nullptr, nullptr, n, batch_size, avg_loss, hip_stream);
}

// The grouped pass with a mixing plan per member (include/mmc.h, "regularisers"): partner / lam are arrays of `count` pointers, or
// NULL for a pass in which nobody is mixed; a member whose two entries are NULL is not mixed.
extern "C" int mmc_trainer_group_partial_fit_set_mixed(mmc_trainer* const* trainers, int count, mmc_featureset* fs,
                                                       const int64_t* const* visit, const int64_t* const* partner, const float* const* lam,
                                                       const int64_t* n, const int* batch_size, double* avg_loss, void* hip_stream)
{
    if (int r = check_group_args(trainers, count, fs, visit, n, batch_size, avg_loss)) return r;
    if (!partner != !lam) return mmc_fail(MMC_ERR_ARG, "partner and lam go together: only %s was given", partner ? "partner" : "lam");
    return set_pass(true, trainers, count, fs, visit, partner, lam, nullptr, nullptr, nullptr, n, batch_size, avg_loss,
                    static_cast<hipStream_t>(hip_stream));
}

// mmc_trainer_partial_fit_set with per-row weights and / or groups (include/mmc.h, "group-robust training"); both NULL: that call.
extern "C" int mmc_trainer_partial_fit_set_weighted(mmc_trainer* t, mmc_featureset* fs, const int64_t* visit, const float* row_weight,
                                                    const int32_t* row_group, int64_t n, int batch_size, double* avg_loss, void* hip_stream)
{
    return solo_pass(t, fs, visit, nullptr, nullptr, row_weight, row_group, n, batch_size, avg_loss, hip_stream);
}

// The grouped pass with weights and groups per member: arrays of `count` pointers, or NULL; a member whose two entries are NULL
// takes the plain kernels.
extern "C" int mmc_trainer_group_partial_fit_set_weighted(mmc_trainer* const* trainers, int count, mmc_featureset* fs,
                                                          const int64_t* const* visit, const float* const* row_weight,
                                                          const int32_t* const* row_group, const int64_t* n, const int* batch_size,
                                                          double* avg_loss, void* hip_stream)
{
    if (int r = check_group_args(trainers, count, fs, visit, n, batch_size, avg_loss)) return r;
    return set_pass(true, trainers, count, fs, visit, nullptr, nullptr, row_weight, row_group, nullptr, n, batch_size, avg_loss,
                    static_cast<hipStream_t>(hip_stream));
}

// mmc_trainer_partial_fit_set_weighted with per-row soft targets (include/mmc.h, "distillation"); ts NULL: that call.
extern "C" int mmc_trainer_partial_fit_set_distill(mmc_trainer* t, mmc_featureset* fs, mmc_targetset* ts, const int64_t* visit,
                                                   const float* row_weight, const int32_t* row_group, int64_t n, int batch_size,
                                                   double* avg_loss, void* hip_stream)
{
    return solo_pass(t, fs, visit, nullptr, nullptr, row_weight, row_group, n, batch_size, avg_loss, hip_stream, ts);
}

// The grouped pass with a target set per member: `targets` is an array of `count` pointers, or NULL; a member whose entry is NULL
// runs as in mmc_trainer_group_partial_fit_set_weighted.  Members may share one set: it is only read.
extern "C" int mmc_trainer_group_partial_fit_set_distill(mmc_trainer* const* trainers, int count, mmc_featureset* fs,
                                                         mmc_targetset* const* targets, const int64_t* const* visit,
                                                         const float* const* row_weight, const int32_t* const* row_group, const int64_t* n,
                                                         const int* batch_size, double* avg_loss, void* hip_stream)
{
    if (int r = check_group_args(trainers, count, fs, visit, n, batch_size, avg_loss)) return r;
    return set_pass(true, trainers, count, fs, visit, nullptr, nullptr, row_weight, row_group, targets, n, batch_size, avg_loss,
                    static_cast<hipStream_t>(hip_stream));
}
