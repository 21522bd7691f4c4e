// mmc_ensemble.cpp -- head ensembles of the C ABI (include/mmc.h, "head ensembles"): M calibrated heads on one class list scored
// together.  The Linear layers of all members run as one launch per layer index (launch_mlp_group), their logits land in one
// [M][rows][K] buffer, and one kernel forms the mean of the calibrated probabilities, its top-k (or its validation tables) and the
// per-point entropies and votes.  The members are borrowed mmc_head handles: only their device weights and Platt parameters are
// read; the activations, logits and staging buffers are the ensemble's own.
// Host C++ only; the kernels are launched through kernels.h.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "api_internal.h"
#include "head_internal.h"
#include "kernels.h"
#include "trainer_internal.h"

static_assert(MMC_ENSEMBLE_MAX == ENSEMBLE_MAX && MMC_ENSEMBLE_MAX_CLASSES == ENSEMBLE_MAX_K && MMC_ENSEMBLE_STATS == ENSEMBLE_STATS,
              "include/mmc.h and kernels.h disagree on the ensembles");

struct mmc_ensemble {
    int device = 0, M = 0, K = 0, input_dim = 0, in_pad = 0;
    int max_layers = 0;   // of the deepest member
    int wh = 0;           // the widest (padded) hidden layer of any member; 0 when every member is one Linear layer
    std::vector<mmc_head*> members;
    EnsembleCal cal{};
    // one chunk: the padded input rows, the members' ping-pong activations [2][M][rows][wh] and logits [M][rows][K]
    DevBuf<float> in_stage, act, logits;
    // MMC_OUT_HOST staging of one chunk's outputs (evaluate: always), and mmc_ensemble_classify_patches' feature rows
    DevBuf<float> proba_stage, stats_stage, score_stage, cls_feats;
    DevBuf<int32_t> idx_stage, votes_stage;
    // mmc_ensemble_evaluate*: one chunk's labels and per-row outputs ([5][rows] dwords), the label map, the int64 tables
    DevBuf<int32_t> eval_rows, eval_map;
    DevBuf<long long> eval_tot;
};

extern "C" void mmc_ensemble_destroy(mmc_ensemble* e)
{
    if (!e) return;
    hipSetDevice(e->device);
    delete e;
}

extern "C" int mmc_ensemble_create(mmc_head* const* members, int count, mmc_ensemble** out)
{
    if (!out) return fail(MMC_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!members) return fail(MMC_ERR_ARG, "members is NULL");
    if (count < 1 || count > ENSEMBLE_MAX) return fail(MMC_ERR_ARG, "count = %d members outside [1, %d]", count, ENSEMBLE_MAX);
    for (int j = 0; j < count; ++j)
        if (!members[j]) return fail(MMC_ERR_ARG, "member %d is NULL", j);
    const mmc_head* h0 = members[0];
    for (int j = 1; j < count; ++j) {
        const mmc_head* h = members[j];
        if (h->K != h0->K) return fail(MMC_ERR_ARG, "member %d has %d classes, member 0 has %d", j, h->K, h0->K);
        if (h->input_dim != h0->input_dim) return fail(MMC_ERR_ARG, "member %d has input_dim %d, member 0 has %d", j, h->input_dim, h0->input_dim);
        if (h->device != h0->device) return fail(MMC_ERR_ARG, "member %d lives on device %d, member 0 on device %d", j, h->device, h0->device);
    }
    if (h0->K > ENSEMBLE_MAX_K) return fail(MMC_ERR_ARG, "K = %d classes: an ensemble takes at most %d", h0->K, ENSEMBLE_MAX_K);
    mmc_ensemble* e = new mmc_ensemble();
    e->device = h0->device; e->M = count; e->K = h0->K; e->input_dim = h0->input_dim; e->in_pad = h0->in_pad;
    e->members.assign(members, members + count);
    for (int j = 0; j < count; ++j) {
        const mmc_head* h = members[j];
        e->cal.a[j] = h->a.p;
        e->cal.b[j] = h->bc.p;
        e->max_layers = h->n_layers > e->max_layers ? h->n_layers : e->max_layers;
        for (int l = 1; l < h->n_layers; ++l) e->wh = h->dims_pad[l] > e->wh ? h->dims_pad[l] : e->wh;
    }
    *out = e;
    return MMC_OK;
}

extern "C" int mmc_ensemble_size(const mmc_ensemble* e) { return e ? e->M : 0; }
extern "C" int mmc_ensemble_num_classes(const mmc_ensemble* e) { return e ? e->K : 0; }
extern "C" int mmc_ensemble_input_dim(const mmc_ensemble* e) { return e ? e->input_dim : 0; }

// rows per chunk: the largest multiple of G with M x rows inside one head's HEAD_CHUNK rows (never less than one point)
static int64_t ensemble_chunk(const mmc_ensemble* e, int G)
{
    const int64_t pts = HEAD_CHUNK / e->M / G;
    return (pts < 1 ? 1 : pts) * G;
}
extern "C" int mmc_ensemble_chunk_rows(const mmc_ensemble* e, int G)
{
    if (!e || G < 1 || G > VIEWS_MAX) return 0;
    return (int)ensemble_chunk(e, G);
}

// the Linear layers of one chunk: per layer index one launch over the members that have that layer; member j's logits (cur x K)
// end at e->logits + j * cur * K
static int ensemble_logits(mmc_ensemble* e, const float* x, int cur, unsigned flags, hipStream_t st)
{
    const hipMemcpyKind kin = (flags & MMC_IN_HOST) ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    if ((flags & MMC_IN_HOST) || e->in_pad != e->input_dim) {
        if (e->in_pad != e->input_dim) HIP_TRY(hipMemsetAsync(e->in_stage.p, 0, (size_t)cur * e->in_pad * 4, st));
        HIP_TRY(hipMemcpy2DAsync(e->in_stage.p, (size_t)e->in_pad * 4, x, (size_t)e->input_dim * 4, (size_t)e->input_dim * 4, cur, kin, st));
        x = e->in_stage.p;
    }
    auto slot = [&](int p, int j) { return e->act.p + (size_t)(p * e->M + j) * cur * e->wh; };
    for (int l = 0; l < e->max_layers; ++l) {
        MlpGroupArgs g{};
        g.M = cur;
        int cnt = 0;
        for (int j = 0; j < e->M; ++j) {
            const mmc_head* h = e->members[j];
            if (l >= h->n_layers) continue;
            const bool last = l == h->n_layers - 1;
            MlpGroupMember& m = g.m[cnt++];
            m.X = l == 0 ? x : slot((l - 1) & 1, j);
            m.W = h->W[l].p;
            m.bias = h->b[l].p;
            m.Y = last ? e->logits.p + (size_t)j * cur * e->K : slot(l & 1, j);
            m.K = h->dims_pad[l];
            m.N = h->dims_pad[l + 1];
            m.relu = last ? 0 : 1;
        }
        KTRY(launch_mlp_group(g, cnt, st));
    }
    return 0;
}

// the one chunk loop: rows [0, n) of x in chunks of `chunk`; per chunk it grows the buffers, runs the Linear layers and calls
// each(offset, rows), which enqueues what its entry point does with e->logits (member stride rows x K)
template <class F>
static int ensemble_for_chunks(mmc_ensemble* e, const float* x, int64_t n, int64_t chunk, unsigned flags, hipStream_t st, F each)
{
    for (int64_t off = 0; off < n; off += chunk) {
        const int cur = (int)((n - off) < chunk ? (n - off) : chunk);
        int r;
        if ((r = e->in_stage.reserve((int64_t)cur * e->in_pad)) || (r = e->act.reserve((int64_t)2 * e->M * cur * e->wh)) ||
            (r = e->logits.reserve((int64_t)e->M * cur * e->K)))
            return r;
        if ((r = ensemble_logits(e, x + (size_t)off * e->input_dim, cur, flags, st))) return r;
        if ((r = each(off, cur))) return r;
    }
    return MMC_OK;
}

static int topk_check(const mmc_ensemble* e, int64_t n_points, int G, int k)
{
    if (!e) return fail(MMC_ERR_ARG, "ensemble handle is NULL");
    if (G < 1 || G > VIEWS_MAX) return fail(MMC_ERR_ARG, "G = %d views per point is outside [1, %d]", G, VIEWS_MAX);
    if (n_points < 0) return fail(MMC_ERR_ARG, "n_points = %lld is negative", (long long)n_points);
    if (k < 1 || k > e->K) return fail(MMC_ERR_ARG, "k = %d is outside [1, %d] (the ensemble has %d classes)", k, e->K, e->K);
    return MMC_OK;
}

extern "C" int mmc_ensemble_topk(mmc_ensemble* e, const float* feats, int64_t n_points, int G, int k, int32_t* idx, float* scores,
                                 float* proba, float* stats, int32_t* votes, unsigned flags, void* hip_stream)
{
    if (int r = topk_check(e, n_points, G, k)) return r;
    if (n_points == 0) return MMC_OK;
    if (!feats) return fail(MMC_ERR_ARG, "feats is NULL");
    if (!idx || !scores) return fail(MMC_ERR_ARG, "idx/scores is NULL");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(e->device));
    const bool out_host = (flags & MMC_OUT_HOST) != 0;
    const int64_t chunk = ensemble_chunk(e, G);
    const int K = e->K;
    if (out_host) {   // the first chunk is the largest: staging that holds it holds every later one
        const int64_t pts = n_points < chunk / G ? n_points : chunk / G;
        int r;
        if ((r = e->idx_stage.reserve(pts * k)) || (r = e->score_stage.reserve(pts * k)) || (proba && (r = e->proba_stage.reserve(pts * K))) ||
            (stats && (r = e->stats_stage.reserve(pts * ENSEMBLE_STATS))) || (votes && (r = e->votes_stage.reserve(pts))))
            return r;
    }
    return ensemble_for_chunks(e, feats, n_points * G, chunk, flags, st, [&](int64_t off, int cur) -> int {
        const int64_t p0 = off / G;
        const int pts = cur / G;
        int32_t* iout = out_host ? e->idx_stage.p : idx + (size_t)p0 * k;
        float* sout = out_host ? e->score_stage.p : scores + (size_t)p0 * k;
        float* pout = proba ? (out_host ? e->proba_stage.p : proba + (size_t)p0 * K) : nullptr;
        float* tout = stats ? (out_host ? e->stats_stage.p : stats + (size_t)p0 * ENSEMBLE_STATS) : nullptr;
        int32_t* vout = votes ? (out_host ? e->votes_stage.p : votes + p0) : nullptr;
        KTRY(launch_ensemble_topk(e->logits.p, pts, G, K, e->M, (size_t)cur * K, e->cal, k, iout, sout, pout, tout, vout, st));
        if (out_host) {
            HIP_TRY(hipMemcpyAsync(idx + (size_t)p0 * k, iout, (size_t)pts * k * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(scores + (size_t)p0 * k, sout, (size_t)pts * k * 4, hipMemcpyDeviceToHost, st));
            if (proba) HIP_TRY(hipMemcpyAsync(proba + (size_t)p0 * K, pout, (size_t)pts * K * 4, hipMemcpyDeviceToHost, st));
            if (stats) HIP_TRY(hipMemcpyAsync(stats + (size_t)p0 * ENSEMBLE_STATS, tout, (size_t)pts * ENSEMBLE_STATS * 4, hipMemcpyDeviceToHost, st));
            if (votes) HIP_TRY(hipMemcpyAsync(votes + p0, vout, (size_t)pts * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        return MMC_OK;
    });
}

extern "C" int mmc_ensemble_classify_patches(mmc_backbone* bb, mmc_ensemble* e, const void* patches, int64_t n_points, int G, int k,
                                             int32_t* idx, float* scores, float* stats, int32_t* votes, unsigned flags, void* hip_stream)
{
    if (!bb) return fail(MMC_ERR_ARG, "backbone handle is NULL");
    if (int r = topk_check(e, n_points, G, k)) return r;
    if (mmc_backbone_device(bb) != e->device)
        return fail(MMC_ERR_ARG, "backbone lives on device %d, ensemble on device %d", mmc_backbone_device(bb), e->device);
    if (mmc_feature_dim(bb) != e->input_dim)
        return fail(MMC_ERR_ARG, "backbone feature_dim %d != ensemble input_dim %d", mmc_feature_dim(bb), e->input_dim);
    if (n_points == 0) return MMC_OK;
    if (!patches) return fail(MMC_ERR_ARG, "patches is NULL");
    if (!idx || !scores) return fail(MMC_ERR_ARG, "idx/scores is NULL");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(e->device));
    const int64_t chunk = CLASSIFY_CHUNK / G * G, n = n_points * G;   // patches: whole points only
    int r = e->cls_feats.reserve((n < chunk ? n : chunk) * e->input_dim);
    if (r) return r;
    const size_t psz = (size_t)MMC_PATCH * MMC_PATCH * 3;
    const uint8_t* in = static_cast<const uint8_t*>(patches);
    for (int64_t off = 0; off < n; off += chunk) {
        const int64_t cur = (n - off) < chunk ? (n - off) : chunk, p0 = off / G;
        if ((r = mmc_backbone_extract(bb, in + (size_t)off * psz, cur, e->cls_feats.p, flags & MMC_IN_HOST, st))) return r;
        if ((r = mmc_ensemble_topk(e, e->cls_feats.p, cur / G, G, k, idx + (size_t)p0 * k, scores + (size_t)p0 * k, nullptr,
                                   stats ? stats + (size_t)p0 * ENSEMBLE_STATS : nullptr, votes ? votes + p0 : nullptr,
                                   flags & MMC_OUT_HOST, st)))
            return r;
    }
    return MMC_OK;
}

// ------------------------------------------------------------------------------------------
// validation of an ensemble: mmc_ensemble_evaluate / mmc_ensemble_evaluate_set (the contract of mmc_head_evaluate*)
// ------------------------------------------------------------------------------------------
struct EnsEvalOut {
    int32_t* est; float* score; int32_t* rank; float* p_true; float* stats; int32_t* votes;
    int64_t* totals; int64_t* confusion; int64_t* rank_hist;
};

static int ens_eval_check(const mmc_ensemble* e, int64_t n, const int32_t* label_map, int n_labels, const EnsEvalOut& o)
{
    if (!e) return fail(MMC_ERR_ARG, "ensemble handle is NULL");
    if (n < 0) return fail(MMC_ERR_ARG, "n = %lld is negative", (long long)n);
    if (!o.totals) return fail(MMC_ERR_ARG, "totals is NULL");
    if (n > MMC_EVALUATE_SET_MAX_ROWS)
        return fail(MMC_ERR_ARG, "n = %lld rows in one call: split it (at most %lld)", (long long)n, (long long)MMC_EVALUATE_SET_MAX_ROWS);
    if (!label_map && n_labels != 0) return fail(MMC_ERR_ARG, "n_labels = %d without a label_map (pass NULL, 0)", n_labels);
    if (label_map) {
        if (n_labels < 1) return fail(MMC_ERR_ARG, "n_labels = %d with a label_map: must be positive", n_labels);
        for (int i = 0; i < n_labels; ++i)
            if (label_map[i] < -1 || label_map[i] >= e->K)
                return fail(MMC_ERR_ARG, "label_map[%d] = %d outside [-1, %d)", i, label_map[i], e->K);
    }
    return MMC_OK;
}

// X: the rows (host with MMC_IN_HOST in flags, else device); y_host or y_dev: the labels.  Every argument has been checked.
static int ensemble_evaluate(mmc_ensemble* e, const float* X, const int32_t* y_host, const int32_t* y_dev, int64_t n, unsigned flags,
                             const int32_t* label_map, int n_labels, const EnsEvalOut& o, hipStream_t st)
{
    const int K = e->K;
    memset(o.totals, 0, EVAL_TOTALS * sizeof(int64_t));
    if (o.rank_hist) memset(o.rank_hist, 0, (size_t)K * sizeof(int64_t));
    if (o.confusion) memset(o.confusion, 0, (size_t)K * K * sizeof(int64_t));
    if (n == 0) return MMC_OK;
    HIP_TRY(hipSetDevice(e->device));
    const int64_t chunk = ensemble_chunk(e, 1);
    const int64_t rows = n < chunk ? n : chunk;
    const int64_t ntot = EVAL_TOTALS + K + (o.confusion ? (int64_t)K * K : 0);
    int r;
    if ((r = e->eval_rows.reserve(5 * rows)) || (r = e->eval_tot.reserve(ntot)) || (label_map && (r = e->eval_map.reserve(n_labels))) ||
        (o.stats && (r = e->stats_stage.reserve(rows * ENSEMBLE_STATS))) || (o.votes && (r = e->votes_stage.reserve(rows))))
        return r;
    int32_t* dy = e->eval_rows.p;
    int32_t* dest = o.est ? dy + rows : nullptr;
    float* dscore = o.score ? reinterpret_cast<float*>(dy + 2 * rows) : nullptr;
    int32_t* drank = o.rank ? dy + 3 * rows : nullptr;
    float* dptrue = o.p_true ? reinterpret_cast<float*>(dy + 4 * rows) : nullptr;
    float* dstats = o.stats ? e->stats_stage.p : nullptr;
    int32_t* dvotes = o.votes ? e->votes_stage.p : nullptr;
    long long* dtot = e->eval_tot.p;
    long long* dhist = dtot + EVAL_TOTALS;
    long long* dconf = o.confusion ? dhist + K : nullptr;
    const int32_t* dmap = label_map ? e->eval_map.p : nullptr;
    HIP_TRY(hipMemsetAsync(dtot, 0, (size_t)ntot * sizeof(long long), st));
    if (label_map) HIP_TRY(hipMemcpyAsync(e->eval_map.p, label_map, (size_t)n_labels * 4, hipMemcpyHostToDevice, st));
    r = ensemble_for_chunks(e, X, n, chunk, flags & MMC_IN_HOST, st, [&](int64_t off, int cur) -> int {
        if (!y_dev) HIP_TRY(hipMemcpyAsync(dy, y_host + off, (size_t)cur * 4, hipMemcpyHostToDevice, st));
        KTRY(launch_ensemble_eval(e->logits.p, cur, K, e->M, (size_t)cur * K, e->cal, y_dev ? y_dev + off : dy, dmap, n_labels, dest, dscore,
                                  drank, dptrue, dstats, dvotes, dtot, dconf, dhist, st));
        // stream order keeps the next chunk's kernel behind these copies
        if (o.est) HIP_TRY(hipMemcpyAsync(o.est + off, dest, (size_t)cur * 4, hipMemcpyDeviceToHost, st));
        if (o.score) HIP_TRY(hipMemcpyAsync(o.score + off, dscore, (size_t)cur * 4, hipMemcpyDeviceToHost, st));
        if (o.rank) HIP_TRY(hipMemcpyAsync(o.rank + off, drank, (size_t)cur * 4, hipMemcpyDeviceToHost, st));
        if (o.p_true) HIP_TRY(hipMemcpyAsync(o.p_true + off, dptrue, (size_t)cur * 4, hipMemcpyDeviceToHost, st));
        if (o.stats) HIP_TRY(hipMemcpyAsync(o.stats + (size_t)off * ENSEMBLE_STATS, dstats, (size_t)cur * ENSEMBLE_STATS * 4, hipMemcpyDeviceToHost, st));
        if (o.votes) HIP_TRY(hipMemcpyAsync(o.votes + off, dvotes, (size_t)cur * 4, hipMemcpyDeviceToHost, st));
        return MMC_OK;
    });
    if (r) return r;
    HIP_TRY(hipMemcpyAsync(o.totals, dtot, EVAL_TOTALS * sizeof(long long), hipMemcpyDeviceToHost, st));
    if (o.rank_hist) HIP_TRY(hipMemcpyAsync(o.rank_hist, dhist, (size_t)K * sizeof(long long), hipMemcpyDeviceToHost, st));
    if (o.confusion) HIP_TRY(hipMemcpyAsync(o.confusion, dconf, (size_t)K * K * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MMC_OK;
}

extern "C" int mmc_ensemble_evaluate(mmc_ensemble* e, const float* feats, const int32_t* y, int64_t n, const int32_t* label_map, int n_labels,
                                     int32_t* est, float* score, int32_t* rank, float* p_true, float* stats, int32_t* votes,
                                     int64_t* totals, int64_t* confusion, int64_t* rank_hist, unsigned flags, void* hip_stream)
{
    const EnsEvalOut o{est, score, rank, p_true, stats, votes, totals, confusion, rank_hist};
    if (int r = ens_eval_check(e, n, label_map, n_labels, o)) return r;
    if (n > 0) {
        if (!feats || !y) return fail(MMC_ERR_ARG, "feats/y is NULL");
        const int hi = label_map ? n_labels : e->K;
        for (int64_t i = 0; i < n; ++i)
            if (y[i] < 0 || y[i] >= hi) return fail(MMC_ERR_ARG, "label index y[%lld] = %d outside [0, %d)", (long long)i, y[i], hi);
    }
    return ensemble_evaluate(e, feats, y, nullptr, n, flags, label_map, n_labels, o, static_cast<hipStream_t>(hip_stream));
}

extern "C" int mmc_ensemble_evaluate_set(mmc_ensemble* e, mmc_featureset* fs, int64_t first, int64_t n, const int32_t* label_map,
                                         int n_labels, int32_t* est, float* score, int32_t* rank, float* p_true, float* stats,
                                         int32_t* votes, int64_t* totals, int64_t* confusion, int64_t* rank_hist, void* hip_stream)
{
    const EnsEvalOut o{est, score, rank, p_true, stats, votes, totals, confusion, rank_hist};
    if (!e) return fail(MMC_ERR_ARG, "ensemble handle is NULL");
    if (!fs) return fail(MMC_ERR_ARG, "feature set handle is NULL");
    if (fs->dim != e->input_dim) return fail(MMC_ERR_ARG, "feature set has %d columns, ensemble expects %d", fs->dim, e->input_dim);
    if (fs->device != e->device) return fail(MMC_ERR_ARG, "feature set is on device %d, ensemble on device %d", fs->device, e->device);
    if (first < 0 || n < 0 || first > fs->n || n > fs->n - first)
        return fail(MMC_ERR_ARG, "rows [%lld, %lld + %lld) outside the set's %lld rows", (long long)first, (long long)first, (long long)n,
                    (long long)fs->n);
    if (int r = ens_eval_check(e, n, label_map, n_labels, o)) return r;
    if (label_map ? fs->K != n_labels : fs->K != e->K)
        return fail(MMC_ERR_ARG, "feature set has %d classes, %s %d", fs->K, label_map ? "label_map covers" : "ensemble", label_map ? n_labels : e->K);
    return ensemble_evaluate(e, fs->X + (size_t)first * fs->dim, nullptr, fs->y + first, n, 0u, label_map, n_labels, o,
                             static_cast<hipStream_t>(hip_stream));
}

// ------------------------------------------------------------------------------------------
// mmc_ensemble_predict_set: the ensemble mean of set rows into a target set (include/mmc.h, "distillation")
// ------------------------------------------------------------------------------------------
// mmc_ensemble_topk's proba at G = 1 and k = 1, chunk by chunk in the ensemble's own chunks, written straight past the target set's
// committed rows; the selection goes to the ensemble's staging and is dropped.  The rows are committed by the set's own rule.
extern "C" int mmc_ensemble_predict_set(mmc_ensemble* e, mmc_featureset* fs, int64_t first, int64_t n, mmc_targetset* ts, void* hip_stream)
{
    if (!e) return fail(MMC_ERR_ARG, "ensemble handle is NULL");
    if (!fs) return fail(MMC_ERR_ARG, "feature set handle is NULL");
    if (!ts) return fail(MMC_ERR_ARG, "target set handle is NULL");
    if (fs->dim != e->input_dim) return fail(MMC_ERR_ARG, "feature set has %d columns, ensemble expects %d", fs->dim, e->input_dim);
    if (fs->device != e->device) return fail(MMC_ERR_ARG, "feature set is on device %d, ensemble on device %d", fs->device, e->device);
    if (ts->device != e->device) return fail(MMC_ERR_ARG, "target set is on device %d, ensemble on device %d", ts->device, e->device);
    if (ts->K != e->K) return fail(MMC_ERR_ARG, "target set has %d classes, ensemble %d", ts->K, e->K);
    if (first < 0 || n < 0 || first > fs->n || n > fs->n - first)
        return fail(MMC_ERR_ARG, "rows [%lld, %lld + %lld) outside the set's %lld rows", (long long)first, (long long)first, (long long)n,
                    (long long)fs->n);
    if (n == 0) return MMC_OK;
    if (n > MMC_TARGETSET_MAX_CELLS / ts->K - ts->n)
        return fail(MMC_ERR_ARG, "%lld + %lld rows x %d classes: a target set holds at most %lld cells (MMC_TARGETSET_MAX_CELLS)",
                    (long long)ts->n, (long long)n, ts->K, (long long)MMC_TARGETSET_MAX_CELLS);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(e->device));
    const int64_t chunk = ensemble_chunk(e, 1);
    const int64_t pts = n < chunk ? n : chunk;
    int r;
    if ((r = e->idx_stage.reserve(pts)) || (r = e->score_stage.reserve(pts))) return r;
    if ((r = targetset_reserve(ts, ts->n + n, st))) return r;
    float* out = ts->P.p + (size_t)ts->n * ts->K;
    const int K = e->K;
    r = ensemble_for_chunks(e, fs->X + (size_t)first * fs->dim, n, chunk, 0u, st, [&](int64_t off, int cur) -> int {
        KTRY(launch_ensemble_topk(e->logits.p, cur, 1, K, e->M, (size_t)cur * K, e->cal, 1, e->idx_stage.p, e->score_stage.p,
                                  out + (size_t)off * K, nullptr, nullptr, st));
        return MMC_OK;
    });
    if (r) return r;
    return targetset_commit(ts, n, first, st);
}
