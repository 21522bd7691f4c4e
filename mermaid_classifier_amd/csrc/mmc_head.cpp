// mmc_head.cpp -- the calibrated MLP head of the C ABI (include/mmc.h): create / predict / top-k, the validation passes
// (mmc_head_evaluate*), cover estimation (mmc_cover_proba, mmc_head_cover*) and mmc_classify_patches.  Every entry point that scores rows goes through head_for_chunks.
// Host C++ only; the kernels are launched through kernels.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "api_internal.h"
#include "head_internal.h"
#include "kernels.h"
#include "trainer_internal.h"

extern "C" void mmc_head_destroy(mmc_head* h)
{
    if (!h) return;
    hipSetDevice(h->device);
    delete h;
}

extern "C" int mmc_head_create(const float* const* W, const float* const* b, const int* dims, int n_layers,
                               const float* a, const float* bcal, int K, int device, mmc_head** out)
{
    if (!out) return fail(MMC_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!W || !b || !dims || !a || !bcal) return fail(MMC_ERR_ARG, "NULL argument");
    if (n_layers < 1 || n_layers > 16) return fail(MMC_ERR_ARG, "n_layers %d out of range [1,16]", n_layers);
    if (K <= 2) return fail(MMC_ERR_ARG, "CalibratedHead only supports the multiclass (K > 2) path; got K=%d", K);
    if (dims[n_layers] != K) return fail(MMC_ERR_ARG, "dims[n_layers]=%d != K=%d", dims[n_layers], K);
    for (int l = 0; l <= n_layers; ++l)
        if (dims[l] < 1) return fail(MMC_ERR_ARG, "dims[%d]=%d must be positive", l, dims[l]);
    if (int r = check_device(device)) return r;
    HIP_TRY(hipSetDevice(device));
    mmc_head* h = new mmc_head();
    h->device = device; h->n_layers = n_layers; h->K = K; h->input_dim = dims[0];
    h->dims_pad.resize(n_layers + 1);
    for (int l = 0; l <= n_layers; ++l) h->dims_pad[l] = (l == n_layers) ? dims[l] : (dims[l] + 3) / 4 * 4;
    h->in_pad = h->dims_pad[0];
    for (int l = 0; l < n_layers; ++l) {
        const int kin = dims[l], kp = h->dims_pad[l], nout = dims[l + 1], np = h->dims_pad[l + 1];
        std::vector<float> wp((size_t)np * kp, 0.f), bp(np, 0.f);
        for (int n = 0; n < nout; ++n) {
            memcpy(&wp[(size_t)n * kp], W[l] + (size_t)n * kin, (size_t)kin * sizeof(float));
            bp[n] = b[l][n];
        }
        DevBuf<float> dw, db;
        if (!dw.alloc((int64_t)wp.size()) || !db.alloc((int64_t)bp.size())) {
            mmc_head_destroy(h);
            return fail(MMC_ERR_NOMEM, "hipMalloc failed for head layer %d", l);
        }
        hipMemcpy(dw, wp.data(), wp.size() * 4, hipMemcpyHostToDevice);
        hipMemcpy(db, bp.data(), bp.size() * 4, hipMemcpyHostToDevice);
        h->W.push_back(std::move(dw)); h->b.push_back(std::move(db));
    }
    if (!h->a.alloc(K) || !h->bc.alloc(K)) {
        mmc_head_destroy(h);
        return fail(MMC_ERR_NOMEM, "hipMalloc failed for calibration parameters");
    }
    hipMemcpy(h->a, a, K * 4, hipMemcpyHostToDevice);
    hipMemcpy(h->bc, bcal, K * 4, hipMemcpyHostToDevice);
    *out = h;
    return MMC_OK;
}

extern "C" int mmc_head_input_dim(const mmc_head* h) { return h ? h->input_dim : 0; }
extern "C" int mmc_head_num_classes(const mmc_head* h) { return h ? h->K : 0; }

// the Linear layers of one chunk (rows staged / padded as needed): returns the last layer's logits (cur x K) in *logits
static int head_logits(mmc_head* h, const float* x, int cur, unsigned flags, hipStream_t st, const float** logits)
{
    const hipMemcpyKind kin = (flags & MMC_IN_HOST) ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    if ((flags & MMC_IN_HOST) || h->in_pad != h->input_dim) {
        if (h->in_pad != h->input_dim) HIP_TRY(hipMemsetAsync(h->in_stage.p, 0, (size_t)cur * h->in_pad * 4, st));
        HIP_TRY(hipMemcpy2DAsync(h->in_stage.p, (size_t)h->in_pad * 4, x, (size_t)h->input_dim * 4,
                                 (size_t)h->input_dim * 4, cur, kin, st));
        x = h->in_stage.p;
    }
    float* pa = h->buf0.p;
    float* pb = h->buf1.p;
    for (int l = 0; l < h->n_layers; ++l) {
        const bool last = l == h->n_layers - 1;
        KTRY(launch_mlp_layer(x, cur, h->dims_pad[l], h->W[l], h->b[l], pa, h->dims_pad[l + 1], !last, st));
        x = pa;
        float* t = pa; pa = pb; pb = t;
    }
    *logits = x;
    return 0;
}

// The one chunk loop of the head: walks rows [0, n) of x (host with MMC_IN_HOST in `flags`, else on the head's device) in chunks
// of HEAD_CHUNK; per chunk it grows the activation buffers, runs the Linear layers and calls each(offset, rows, logits), which
// enqueues what its entry point does with the logits (and synchronises, if it must, before the next chunk reuses the buffers).
// predict, top-k and evaluate all come through here, so the same rows see the same launches and give the same bits.
// (`chunk`: mmc_head_topk_views walks in the largest multiple of its G rows per point below HEAD_CHUNK, so no point is split.)
template <class F>
static int head_for_chunks(mmc_head* h, const float* x, int64_t n, unsigned flags, hipStream_t st, F each, int64_t chunk = HEAD_CHUNK)
{
    int wmax = h->K;
    for (int d : h->dims_pad) wmax = d > wmax ? d : wmax;
    for (int64_t off = 0; off < n; off += chunk) {
        const int cur = (int)((n - off) < chunk ? (n - off) : chunk);
        int r;
        if ((r = h->buf0.reserve((int64_t)cur * wmax)) || (r = h->buf1.reserve((int64_t)cur * wmax)) ||
            (r = h->in_stage.reserve((int64_t)cur * h->in_pad)) || (r = h->proba_stage.reserve((int64_t)cur * h->K)) ||
            (r = h->arg_stage.reserve(cur)))
            return r;
        const float* logits = nullptr;
        if ((r = head_logits(h, x + (size_t)off * h->input_dim, cur, flags, st, &logits))) return r;
        if ((r = each(off, cur, logits))) return r;
    }
    return MMC_OK;
}

extern "C" int mmc_head_predict(mmc_head* h, const float* feats, int64_t n, float* proba, int32_t* argmax,
                                unsigned flags, void* hip_stream)
{
    if (!h) return fail(MMC_ERR_ARG, "head handle is NULL");
    if (n < 0) return fail(MMC_ERR_ARG, "n = %lld is negative", (long long)n);
    if (n == 0) return MMC_OK;
    if (!feats || !proba) return fail(MMC_ERR_ARG, "feats/proba is NULL");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(h->device));
    const bool out_host = (flags & MMC_OUT_HOST) != 0;
    return head_for_chunks(h, feats, n, flags, st, [&](int64_t off, int cur, const float* logits) -> int {
        float* pout = out_host ? h->proba_stage.p : proba + (size_t)off * h->K;
        int32_t* aout = argmax ? (out_host ? h->arg_stage.p : argmax + off) : nullptr;
        KTRY(launch_calibrate(logits, cur, h->K, h->a, h->bc, pout, aout, st));
        if (out_host) {
            HIP_TRY(hipMemcpyAsync(proba + (size_t)off * h->K, pout, (size_t)cur * h->K * 4, hipMemcpyDeviceToHost, st));
            if (argmax) HIP_TRY(hipMemcpyAsync(argmax + off, aout, (size_t)cur * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        return MMC_OK;
    });
}

extern "C" int mmc_head_topk(mmc_head* h, const float* feats, int64_t n, int k, int32_t* idx, float* scores, float* proba,
                             unsigned flags, void* hip_stream)
{
    if (!h) return fail(MMC_ERR_ARG, "head handle is NULL");
    if (n < 0) return fail(MMC_ERR_ARG, "n = %lld is negative", (long long)n);
    if (k < 1 || k > h->K) return fail(MMC_ERR_ARG, "k = %d is outside [1, %d] (the head has %d classes)", k, h->K, h->K);
    if (n == 0) return MMC_OK;
    if (!feats) return fail(MMC_ERR_ARG, "feats is NULL");
    if (!idx || !scores) return fail(MMC_ERR_ARG, "idx/scores is NULL");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(h->device));
    const bool out_host = (flags & MMC_OUT_HOST) != 0;
    if (out_host) {   // the first chunk is the largest: staging that holds it holds every later one
        const int64_t stage = (n < HEAD_CHUNK ? n : HEAD_CHUNK) * k;
        int r;
        if ((r = h->topk_idx_stage.reserve(stage)) || (r = h->topk_score_stage.reserve(stage))) return r;
    }
    return head_for_chunks(h, feats, n, flags, st, [&](int64_t off, int cur, const float* logits) -> int {
        int32_t* iout = out_host ? h->topk_idx_stage.p : idx + (size_t)off * k;
        float* sout = out_host ? h->topk_score_stage.p : scores + (size_t)off * k;
        float* pout = proba ? (out_host ? h->proba_stage.p : proba + (size_t)off * h->K) : nullptr;
        KTRY(launch_calibrate_topk(logits, cur, h->K, h->a, h->bc, k, iout, sout, pout, h->proba_stage.p, st));
        if (out_host) {
            HIP_TRY(hipMemcpyAsync(idx + (size_t)off * k, iout, (size_t)cur * k * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(scores + (size_t)off * k, sout, (size_t)cur * k * 4, hipMemcpyDeviceToHost, st));
            if (proba) HIP_TRY(hipMemcpyAsync(proba + (size_t)off * h->K, pout, (size_t)cur * h->K * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        return MMC_OK;
    });
}

static_assert(MMC_VIEWS_MAX == VIEWS_MAX, "include/mmc.h and kernels.h disagree on the views per point");
extern "C" int mmc_head_topk_views(mmc_head* h, const float* feats, int64_t n_points, int G, int k, int32_t* idx, float* scores,
                                   float* proba, unsigned flags, void* hip_stream)
{
    if (G < 1 || G > VIEWS_MAX) return fail(MMC_ERR_ARG, "G = %d views per point is outside [1, %d]", G, VIEWS_MAX);
    if (k < 1) return fail(MMC_ERR_ARG, "k = %d must be at least 1", k);
    if (!h) return fail(MMC_ERR_ARG, "head handle is NULL");
    if (n_points < 0) return fail(MMC_ERR_ARG, "n_points = %lld is negative", (long long)n_points);
    if (k > h->K) return fail(MMC_ERR_ARG, "k = %d is outside [1, %d] (the head has %d classes)", k, h->K, h->K);
    if (n_points == 0) return MMC_OK;
    if (!feats) return fail(MMC_ERR_ARG, "feats is NULL");
    if (!idx || !scores) return fail(MMC_ERR_ARG, "idx/scores is NULL");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(h->device));
    const bool out_host = (flags & MMC_OUT_HOST) != 0;
    const int64_t chunk = HEAD_CHUNK / G * G;   // rows: whole points only
    if (out_host) {
        const int64_t stage = (n_points < chunk / G ? n_points : chunk / G) * k;
        int r;
        if ((r = h->topk_idx_stage.reserve(stage)) || (r = h->topk_score_stage.reserve(stage))) return r;
    }
    // the means of a chunk's points go to the front of proba_stage (rows x K floats: room for points x K)
    return head_for_chunks(h, feats, n_points * G, flags, st, [&](int64_t off, int cur, const float* logits) -> int {
        const int64_t p0 = off / G;
        const int pts = cur / G;
        int32_t* iout = out_host ? h->topk_idx_stage.p : idx + (size_t)p0 * k;
        float* sout = out_host ? h->topk_score_stage.p : scores + (size_t)p0 * k;
        float* pout = proba ? (out_host ? h->proba_stage.p : proba + (size_t)p0 * h->K) : nullptr;
        KTRY(launch_mean_topk(logits, pts, G, h->K, h->a, h->bc, k, iout, sout, pout, h->proba_stage.p, st));
        if (out_host) {
            HIP_TRY(hipMemcpyAsync(idx + (size_t)p0 * k, iout, (size_t)pts * k * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(scores + (size_t)p0 * k, sout, (size_t)pts * k * 4, hipMemcpyDeviceToHost, st));
            if (proba) HIP_TRY(hipMemcpyAsync(proba + (size_t)p0 * h->K, pout, (size_t)pts * h->K * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        return MMC_OK;
    }, chunk);
}

// ------------------------------------------------------------------------------------------
// validation of a calibrated head: mmc_head_evaluate / mmc_head_evaluate_set
// ------------------------------------------------------------------------------------------
static_assert(MMC_EVAL_TOTALS == EVAL_TOTALS, "include/mmc.h and kernels.h disagree on the totals");
struct EvalOut {
    int32_t* est; float* score; int32_t* rank; float* p_true;
    int64_t* totals; int64_t* confusion; int64_t* rank_hist;
};
// the group inputs and outputs of mmc_head_evaluate_grouped* (include/mmc.h)
struct GroupIO {
    const int64_t* offsets; int64_t n_images; const int32_t* source; int n_sources; int n_bins;
    int64_t *support, *nll_q32, *score_q32, *source_confusion;
    double* cover; int64_t* n_images_used;
    int64_t *bin_count, *bin_correct, *bin_conf_q32; float *bin_conf_min, *bin_conf_max;
    // mmc_head_evaluate_categories* only (with_cat): the category of every class and the per-category tables
    bool with_cat; const int32_t* category_of_class; int n_categories;
    int64_t* cat_rows; int32_t* cat_n_bins;
    int64_t *cat_bin_count, *cat_bin_correct, *cat_bin_conf_q32; float *cat_bin_conf_min, *cat_bin_conf_max;
};
// where the rows and labels of an evaluation come from: rows X (host with MMC_IN_HOST in `flags`, else on the head's device) with
// host labels y, uploaded per chunk; or (`set`) rows [first, first + n) of a feature set, rows and labels read where they lie
struct EvalSrc {
    bool set; int64_t n;
    const float* X; const int32_t* y; unsigned flags;
    const mmc_featureset* fs; int64_t first;
};

static int eval_check_common(const mmc_head* h, int64_t n, const int32_t* label_map, int n_labels, const EvalOut& o)
{
    if (n < 0) return fail(MMC_ERR_ARG, "n = %lld is negative", (long long)n);
    if (!o.totals) return fail(MMC_ERR_ARG, "totals is NULL");
    // the int64 loss total: a row adds at most -log(1e-15) * 2^32 < 36.05 * 2^32 (see MMC_EVALUATE_SET_MAX_ROWS)
    if (n > MMC_EVALUATE_SET_MAX_ROWS)
        return fail(MMC_ERR_ARG, "n = %lld rows in one call: split it (at most %lld)", (long long)n, (long long)MMC_EVALUATE_SET_MAX_ROWS);
    if (!label_map && n_labels != 0) return fail(MMC_ERR_ARG, "n_labels = %d without a label_map (pass NULL, 0)", n_labels);
    if (label_map) {
        if (n_labels < 1) return fail(MMC_ERR_ARG, "n_labels = %d with a label_map: must be positive", n_labels);
        for (int i = 0; i < n_labels; ++i)
            if (label_map[i] < -1 || label_map[i] >= h->K)
                return fail(MMC_ERR_ARG, "label_map[%d] = %d outside [-1, %d)", i, label_map[i], h->K);
    }
    return MMC_OK;
}

// where the grouped pass keeps its device state inside h->grp (every part 256-byte aligned); the first `zero_bytes` are the integer
// tables a call starts from zero
struct GroupLayout {
    size_t true_cnt, pred_cnt, points, cls_tab, source_conf, zero_bytes, offsets, source, keys, slab, cov, n_used, sel, raw, hist;
    size_t cat_of_class, seg, ckeys, cat_rows, cat_bins, cat_sel, cat_raw, bytes;   // (all empty without categories)
    int chunks;
};
static GroupLayout group_layout(int K, int64_t n, const GroupIO& g)
{
    GroupLayout L{};
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t o = at; at += (bytes + 255) / 256 * 256; return o; };
    const bool src = g.source && g.n_sources > 0;
    int64_t per_chunk;
    group_cover_chunks(g.n_images, &per_chunk, &L.chunks);
    L.true_cnt = take((size_t)g.n_images * K * 4);
    L.pred_cnt = take((size_t)g.n_images * K * 4);
    L.points = take((size_t)g.n_images * 4);
    L.cls_tab = take((size_t)3 * K * 8);
    L.source_conf = take(src ? (size_t)g.n_sources * K * K * 8 : 0);
    L.zero_bytes = at;
    L.offsets = take((size_t)(g.n_images + 1) * 8);
    L.source = take(src ? (size_t)g.n_images * 4 : 0);
    L.keys = take((size_t)n * 4);
    L.slab = take((size_t)L.chunks * K * 8 * 8);
    L.cov = take((size_t)K * 8 * 8);
    L.n_used = take(8);
    L.sel = take(sizeof(GroupSelect));
    L.raw = take((size_t)4 * GROUP_MAX_TARGETS * 8);
    L.hist = take((size_t)GROUP_HIST_WORDS * 4);
    const size_t nc = g.with_cat ? (size_t)g.n_categories : 0;
    L.cat_of_class = take(nc ? (size_t)K * 4 : 0);
    L.seg = take(nc ? (size_t)n : 0);
    L.ckeys = take(nc ? (size_t)n * 4 : 0);
    L.cat_rows = take(nc * 8);
    L.cat_bins = take(nc * 4);
    L.cat_sel = take(nc * sizeof(GroupSelect));
    L.cat_raw = take(nc * 4 * GROUP_MAX_TARGETS * 8);
    L.bytes = at;
    return L;
}

// the grouped pass's device state, resolved to typed pointers (source / source_conf are null without source ids)
struct GroupScratch {
    int32_t *true_cnt, *pred_cnt, *points;
    unsigned long long *cls_tab, *source_conf;
    int64_t* offsets; int32_t* source; uint32_t* keys;
    double *slab, *cov; long long* n_used;
    GroupSelect* sel; unsigned long long* raw; uint32_t* hist;
    // null without categories; cat_sel / cat_raw hold one GroupSelect / one raw table per category
    int32_t* cat_of_class; uint8_t* seg; uint32_t* ckeys; long long* cat_rows; int32_t* cat_bins; GroupSelect* cat_sel; unsigned long long* cat_raw;
};

// once per grouped call: lays out and grows h->grp, zeroes the integer tables, uploads offsets and source ids
static int group_prepare(mmc_head* h, int64_t n, const GroupIO& g, hipStream_t st, GroupScratch* s)
{
    const GroupLayout L = group_layout(h->K, n, g);
    int r;
    if ((r = h->grp.reserve((int64_t)L.bytes))) return r;
    char* b = h->grp.p;
    const bool src = g.source && g.n_sources > 0;
    s->true_cnt = reinterpret_cast<int32_t*>(b + L.true_cnt);
    s->pred_cnt = reinterpret_cast<int32_t*>(b + L.pred_cnt);
    s->points = reinterpret_cast<int32_t*>(b + L.points);
    s->cls_tab = reinterpret_cast<unsigned long long*>(b + L.cls_tab);
    s->source_conf = src ? reinterpret_cast<unsigned long long*>(b + L.source_conf) : nullptr;
    s->offsets = reinterpret_cast<int64_t*>(b + L.offsets);
    s->source = src ? reinterpret_cast<int32_t*>(b + L.source) : nullptr;
    s->keys = reinterpret_cast<uint32_t*>(b + L.keys);
    s->slab = reinterpret_cast<double*>(b + L.slab);
    s->cov = reinterpret_cast<double*>(b + L.cov);
    s->n_used = reinterpret_cast<long long*>(b + L.n_used);
    s->sel = reinterpret_cast<GroupSelect*>(b + L.sel);
    s->raw = reinterpret_cast<unsigned long long*>(b + L.raw);
    s->hist = reinterpret_cast<uint32_t*>(b + L.hist);
    HIP_TRY(hipMemsetAsync(b, 0, L.zero_bytes, st));
    HIP_TRY(hipMemcpyAsync(s->offsets, g.offsets, (size_t)(g.n_images + 1) * 8, hipMemcpyHostToDevice, st));
    if (src) HIP_TRY(hipMemcpyAsync(s->source, g.source, (size_t)g.n_images * 4, hipMemcpyHostToDevice, st));
    if (g.with_cat) {
        s->cat_of_class = reinterpret_cast<int32_t*>(b + L.cat_of_class);
        s->seg = reinterpret_cast<uint8_t*>(b + L.seg);
        s->ckeys = reinterpret_cast<uint32_t*>(b + L.ckeys);
        s->cat_rows = reinterpret_cast<long long*>(b + L.cat_rows);
        s->cat_bins = reinterpret_cast<int32_t*>(b + L.cat_bins);
        s->cat_sel = reinterpret_cast<GroupSelect*>(b + L.cat_sel);
        s->cat_raw = reinterpret_cast<unsigned long long*>(b + L.cat_raw);
        HIP_TRY(hipMemcpyAsync(s->cat_of_class, g.category_of_class, (size_t)h->K * 4, hipMemcpyHostToDevice, st));
    }
    return 0;
}
static int head_evaluate_groups(mmc_head* h, int64_t n, const GroupIO& g, const GroupScratch& s, hipStream_t st);

// the extra inputs and outputs of mmc_head_evaluate_ranked* (include/mmc.h)
struct RankIO {
    const uint8_t* sim_level; int n_levels; int kmax;
    int64_t *class_rank_hist, *hier_hist;
};
static_assert(MMC_RANKED_MAX_K == RANK_MAX_K, "include/mmc.h and kernels.h disagree on the selection rounds");
// the ranked pass's device state inside h->rnk (sim_level / hier_hist are null without a level table, class_hist when not asked for)
struct RankScratch { long long *class_hist, *hier_hist; uint8_t* sim_level; };

// once per ranked call: lays out and grows h->rnk, zeroes the two tables, uploads the level table
static int rank_prepare(mmc_head* h, const RankIO& k, hipStream_t st, RankScratch* s)
{
    const size_t cells = (size_t)h->K * h->K;
    const size_t class_bytes = k.class_rank_hist ? cells * 8 : 0, hier_bytes = k.sim_level ? (size_t)k.kmax * k.n_levels * 8 : 0;
    int r;
    if ((r = h->rnk.reserve((int64_t)(class_bytes + hier_bytes + (k.sim_level ? cells : 0))))) return r;
    char* b = h->rnk.p;
    s->class_hist = k.class_rank_hist ? reinterpret_cast<long long*>(b) : nullptr;
    s->hier_hist = k.sim_level ? reinterpret_cast<long long*>(b + class_bytes) : nullptr;
    s->sim_level = k.sim_level ? reinterpret_cast<uint8_t*>(b + class_bytes + hier_bytes) : nullptr;
    if (class_bytes + hier_bytes) HIP_TRY(hipMemsetAsync(b, 0, class_bytes + hier_bytes, st));
    if (k.sim_level) HIP_TRY(hipMemcpyAsync(s->sim_level, k.sim_level, cells, hipMemcpyHostToDevice, st));
    return 0;
}

// scores the rows of `src` (every argument has been checked) and ends in one synchronisation
// with `grp`: every chunk's scored rows also go into the grouped tables, and head_evaluate_groups ends the call
// with `rnk`: every chunk's scored rows also go into the ranking tables (rank_rows_kernel, on the chunk's logits)
static int head_evaluate(mmc_head* h, const EvalSrc& src, const int32_t* label_map, int n_labels, const EvalOut& o, hipStream_t st,
                         const GroupIO* grp, const RankIO* rnk)
{
    const int K = h->K;
    const int64_t n = src.n;
    HIP_TRY(hipSetDevice(h->device));
    const float* X = src.set ? src.fs->X + (size_t)src.first * src.fs->dim : src.X;
    const int32_t* y_dev = src.set ? src.fs->y + src.first : nullptr;
    const int64_t rows = n < HEAD_CHUNK ? n : HEAD_CHUNK;
    const int64_t ntot = EVAL_TOTALS + K + (o.confusion ? (int64_t)K * K : 0);
    int r;
    if ((r = h->eval_rows.reserve(6 * rows))) return r;
    if ((r = h->eval_tot.reserve(ntot))) return r;
    if (label_map && (r = h->eval_map.reserve(n_labels))) return r;
    int32_t* dy = h->eval_rows.p;
    int32_t* dest = (o.est || grp) ? dy + rows : nullptr;
    float* dscore = (o.score || grp) ? reinterpret_cast<float*>(dy + 2 * rows) : nullptr;
    int32_t* drank = (o.rank || rnk) ? dy + 3 * rows : nullptr;
    float* dptrue = (o.p_true || grp) ? reinterpret_cast<float*>(dy + 4 * rows) : nullptr;
    int32_t* dscored = (grp || rnk) ? dy + 5 * rows : nullptr;
    GroupScratch gs{};
    if (grp && (r = group_prepare(h, n, *grp, st, &gs))) return r;
    RankScratch rs{};
    if (rnk && (r = rank_prepare(h, *rnk, st, &rs))) return r;
    GroupRowsArgs ga{};   // (rows and row0 are set per chunk)
    if (grp) {
        ga.scored = dscored; ga.est = dest; ga.score = dscore; ga.p_true = dptrue;
        ga.K = K; ga.offsets = gs.offsets; ga.n_images = grp->n_images; ga.source_of_image = gs.source;
        ga.true_cnt = gs.true_cnt; ga.pred_cnt = gs.pred_cnt; ga.points = gs.points;
        ga.cls_tab = gs.cls_tab; ga.source_conf = gs.source_conf; ga.keys = gs.keys;
        ga.category_of_class = gs.cat_of_class; ga.seg = gs.seg;
    }
    long long* dtot = h->eval_tot.p;
    long long* dhist = dtot + EVAL_TOTALS;
    long long* dconf = o.confusion ? dhist + K : nullptr;
    const int32_t* dmap = label_map ? h->eval_map.p : nullptr;
    HIP_TRY(hipMemsetAsync(dtot, 0, (size_t)ntot * sizeof(long long), st));
    if (label_map) HIP_TRY(hipMemcpyAsync(h->eval_map.p, label_map, (size_t)n_labels * 4, hipMemcpyHostToDevice, st));
    r = head_for_chunks(h, X, n, src.set ? 0u : src.flags & MMC_IN_HOST, st, [&](int64_t off, int cur, const float* logits) -> int {
        if (!y_dev) HIP_TRY(hipMemcpyAsync(dy, src.y + off, (size_t)cur * 4, hipMemcpyHostToDevice, st));
        KTRY(launch_calibrate_eval(logits, cur, K, h->a, h->bc, y_dev ? y_dev + off : dy, dmap, n_labels, dest, dscore, drank, dptrue,
                                   dtot, dconf, dhist, dscored, h->proba_stage.p, st));
        if (grp) {
            ga.rows = cur; ga.row0 = off;
            KTRY(launch_group_rows(ga, st));
        }
        if (rnk)
            KTRY(launch_rank_rows(logits, cur, K, h->a, h->bc, dscored, drank, rs.sim_level, rnk->n_levels, rnk->kmax, rs.class_hist,
                                  rs.hier_hist, h->proba_stage.p, st));
        // stream order keeps the next chunk's kernel behind these copies
        if (o.est) HIP_TRY(hipMemcpyAsync(o.est + off, dest, (size_t)cur * 4, hipMemcpyDeviceToHost, st));
        if (o.score) HIP_TRY(hipMemcpyAsync(o.score + off, dscore, (size_t)cur * 4, hipMemcpyDeviceToHost, st));
        if (o.rank) HIP_TRY(hipMemcpyAsync(o.rank + off, drank, (size_t)cur * 4, hipMemcpyDeviceToHost, st));
        if (o.p_true) HIP_TRY(hipMemcpyAsync(o.p_true + off, dptrue, (size_t)cur * 4, hipMemcpyDeviceToHost, st));
        return MMC_OK;
    });
    if (r) return r;
    HIP_TRY(hipMemcpyAsync(o.totals, dtot, EVAL_TOTALS * sizeof(long long), hipMemcpyDeviceToHost, st));
    if (o.rank_hist) HIP_TRY(hipMemcpyAsync(o.rank_hist, dhist, (size_t)K * sizeof(long long), hipMemcpyDeviceToHost, st));
    if (o.confusion) HIP_TRY(hipMemcpyAsync(o.confusion, dconf, (size_t)K * K * sizeof(long long), hipMemcpyDeviceToHost, st));
    if (rnk && rnk->class_rank_hist)
        HIP_TRY(hipMemcpyAsync(rnk->class_rank_hist, rs.class_hist, (size_t)K * K * sizeof(long long), hipMemcpyDeviceToHost, st));
    if (rnk && rnk->hier_hist)
        HIP_TRY(hipMemcpyAsync(rnk->hier_hist, rs.hier_hist, (size_t)rnk->kmax * rnk->n_levels * sizeof(long long), hipMemcpyDeviceToHost, st));
    if (grp) return head_evaluate_groups(h, n, *grp, gs, st);
    HIP_TRY(hipStreamSynchronize(st));
    return MMC_OK;
}

static void eval_clear(const mmc_head* h, const EvalOut& o)
{
    if (o.totals) memset(o.totals, 0, EVAL_TOTALS * sizeof(int64_t));
    if (h && o.rank_hist) memset(o.rank_hist, 0, (size_t)h->K * sizeof(int64_t));
    if (h && o.confusion) memset(o.confusion, 0, (size_t)h->K * h->K * sizeof(int64_t));
}

// ------------------------------------------------------------------------------------------
// grouped validation: the part of mmc_head_evaluate_grouped / mmc_head_evaluate_grouped_set after the last chunk
// ------------------------------------------------------------------------------------------
static_assert(MMC_GROUPED_MAX_BINS == GROUP_MAX_BINS, "include/mmc.h and kernels.h disagree on the bins");

// the per-bin tables from the edge keys and the per-edge-key sums: in sorted order the rows are [== e_0][between e_0 and e_1][== e_1]
// ... [== e_last]; a between-region lies in one bin, an equal-key group is split by its positions (all its rows contribute alike)
// count / correct / conf / cmin / cmax: nb entries each, zeroed here
static int bins_from_select(const GroupSelect& s, const unsigned long long* raw, int nb, int64_t* count, int64_t* correct, int64_t* conf,
                            float* cmin, float* cmax)
{
    const int64_t ns = s.n_scored;
    for (int i = 0; i < nb; ++i) { count[i] = correct[i] = conf[i] = 0; cmin[i] = cmax[i] = 0.f; }
    if (ns > 0) {
        if (s.n_targets != 2u * nb || s.n_slots < 1 || s.n_slots > s.n_targets) return fail(MMC_ERR_HIP, "grouped validation: select state is inconsistent");
        auto edge = [&](int b) { return (int64_t)b * ns / nb; };
        auto score_of = [](uint32_t key) { const uint32_t u = key >> 1; float f; memcpy(&f, &u, 4); return f; };
        int64_t pos = 0;
        int b = 0;
        for (uint32_t j = 0; j < s.n_slots; ++j) {
            const uint32_t key = s.slot_prefix[j];
            const int64_t q = llrint((double)score_of(key) * 4294967296.0);
            int64_t at = pos, end = pos + (int64_t)raw[j];
            while (at < end) {
                while (b < nb - 1 && edge(b + 1) <= at) ++b;
                const int64_t hi = edge(b + 1) < end ? edge(b + 1) : end, m = hi - at;
                if (m <= 0) return fail(MMC_ERR_HIP, "grouped validation: bin positions are inconsistent");
                count[b] += m; correct[b] += (key & 1u) ? m : 0; conf[b] += m * q;
                at = hi;
            }
            pos = end;
            const int64_t ic = (int64_t)raw[GROUP_MAX_TARGETS + j];
            if (ic > 0) {
                while (b < nb - 1 && edge(b + 1) <= pos) ++b;
                count[b] += ic; correct[b] += (int64_t)raw[2 * GROUP_MAX_TARGETS + j]; conf[b] += (int64_t)raw[3 * GROUP_MAX_TARGETS + j];
                pos += ic;
            }
        }
        if (pos != ns) return fail(MMC_ERR_HIP, "grouped validation: %lld keys binned, %lld rows scored", (long long)pos, (long long)ns);
        for (int i = 0; i < nb; ++i) {
            if (count[i] != edge(i + 1) - edge(i)) return fail(MMC_ERR_HIP, "grouped validation: bin %d holds %lld rows", i, (long long)count[i]);
            if (count[i]) { cmin[i] = score_of(s.tgt_prefix[2 * i]); cmax[i] = score_of(s.tgt_prefix[2 * i + 1]); }
        }
    }
    return MMC_OK;
}

// the bins of the whole split
static int group_bins(const GroupSelect& s, const unsigned long long* raw, const GroupIO& g)
{
    const int nb = g.n_bins;
    std::vector<int64_t> count(nb), correct(nb), conf(nb);
    std::vector<float> cmin(nb), cmax(nb);
    int r = bins_from_select(s, raw, nb, count.data(), correct.data(), conf.data(), cmin.data(), cmax.data());
    if (r) return r;
    if (g.bin_count) memcpy(g.bin_count, count.data(), (size_t)nb * 8);
    if (g.bin_correct) memcpy(g.bin_correct, correct.data(), (size_t)nb * 8);
    if (g.bin_conf_q32) memcpy(g.bin_conf_q32, conf.data(), (size_t)nb * 8);
    if (g.bin_conf_min) memcpy(g.bin_conf_min, cmin.data(), (size_t)nb * 4);
    if (g.bin_conf_max) memcpy(g.bin_conf_max, cmax.data(), (size_t)nb * 4);
    return MMC_OK;
}

static_assert(MMC_CATEGORY_MAX == GROUP_MAX_CATEGORIES && MMC_CATEGORY_MAX_BINS == GROUP_CAT_BINS_MAX &&
                  MMC_CATEGORY_MIN_BINS == GROUP_CAT_BINS_MIN && MMC_CATEGORY_ROWS_PER_BIN == GROUP_CAT_ROWS_PER_BIN &&
                  2 * GROUP_CAT_BINS_MAX <= GROUP_MAX_TARGETS,
              "include/mmc.h and kernels.h disagree on the categories");
// the bins of a category of `rows` > 0 rows (calibration.py:137), as category_counts_kernel computes them on the device
static int category_bins(int64_t rows)
{
    int64_t nb = rows / GROUP_CAT_ROWS_PER_BIN;
    nb = nb < GROUP_CAT_BINS_MIN ? GROUP_CAT_BINS_MIN : nb;
    return (int)(nb > GROUP_CAT_BINS_MAX ? GROUP_CAT_BINS_MAX : nb);
}

// after the last chunk: the cover reduction and the select on the device, the tables to the host, one synchronisation, the bins
static int head_evaluate_groups(mmc_head* h, int64_t n, const GroupIO& g, const GroupScratch& s, hipStream_t st)
{
    const int K = h->K;
    KTRY(launch_group_cover(s.true_cnt, s.pred_cnt, s.points, g.n_images, K, s.slab, s.cov, s.n_used, st));
    KTRY(launch_group_select(s.keys, n, h->eval_tot.p, g.n_bins, s.sel, s.hist, s.raw, st));
    GroupSelect sel;
    std::vector<unsigned long long> raw((size_t)4 * GROUP_MAX_TARGETS);
    if (g.support) HIP_TRY(hipMemcpyAsync(g.support, s.cls_tab, (size_t)K * 8, hipMemcpyDeviceToHost, st));
    if (g.nll_q32) HIP_TRY(hipMemcpyAsync(g.nll_q32, s.cls_tab + K, (size_t)K * 8, hipMemcpyDeviceToHost, st));
    if (g.score_q32) HIP_TRY(hipMemcpyAsync(g.score_q32, s.cls_tab + 2 * K, (size_t)K * 8, hipMemcpyDeviceToHost, st));
    if (g.source_confusion && s.source_conf)
        HIP_TRY(hipMemcpyAsync(g.source_confusion, s.source_conf, (size_t)g.n_sources * K * K * 8, hipMemcpyDeviceToHost, st));
    if (g.cover) HIP_TRY(hipMemcpyAsync(g.cover, s.cov, (size_t)K * 8 * 8, hipMemcpyDeviceToHost, st));
    if (g.n_images_used) HIP_TRY(hipMemcpyAsync(g.n_images_used, s.n_used, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&sel, s.sel, sizeof(sel), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(raw.data(), s.raw, raw.size() * 8, hipMemcpyDeviceToHost, st));
    // per category: its rows and bins from the per-class support, then the same select over its rows alone (metrics.hip)
    const int nc = g.with_cat ? g.n_categories : 0;
    std::vector<GroupSelect> cat_sel(nc);
    std::vector<unsigned long long> cat_raw((size_t)nc * 4 * GROUP_MAX_TARGETS);
    std::vector<long long> cat_rows(nc);
    if (nc) {
        KTRY(launch_group_category_counts(s.cls_tab, s.cat_of_class, K, nc, s.cat_rows, s.cat_bins, st));
        for (int c = 0; c < nc; ++c)
            KTRY(launch_group_select_category(s.keys, s.seg, n, c, s.cat_rows, s.cat_bins, s.ckeys, s.cat_sel + c, s.hist,
                                              s.cat_raw + (size_t)c * 4 * GROUP_MAX_TARGETS, st));
        HIP_TRY(hipMemcpyAsync(cat_rows.data(), s.cat_rows, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(cat_sel.data(), s.cat_sel, (size_t)nc * sizeof(GroupSelect), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(cat_raw.data(), s.cat_raw, cat_raw.size() * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    int r = group_bins(sel, raw.data(), g);
    if (r) return r;
    for (int c = 0; c < nc; ++c) {
        const int64_t rows = cat_rows[c];
        const int nb = rows > 0 ? category_bins(rows) : 0;
        int64_t count[MMC_CATEGORY_MAX_BINS] = {}, correct[MMC_CATEGORY_MAX_BINS] = {}, conf[MMC_CATEGORY_MAX_BINS] = {};
        float cmin[MMC_CATEGORY_MAX_BINS] = {}, cmax[MMC_CATEGORY_MAX_BINS] = {};
        if ((int64_t)cat_sel[c].n_scored != rows)
            return fail(MMC_ERR_HIP, "category validation: category %d selected over %u rows, holds %lld", c, cat_sel[c].n_scored, (long long)rows);
        if ((r = bins_from_select(cat_sel[c], cat_raw.data() + (size_t)c * 4 * GROUP_MAX_TARGETS, nb, count, correct, conf, cmin, cmax))) return r;
        const size_t at = (size_t)c * MMC_CATEGORY_MAX_BINS;
        if (g.cat_rows) g.cat_rows[c] = rows;
        if (g.cat_n_bins) g.cat_n_bins[c] = nb;
        if (g.cat_bin_count) memcpy(g.cat_bin_count + at, count, sizeof(count));
        if (g.cat_bin_correct) memcpy(g.cat_bin_correct + at, correct, sizeof(correct));
        if (g.cat_bin_conf_q32) memcpy(g.cat_bin_conf_q32 + at, conf, sizeof(conf));
        if (g.cat_bin_conf_min) memcpy(g.cat_bin_conf_min + at, cmin, sizeof(cmin));
        if (g.cat_bin_conf_max) memcpy(g.cat_bin_conf_max + at, cmax, sizeof(cmax));
    }
    return MMC_OK;
}

// zeroes every group output whose size the arguments determine
static void group_clear(const mmc_head* h, const GroupIO& g)
{
    if (g.with_cat && g.n_categories >= 1 && g.n_categories <= MMC_CATEGORY_MAX) {
        const size_t nc = (size_t)g.n_categories, cells = nc * MMC_CATEGORY_MAX_BINS;
        if (g.cat_rows) memset(g.cat_rows, 0, nc * 8);
        if (g.cat_n_bins) memset(g.cat_n_bins, 0, nc * 4);
        if (g.cat_bin_count) memset(g.cat_bin_count, 0, cells * 8);
        if (g.cat_bin_correct) memset(g.cat_bin_correct, 0, cells * 8);
        if (g.cat_bin_conf_q32) memset(g.cat_bin_conf_q32, 0, cells * 8);
        if (g.cat_bin_conf_min) memset(g.cat_bin_conf_min, 0, cells * 4);
        if (g.cat_bin_conf_max) memset(g.cat_bin_conf_max, 0, cells * 4);
    }
    if (!h) return;
    const size_t K = (size_t)h->K;
    if (g.support) memset(g.support, 0, K * 8);
    if (g.nll_q32) memset(g.nll_q32, 0, K * 8);
    if (g.score_q32) memset(g.score_q32, 0, K * 8);
    if (g.source_confusion && g.n_sources > 0 && (int64_t)g.n_sources * h->K * h->K <= MMC_GROUPED_MAX_SOURCE_CELLS)
        memset(g.source_confusion, 0, (size_t)g.n_sources * K * K * 8);
    if (g.cover) memset(g.cover, 0, K * MMC_COVER_SUMS * 8);
    if (g.n_images_used) *g.n_images_used = 0;
    if (g.n_bins >= 1 && g.n_bins <= MMC_GROUPED_MAX_BINS) {
        if (g.bin_count) memset(g.bin_count, 0, (size_t)g.n_bins * 8);
        if (g.bin_correct) memset(g.bin_correct, 0, (size_t)g.n_bins * 8);
        if (g.bin_conf_q32) memset(g.bin_conf_q32, 0, (size_t)g.n_bins * 8);
        if (g.bin_conf_min) memset(g.bin_conf_min, 0, (size_t)g.n_bins * 4);
        if (g.bin_conf_max) memset(g.bin_conf_max, 0, (size_t)g.n_bins * 4);
    }
}

static int group_check(const mmc_head* h, int64_t n, const GroupIO& g)
{
    if (g.n_bins < 1 || g.n_bins > MMC_GROUPED_MAX_BINS)
        return fail(MMC_ERR_ARG, "n_bins = %d outside [1, %d]", g.n_bins, MMC_GROUPED_MAX_BINS);
    if (g.n_sources < 0) return fail(MMC_ERR_ARG, "n_sources = %d is negative", g.n_sources);
    if (g.n_images < 0) return fail(MMC_ERR_ARG, "n_images = %lld is negative", (long long)g.n_images);
    if (g.with_cat) {
        if (g.n_categories < 1 || g.n_categories > MMC_CATEGORY_MAX)
            return fail(MMC_ERR_ARG, "n_categories = %d outside [1, %d]", g.n_categories, MMC_CATEGORY_MAX);
        if (!g.category_of_class) return fail(MMC_ERR_ARG, "category_of_class is NULL");
        for (int k = 0; k < h->K; ++k)
            if (g.category_of_class[k] < -1 || g.category_of_class[k] >= g.n_categories)
                return fail(MMC_ERR_ARG, "category_of_class[%d] = %d outside [-1, %d)", k, g.category_of_class[k], g.n_categories);
    }
    if (n == 0) return g.n_images == 0 ? MMC_OK : fail(MMC_ERR_ARG, "%lld images over no rows", (long long)g.n_images);
    if (!g.offsets) return fail(MMC_ERR_ARG, "image_offsets is NULL");
    if (g.n_images < 1 || g.n_images > n) return fail(MMC_ERR_ARG, "n_images = %lld for %lld rows: every image owns at least one row", (long long)g.n_images, (long long)n);
    if (g.n_images * h->K > MMC_GROUPED_MAX_COVER_CELLS)
        return fail(MMC_ERR_ARG, "n_images * K = %lld cells of per-image counts: at most %lld", (long long)(g.n_images * h->K), (long long)MMC_GROUPED_MAX_COVER_CELLS);
    if (g.offsets[0] != 0) return fail(MMC_ERR_ARG, "image_offsets[0] = %lld: must be 0", (long long)g.offsets[0]);
    for (int64_t i = 0; i < g.n_images; ++i)
        if (g.offsets[i + 1] <= g.offsets[i])
            return fail(MMC_ERR_ARG, "image_offsets[%lld] = %lld is not above image_offsets[%lld] = %lld (offsets increase strictly: no empty image)",
                        (long long)(i + 1), (long long)g.offsets[i + 1], (long long)i, (long long)g.offsets[i]);
    if (g.offsets[g.n_images] != n) return fail(MMC_ERR_ARG, "image_offsets[n_images] = %lld: must be n = %lld", (long long)g.offsets[g.n_images], (long long)n);
    if (g.source && g.n_sources > 0) {
        if ((int64_t)g.n_sources * h->K * h->K > MMC_GROUPED_MAX_SOURCE_CELLS)
            return fail(MMC_ERR_ARG, "n_sources * K * K = %lld cells of per-source confusion: at most %lld", (long long)g.n_sources * h->K * h->K,
                        (long long)MMC_GROUPED_MAX_SOURCE_CELLS);
        for (int64_t i = 0; i < g.n_images; ++i)
            if (g.source[i] < 0 || g.source[i] >= g.n_sources)
                return fail(MMC_ERR_ARG, "source_of_image[%lld] = %d outside [0, %d)", (long long)i, g.source[i], g.n_sources);
    }
    return MMC_OK;
}

// zeroes every ranking output whose size the arguments determine
static void rank_clear(const mmc_head* h, const RankIO& k)
{
    if (h && k.class_rank_hist) memset(k.class_rank_hist, 0, (size_t)h->K * h->K * 8);
    if (k.hier_hist && k.n_levels >= 1 && k.n_levels <= 256 && k.kmax >= 1 && k.kmax <= MMC_RANKED_MAX_K)
        memset(k.hier_hist, 0, (size_t)k.kmax * k.n_levels * 8);
}

static int rank_check(const mmc_head* h, const RankIO& k)
{
    if (k.n_levels < 1 || k.n_levels > 256) return fail(MMC_ERR_ARG, "n_levels = %d outside [1, 256]", k.n_levels);
    const int top = h->K < MMC_RANKED_MAX_K ? h->K : MMC_RANKED_MAX_K;
    if (k.kmax < 1 || k.kmax > top) return fail(MMC_ERR_ARG, "kmax = %d outside [1, %d] (the head has %d classes)", k.kmax, top, h->K);
    if (k.sim_level && !k.hier_hist) return fail(MMC_ERR_ARG, "sim_level without hier_hist");
    if (!k.sim_level && k.hier_hist) return fail(MMC_ERR_ARG, "hier_hist without sim_level");
    if (k.sim_level)
        for (int64_t i = 0, e = (int64_t)h->K * h->K; i < e; ++i)
            if (k.sim_level[i] >= k.n_levels)
                return fail(MMC_ERR_ARG, "sim_level[%lld] = %d outside [0, %d)", (long long)i, (int)k.sim_level[i], k.n_levels);
    return MMC_OK;
}

// ------------------------------------------------------------------------------------------
// the eight evaluate entry points: each names its source, its outputs and (grouped, categories, ranked) its extra tables, and makes one call
// ------------------------------------------------------------------------------------------
// the feature-set form: the slice, then the common checks, then the classes (the set's labels lie in [0, fs->K): that range must be
// the head's classes, or the map's domain)
static int eval_check_set(const mmc_head* h, const EvalSrc& s, const int32_t* label_map, int n_labels, const EvalOut& o)
{
    const mmc_featureset* fs = s.fs;
    if (!fs) return fail(MMC_ERR_ARG, "feature set handle is NULL");
    if (fs->dim != h->input_dim) return fail(MMC_ERR_ARG, "feature set has %d columns, head expects %d", fs->dim, h->input_dim);
    if (fs->device != h->device) return fail(MMC_ERR_ARG, "feature set is on device %d, head on device %d", fs->device, h->device);
    if (s.first < 0 || s.n < 0 || s.first > fs->n || s.n > fs->n - s.first)
        return fail(MMC_ERR_ARG, "rows [%lld, %lld + %lld) outside the set's %lld rows", (long long)s.first, (long long)s.first,
                    (long long)s.n, (long long)fs->n);
    int r = eval_check_common(h, s.n, label_map, n_labels, o);
    if (r) return r;
    if (label_map ? fs->K != n_labels : fs->K != h->K)
        return fail(MMC_ERR_ARG, "feature set has %d classes, %s %d", fs->K, label_map ? "label_map covers" : "head", label_map ? n_labels : h->K);
    return MMC_OK;
}

// host labels index the head's classes, or the map's domain
static int eval_check_labels(const mmc_head* h, const EvalSrc& s, const int32_t* label_map, int n_labels)
{
    if (!s.X || !s.y) return fail(MMC_ERR_ARG, "feats/y is NULL");
    const int hi = label_map ? n_labels : h->K;
    for (int64_t i = 0; i < s.n; ++i)
        if (s.y[i] < 0 || s.y[i] >= hi) return fail(MMC_ERR_ARG, "label index y[%lld] = %d outside [0, %d)", (long long)i, s.y[i], hi);
    return MMC_OK;
}

static int evaluate(mmc_head* h, const EvalSrc& s, const int32_t* label_map, int n_labels, const EvalOut& o, const GroupIO* g,
                    const RankIO* k, void* hip_stream)
{
    // When the outputs are zeroed is part of each pair's contract (include/mmc.h) and differs on purpose.  A grouped or ranked call zeroes
    // them before any check, the NULL-handle check included, and again when the pass fails: whatever it returns, no table holds
    // stale or partial counts.  A plain call zeroes them only once its arguments have passed: a rejected call writes nothing.
    const bool clear_first = g != nullptr || k != nullptr;
    auto clear_all = [&] { eval_clear(h, o); if (g) group_clear(h, *g); if (k) rank_clear(h, *k); };
    if (clear_first) clear_all();
    if (!h) return fail(MMC_ERR_ARG, "head handle is NULL");
    int r = s.set ? eval_check_set(h, s, label_map, n_labels, o) : eval_check_common(h, s.n, label_map, n_labels, o);
    if (r) return r;
    if (g && (r = group_check(h, s.n, *g))) return r;
    if (k && (r = rank_check(h, *k))) return r;
    if (!clear_first) eval_clear(h, o);
    if (s.n == 0) return MMC_OK;
    if (!s.set && (r = eval_check_labels(h, s, label_map, n_labels))) return r;
    r = head_evaluate(h, s, label_map, n_labels, o, static_cast<hipStream_t>(hip_stream), g, k);
    if (r && clear_first) clear_all();
    return r;
}

static EvalSrc host_rows(const float* feats, const int32_t* y, int64_t n, unsigned flags) { return {false, n, feats, y, flags, nullptr, 0}; }
static EvalSrc set_rows(const mmc_featureset* fs, int64_t first, int64_t n) { return {true, n, nullptr, nullptr, 0u, fs, first}; }

extern "C" int mmc_head_evaluate(mmc_head* h, const float* feats, const int32_t* y, int64_t n, const int32_t* label_map, int n_labels,
                                 int32_t* est, float* score, int32_t* rank, float* p_true, int64_t* totals, int64_t* confusion,
                                 int64_t* rank_hist, unsigned flags, void* hip_stream)
{
    const EvalOut o{est, score, rank, p_true, totals, confusion, rank_hist};
    return evaluate(h, host_rows(feats, y, n, flags), label_map, n_labels, o, nullptr, nullptr, hip_stream);
}

extern "C" int mmc_head_evaluate_set(mmc_head* h, mmc_featureset* fs, int64_t first, int64_t n, const int32_t* label_map, int n_labels,
                                     int32_t* est, float* score, int32_t* rank, float* p_true, int64_t* totals, int64_t* confusion,
                                     int64_t* rank_hist, void* hip_stream)
{
    const EvalOut o{est, score, rank, p_true, totals, confusion, rank_hist};
    return evaluate(h, set_rows(fs, first, n), label_map, n_labels, o, nullptr, nullptr, hip_stream);
}

// the group arguments of the two grouped entry points, in the order of include/mmc.h
static GroupIO group_io(const int64_t* image_offsets, int64_t n_images, const int32_t* source_of_image, int n_sources, int n_bins,
                        int64_t* support, int64_t* nll_q32, int64_t* score_q32, int64_t* source_confusion, double* cover_sums,
                        int64_t* n_images_used, int64_t* bin_count, int64_t* bin_correct, int64_t* bin_conf_q32, float* bin_conf_min,
                        float* bin_conf_max)
{
    return {image_offsets, n_images, source_of_image, n_sources, n_bins, support, nll_q32, score_q32, source_confusion,
            cover_sums, n_images_used, bin_count, bin_correct, bin_conf_q32, bin_conf_min, bin_conf_max,
            false, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
}

extern "C" int mmc_head_evaluate_grouped(mmc_head* h, const float* feats, const int32_t* y, int64_t n, const int32_t* label_map, int n_labels,
                                         int32_t* est, float* score, int32_t* rank, float* p_true, int64_t* totals, int64_t* confusion,
                                         int64_t* rank_hist, const int64_t* image_offsets, int64_t n_images, const int32_t* source_of_image,
                                         int n_sources, int n_bins, int64_t* support, int64_t* nll_q32, int64_t* score_q32,
                                         int64_t* source_confusion, double* cover_sums, int64_t* n_images_used, int64_t* bin_count,
                                         int64_t* bin_correct, int64_t* bin_conf_q32, float* bin_conf_min, float* bin_conf_max, unsigned flags,
                                         void* hip_stream)
{
    const EvalOut o{est, score, rank, p_true, totals, confusion, rank_hist};
    const GroupIO g = group_io(image_offsets, n_images, source_of_image, n_sources, n_bins, support, nll_q32, score_q32, source_confusion,
                               cover_sums, n_images_used, bin_count, bin_correct, bin_conf_q32, bin_conf_min, bin_conf_max);
    return evaluate(h, host_rows(feats, y, n, flags), label_map, n_labels, o, &g, nullptr, hip_stream);
}

extern "C" int mmc_head_evaluate_grouped_set(mmc_head* h, mmc_featureset* fs, int64_t first, int64_t n, const int32_t* label_map, int n_labels,
                                             int32_t* est, float* score, int32_t* rank, float* p_true, int64_t* totals, int64_t* confusion,
                                             int64_t* rank_hist, const int64_t* image_offsets, int64_t n_images,
                                             const int32_t* source_of_image, int n_sources, int n_bins, int64_t* support, int64_t* nll_q32,
                                             int64_t* score_q32, int64_t* source_confusion, double* cover_sums, int64_t* n_images_used,
                                             int64_t* bin_count, int64_t* bin_correct, int64_t* bin_conf_q32, float* bin_conf_min,
                                             float* bin_conf_max, void* hip_stream)
{
    const EvalOut o{est, score, rank, p_true, totals, confusion, rank_hist};
    const GroupIO g = group_io(image_offsets, n_images, source_of_image, n_sources, n_bins, support, nll_q32, score_q32, source_confusion,
                               cover_sums, n_images_used, bin_count, bin_correct, bin_conf_q32, bin_conf_min, bin_conf_max);
    return evaluate(h, set_rows(fs, first, n), label_map, n_labels, o, &g, nullptr, hip_stream);
}

// the category arguments of the two category entry points, in the order of include/mmc.h, onto the group arguments
static GroupIO with_categories(GroupIO g, const int32_t* category_of_class, int n_categories, int64_t* cat_rows, int32_t* cat_n_bins,
                               int64_t* cat_bin_count, int64_t* cat_bin_correct, int64_t* cat_bin_conf_q32, float* cat_bin_conf_min,
                               float* cat_bin_conf_max)
{
    g.with_cat = true; g.category_of_class = category_of_class; g.n_categories = n_categories;
    g.cat_rows = cat_rows; g.cat_n_bins = cat_n_bins;
    g.cat_bin_count = cat_bin_count; g.cat_bin_correct = cat_bin_correct; g.cat_bin_conf_q32 = cat_bin_conf_q32;
    g.cat_bin_conf_min = cat_bin_conf_min; g.cat_bin_conf_max = cat_bin_conf_max;
    return g;
}

extern "C" int mmc_head_evaluate_categories(mmc_head* h, const float* feats, const int32_t* y, int64_t n, const int32_t* label_map, int n_labels,
                                            int32_t* est, float* score, int32_t* rank, float* p_true, int64_t* totals, int64_t* confusion,
                                            int64_t* rank_hist, const int64_t* image_offsets, int64_t n_images, const int32_t* source_of_image,
                                            int n_sources, int n_bins, int64_t* support, int64_t* nll_q32, int64_t* score_q32,
                                            int64_t* source_confusion, double* cover_sums, int64_t* n_images_used, int64_t* bin_count,
                                            int64_t* bin_correct, int64_t* bin_conf_q32, float* bin_conf_min, float* bin_conf_max,
                                            const int32_t* category_of_class, int n_categories, int64_t* cat_rows, int32_t* cat_n_bins,
                                            int64_t* cat_bin_count, int64_t* cat_bin_correct, int64_t* cat_bin_conf_q32, float* cat_bin_conf_min,
                                            float* cat_bin_conf_max, unsigned flags, void* hip_stream)
{
    const EvalOut o{est, score, rank, p_true, totals, confusion, rank_hist};
    const GroupIO g = with_categories(group_io(image_offsets, n_images, source_of_image, n_sources, n_bins, support, nll_q32, score_q32,
                                               source_confusion, cover_sums, n_images_used, bin_count, bin_correct, bin_conf_q32, bin_conf_min,
                                               bin_conf_max),
                                      category_of_class, n_categories, cat_rows, cat_n_bins, cat_bin_count, cat_bin_correct, cat_bin_conf_q32,
                                      cat_bin_conf_min, cat_bin_conf_max);
    return evaluate(h, host_rows(feats, y, n, flags), label_map, n_labels, o, &g, nullptr, hip_stream);
}

extern "C" int mmc_head_evaluate_categories_set(mmc_head* h, mmc_featureset* fs, int64_t first, int64_t n, const int32_t* label_map,
                                                int n_labels, int32_t* est, float* score, int32_t* rank, float* p_true, int64_t* totals,
                                                int64_t* confusion, int64_t* rank_hist, const int64_t* image_offsets, int64_t n_images,
                                                const int32_t* source_of_image, int n_sources, int n_bins, int64_t* support, int64_t* nll_q32,
                                                int64_t* score_q32, int64_t* source_confusion, double* cover_sums, int64_t* n_images_used,
                                                int64_t* bin_count, int64_t* bin_correct, int64_t* bin_conf_q32, float* bin_conf_min,
                                                float* bin_conf_max, const int32_t* category_of_class, int n_categories, int64_t* cat_rows,
                                                int32_t* cat_n_bins, int64_t* cat_bin_count, int64_t* cat_bin_correct, int64_t* cat_bin_conf_q32,
                                                float* cat_bin_conf_min, float* cat_bin_conf_max, void* hip_stream)
{
    const EvalOut o{est, score, rank, p_true, totals, confusion, rank_hist};
    const GroupIO g = with_categories(group_io(image_offsets, n_images, source_of_image, n_sources, n_bins, support, nll_q32, score_q32,
                                               source_confusion, cover_sums, n_images_used, bin_count, bin_correct, bin_conf_q32, bin_conf_min,
                                               bin_conf_max),
                                      category_of_class, n_categories, cat_rows, cat_n_bins, cat_bin_count, cat_bin_correct, cat_bin_conf_q32,
                                      cat_bin_conf_min, cat_bin_conf_max);
    return evaluate(h, set_rows(fs, first, n), label_map, n_labels, o, &g, nullptr, hip_stream);
}

extern "C" int mmc_head_evaluate_ranked(mmc_head* h, const float* feats, const int32_t* y, int64_t n, const int32_t* label_map, int n_labels,
                                        int32_t* est, float* score, int32_t* rank, float* p_true, int64_t* totals, int64_t* confusion,
                                        int64_t* rank_hist, const uint8_t* sim_level, int n_levels, int kmax, int64_t* class_rank_hist,
                                        int64_t* hier_hist, unsigned flags, void* hip_stream)
{
    const EvalOut o{est, score, rank, p_true, totals, confusion, rank_hist};
    const RankIO k{sim_level, n_levels, kmax, class_rank_hist, hier_hist};
    return evaluate(h, host_rows(feats, y, n, flags), label_map, n_labels, o, nullptr, &k, hip_stream);
}

extern "C" int mmc_head_evaluate_ranked_set(mmc_head* h, mmc_featureset* fs, int64_t first, int64_t n, const int32_t* label_map, int n_labels,
                                            int32_t* est, float* score, int32_t* rank, float* p_true, int64_t* totals, int64_t* confusion,
                                            int64_t* rank_hist, const uint8_t* sim_level, int n_levels, int kmax, int64_t* class_rank_hist,
                                            int64_t* hier_hist, void* hip_stream)
{
    const EvalOut o{est, score, rank, p_true, totals, confusion, rank_hist};
    const RankIO k{sim_level, n_levels, kmax, class_rank_hist, hier_hist};
    return evaluate(h, set_rows(fs, first, n), label_map, n_labels, o, nullptr, &k, hip_stream);
}

// ------------------------------------------------------------------------------------------
// cover estimation: mmc_cover_proba / mmc_head_cover / mmc_head_cover_set (include/mmc.h, "cover estimation")
// ------------------------------------------------------------------------------------------
static_assert(MMC_COVER_MAX_CELLS <= (1LL << 31), "a cover call's cell count must keep every grid of cover.hip in range");
// the group arguments and outputs of the three cover entry points, in the order of include/mmc.h
struct CoverIO {
    const int64_t* offsets; int64_t n_groups; const double* train_prior; double strength; int iters;
    int64_t *count, *soft, *unusable; double* prior;
    int k; int32_t* idx; float* scores;
};

// zeroes every host output whose size the arguments determine
static void cover_clear(int K, int64_t n, const CoverIO& c, bool out_host)
{
    if (c.unusable && c.n_groups > 0 && c.n_groups <= MMC_COVER_MAX_CELLS) memset(c.unusable, 0, (size_t)c.n_groups * 8);   // (needs no K)
    if (K < 1) return;
    if (c.n_groups > 0 && c.n_groups <= MMC_COVER_MAX_CELLS / K) {
        const size_t cells = (size_t)c.n_groups * K;
        if (c.count) memset(c.count, 0, cells * 8);
        if (c.soft) memset(c.soft, 0, cells * 8);
        if (c.prior) memset(c.prior, 0, cells * 8);
    }
    if (out_host && c.idx && c.scores && c.k >= 1 && c.k <= K && n > 0 && n <= MMC_COVER_MAX_CELLS / K) {
        memset(c.idx, 0, (size_t)n * c.k * 4);
        memset(c.scores, 0, (size_t)n * c.k * 4);
    }
}

static int cover_check(int K, int64_t n, const CoverIO& c)
{
    if (K < 1) return fail(MMC_ERR_ARG, "K = %d must be positive", K);
    if (n < 0) return fail(MMC_ERR_ARG, "n = %lld is negative", (long long)n);
    if (n > MMC_COVER_MAX_CELLS / K)
        return fail(MMC_ERR_ARG, "n * K = %lld x %d resident probabilities: at most %lld cells per call", (long long)n, K, (long long)MMC_COVER_MAX_CELLS);
    if (c.n_groups < 0) return fail(MMC_ERR_ARG, "n_groups = %lld is negative", (long long)c.n_groups);
    if (c.n_groups > MMC_COVER_MAX_CELLS / K)
        return fail(MMC_ERR_ARG, "n_groups * K = %lld x %d table cells: at most %lld", (long long)c.n_groups, K, (long long)MMC_COVER_MAX_CELLS);
    if (c.n_groups > 0 && (!c.count || !c.soft || !c.unusable || !c.prior)) return fail(MMC_ERR_ARG, "count/soft_q32/unusable/prior is NULL");
    if (!(c.strength >= 0.0) || std::isinf(c.strength)) return fail(MMC_ERR_ARG, "strength = %g must be finite and >= 0", c.strength);
    if (c.iters < 0 || c.iters > MMC_COVER_MAX_ITERS) return fail(MMC_ERR_ARG, "iters = %d outside [0, %d]", c.iters, MMC_COVER_MAX_ITERS);
    if ((c.idx == nullptr) != (c.scores == nullptr)) return fail(MMC_ERR_ARG, "idx and scores come together or not at all");
    if (c.idx && (c.k < 1 || c.k > K)) return fail(MMC_ERR_ARG, "k = %d is outside [1, %d]", c.k, K);
    if (c.train_prior) {
        double sum = 0.0;
        for (int j = 0; j < K; ++j) {
            if (!(c.train_prior[j] > 0.0) || std::isinf(c.train_prior[j]))
                return fail(MMC_ERR_ARG, "train_prior[%d] = %g must be a positive finite number", j, c.train_prior[j]);
            sum += c.train_prior[j];
        }
        if (!(std::fabs(sum - 1.0) <= 1e-6)) return fail(MMC_ERR_ARG, "train_prior sums to %.9g: must be 1 within 1e-6", sum);
    }
    if (c.n_groups == 0) return n == 0 ? MMC_OK : fail(MMC_ERR_ARG, "no groups over %lld points", (long long)n);
    if (!c.offsets) return fail(MMC_ERR_ARG, "group_offsets is NULL");
    if (c.offsets[0] != 0) return fail(MMC_ERR_ARG, "group_offsets[0] = %lld: must be 0", (long long)c.offsets[0]);
    for (int64_t g = 0; g < c.n_groups; ++g)
        if (c.offsets[g + 1] < c.offsets[g])
            return fail(MMC_ERR_ARG, "group_offsets[%lld] = %lld is below group_offsets[%lld] = %lld", (long long)(g + 1),
                        (long long)c.offsets[g + 1], (long long)g, (long long)c.offsets[g]);
    if (c.offsets[c.n_groups] != n)
        return fail(MMC_ERR_ARG, "group_offsets[n_groups] = %lld: must be n = %lld", (long long)c.offsets[c.n_groups], (long long)n);
    return MMC_OK;
}

// a call without points: zero tables (cover_clear has run), train_prior in every row of prior; nothing is launched
static int cover_empty(int K, const CoverIO& c)
{
    for (int64_t g = 0; g < c.n_groups; ++g)
        for (int j = 0; j < K; ++j) c.prior[(size_t)g * K + j] = c.train_prior ? c.train_prior[j] : 1.0 / K;
    return MMC_OK;
}

// where the stage keeps its device state inside CoverScratch::dev (every part 256-byte aligned); the first `zero_bytes` are the
// integer tables a call starts from zero
struct CoverLayout { size_t count, soft, unusable, zero_bytes, offsets, slab_row0, slab_group, group_slab0, prior, pi, w, part, idx, scores, bytes; };
static CoverLayout cover_layout(int64_t n, int K, int64_t n_groups, int64_t n_slabs, int k_stage)
{
    CoverLayout L{};
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t o = at; at += (bytes + 255) / 256 * 256; return o; };
    const size_t cells = (size_t)n_groups * K;
    L.count = take(cells * 8);
    L.soft = take(cells * 8);
    L.unusable = take((size_t)n_groups * 8);
    L.zero_bytes = at;
    L.offsets = take((size_t)(n_groups + 1) * 8);
    L.slab_row0 = take((size_t)n_slabs * 8);
    L.slab_group = take((size_t)n_slabs * 4);
    L.group_slab0 = take((size_t)(n_groups + 1) * 8);
    L.prior = take((size_t)K * 8);
    L.pi = take(cells * 8);
    L.w = take(cells * 8);
    L.part = take((size_t)n_slabs * K * 8);
    L.idx = take((size_t)n * k_stage * 4);
    L.scores = take((size_t)n * k_stage * 4);
    L.bytes = at;
    return L;
}

// the stage on the resident probabilities P (n x K, n > 0, on the current device; every argument has been checked): enqueues the
// uploads, the count pass, the EM iterations and the adapted top-k on `st` and ends in one synchronisation
static int cover_stage(CoverScratch& S, const float* P, int64_t n, int K, const CoverIO& c, bool out_host, hipStream_t st)
{
    const int64_t G = c.n_groups;
    // the slab list: a function of the offsets alone
    S.slab_row0.clear(); S.slab_group.clear();
    S.group_slab0.resize((size_t)G + 1);
    for (int64_t g = 0; g < G; ++g) {
        S.group_slab0[g] = (int64_t)S.slab_row0.size();
        for (int64_t r = c.offsets[g]; r < c.offsets[g + 1]; r += COVER_SLAB_POINTS) {
            S.slab_row0.push_back(r);
            S.slab_group.push_back((int32_t)g);
        }
    }
    const int64_t n_slabs = (int64_t)S.slab_row0.size();
    S.group_slab0[G] = n_slabs;
    S.prior.resize(K);
    for (int j = 0; j < K; ++j) S.prior[j] = c.train_prior ? c.train_prior[j] : 1.0 / K;
    const bool topk = c.idx != nullptr;
    const CoverLayout L = cover_layout(n, K, G, n_slabs, topk && out_host ? c.k : 0);
    int r;
    if ((r = S.dev.reserve((int64_t)L.bytes))) return r;
    char* b = S.dev.p;
    auto* count = reinterpret_cast<unsigned long long*>(b + L.count);
    auto* soft = reinterpret_cast<unsigned long long*>(b + L.soft);
    auto* unusable = reinterpret_cast<unsigned long long*>(b + L.unusable);
    auto* offsets = reinterpret_cast<int64_t*>(b + L.offsets);
    auto* slab_row0 = reinterpret_cast<int64_t*>(b + L.slab_row0);
    auto* slab_group = reinterpret_cast<int32_t*>(b + L.slab_group);
    auto* group_slab0 = reinterpret_cast<int64_t*>(b + L.group_slab0);
    auto* prior = reinterpret_cast<double*>(b + L.prior);
    auto* pi = reinterpret_cast<double*>(b + L.pi);
    auto* w = reinterpret_cast<double*>(b + L.w);
    auto* part = reinterpret_cast<double*>(b + L.part);
    int32_t* didx = topk ? (out_host ? reinterpret_cast<int32_t*>(b + L.idx) : c.idx) : nullptr;
    float* dscores = topk ? (out_host ? reinterpret_cast<float*>(b + L.scores) : c.scores) : nullptr;
    const size_t cells = (size_t)G * K;
    HIP_TRY(hipMemsetAsync(b, 0, L.zero_bytes, st));
    HIP_TRY(hipMemcpyAsync(offsets, c.offsets, (size_t)(G + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(slab_row0, S.slab_row0.data(), (size_t)n_slabs * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(slab_group, S.slab_group.data(), (size_t)n_slabs * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(group_slab0, S.group_slab0.data(), (size_t)(G + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(prior, S.prior.data(), (size_t)K * 8, hipMemcpyHostToDevice, st));
    KTRY(launch_cover_count(P, n, K, offsets, G, count, soft, unusable, st));
    KTRY(launch_cover_em_init(prior, G, K, pi, w, st));
    for (int t = 0; t < c.iters; ++t) {
        KTRY(launch_cover_em_pass(P, K, slab_row0, slab_group, offsets, n_slabs, w, part, st));
        KTRY(launch_cover_em_reduce(part, group_slab0, offsets, unusable, prior, c.strength, G, K, pi, w, st));
    }
    if (topk) KTRY(launch_cover_adapt_topk(P, n, K, offsets, G, w, c.k, didx, dscores, st));
    HIP_TRY(hipMemcpyAsync(c.count, count, cells * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(c.soft, soft, cells * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(c.unusable, unusable, (size_t)G * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(c.prior, pi, cells * 8, hipMemcpyDeviceToHost, st));
    if (topk && out_host) {
        HIP_TRY(hipMemcpyAsync(c.idx, didx, (size_t)n * c.k * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(c.scores, dscores, (size_t)n * c.k * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return MMC_OK;
}

// mmc_cover_proba has no handle: its scratch is kept per device for the life of the process (never freed: the runtime may be gone
// by the time static destructors run), and the calls are serialised
static std::mutex g_cover_mutex;
static std::map<int, CoverScratch*>* g_cover_scratch = nullptr;

extern "C" int mmc_cover_proba(const float* proba, int64_t n, int K, const int64_t* group_offsets, int64_t n_groups,
                               const double* train_prior, double strength, int iters, int64_t* count, int64_t* soft_q32, int64_t* unusable,
                               double* prior, int k, int32_t* idx, float* scores, int device, unsigned flags, void* hip_stream)
{
    const CoverIO c{group_offsets, n_groups, train_prior, strength, iters, count, soft_q32, unusable, prior, k, idx, scores};
    const bool out_host = (flags & MMC_OUT_HOST) != 0;
    cover_clear(K, n, c, out_host);
    int r = cover_check(K, n, c);
    if (r) return r;
    if (n == 0) return cover_empty(K, c);
    if (!proba) return fail(MMC_ERR_ARG, "proba is NULL");
    if ((r = check_device(device))) return r;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::lock_guard<std::mutex> lock(g_cover_mutex);
    HIP_TRY(hipSetDevice(device));
    if (!g_cover_scratch) g_cover_scratch = new std::map<int, CoverScratch*>();
    CoverScratch*& S = (*g_cover_scratch)[device];
    if (!S) S = new CoverScratch();
    const float* P = proba;
    if (flags & MMC_IN_HOST) {
        if ((r = S->proba.reserve(n * K))) return r;
        HIP_TRY(hipMemcpyAsync(S->proba.p, proba, (size_t)n * K * 4, hipMemcpyHostToDevice, st));
        P = S->proba.p;
    }
    r = cover_stage(*S, P, n, K, c, out_host, st);
    if (r) cover_clear(K, n, c, out_host);
    return r;
}

// the two head forms: rows X (host with MMC_IN_HOST in `flags`, else on the head's device), or rows [first, ...) of `fs` when `set`
static int head_cover(mmc_head* h, const float* X, const mmc_featureset* fs, bool set, int64_t first, int64_t n_points, int G,
                      const CoverIO& c, unsigned flags, void* hip_stream)
{
    const bool out_host = (flags & MMC_OUT_HOST) != 0;
    const int K = h ? h->K : 0;
    cover_clear(K, n_points, c, out_host);
    if (!h) return fail(MMC_ERR_ARG, "head handle is NULL");
    if (G < 1 || G > VIEWS_MAX) return fail(MMC_ERR_ARG, "G = %d views per point is outside [1, %d]", G, VIEWS_MAX);
    int r = cover_check(K, n_points, c);
    if (r) return r;
    const int64_t n = n_points * G;   // rows
    if (set) {
        if (!fs) return fail(MMC_ERR_ARG, "feature set handle is NULL");
        if (fs->dim != h->input_dim) return fail(MMC_ERR_ARG, "feature set has %d columns, head expects %d", fs->dim, h->input_dim);
        if (fs->device != h->device) return fail(MMC_ERR_ARG, "feature set is on device %d, head on device %d", fs->device, h->device);
        if (first < 0 || first > fs->n || n > fs->n - first)
            return fail(MMC_ERR_ARG, "rows [%lld, %lld + %lld) outside the set's %lld rows", (long long)first, (long long)first, (long long)n,
                        (long long)fs->n);
    }
    if (n_points == 0) return cover_empty(K, c);
    if (!set && !X) return fail(MMC_ERR_ARG, "feats is NULL");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(h->device));
    const int64_t chunk = HEAD_CHUNK / G * G;   // rows: whole points only
    if ((r = h->cover.proba.reserve(n_points * K))) return r;
    if (G > 1) {   // launch_mean_topk always selects: its best class per point goes to the top-k staging and is not used
        const int64_t stage = n_points < chunk / G ? n_points : chunk / G;
        if ((r = h->topk_idx_stage.reserve(stage)) || (r = h->topk_score_stage.reserve(stage))) return r;
    }
    float* resident = h->cover.proba.p;
    const float* rows = set ? fs->X + (size_t)first * fs->dim : X;
    r = head_for_chunks(h, rows, n, set ? 0u : flags & MMC_IN_HOST, st, [&](int64_t off, int cur, const float* logits) -> int {
        if (G == 1)
            KTRY(launch_calibrate(logits, cur, K, h->a, h->bc, resident + (size_t)off * K, nullptr, st));
        else
            KTRY(launch_mean_topk(logits, cur / G, G, K, h->a, h->bc, 1, h->topk_idx_stage.p, h->topk_score_stage.p,
                                  resident + (size_t)(off / G) * K, h->proba_stage.p, st));
        return MMC_OK;
    }, chunk);
    if (!r) r = cover_stage(h->cover, resident, n_points, K, c, out_host, st);
    if (r) cover_clear(K, n_points, c, out_host);
    return r;
}

extern "C" int mmc_head_cover(mmc_head* h, const float* feats, int64_t n_points, int G, const int64_t* group_offsets, int64_t n_groups,
                              const double* train_prior, double strength, int iters, int64_t* count, int64_t* soft_q32, int64_t* unusable,
                              double* prior, int k, int32_t* idx, float* scores, unsigned flags, void* hip_stream)
{
    const CoverIO c{group_offsets, n_groups, train_prior, strength, iters, count, soft_q32, unusable, prior, k, idx, scores};
    return head_cover(h, feats, nullptr, false, 0, n_points, G, c, flags, hip_stream);
}

extern "C" int mmc_head_cover_set(mmc_head* h, mmc_featureset* fs, int64_t first, int64_t n_points, int G, const int64_t* group_offsets,
                                  int64_t n_groups, const double* train_prior, double strength, int iters, int64_t* count, int64_t* soft_q32,
                                  int64_t* unusable, double* prior, int k, int32_t* idx, float* scores, unsigned flags, void* hip_stream)
{
    const CoverIO c{group_offsets, n_groups, train_prior, strength, iters, count, soft_q32, unusable, prior, k, idx, scores};
    return head_cover(h, nullptr, fs, true, first, n_points, G, c, flags, hip_stream);
}

// ------------------------------------------------------------------------------------------
// patches -> backbone -> head -> top-k
// ------------------------------------------------------------------------------------------
extern "C" int mmc_classify_patches(mmc_backbone* bb, mmc_head* h, const void* patches, int64_t n, int k, int32_t* idx,
                                    float* scores, unsigned flags, void* hip_stream)
{
    if (!bb) return fail(MMC_ERR_ARG, "backbone handle is NULL");
    if (!h) return fail(MMC_ERR_ARG, "head handle is NULL");
    if (mmc_backbone_device(bb) != h->device)
        return fail(MMC_ERR_ARG, "backbone lives on device %d, head on device %d", mmc_backbone_device(bb), h->device);
    if (mmc_feature_dim(bb) != h->input_dim)
        return fail(MMC_ERR_ARG, "backbone feature_dim %d != head input_dim %d", mmc_feature_dim(bb), h->input_dim);
    if (n < 0) return fail(MMC_ERR_ARG, "n = %lld is negative", (long long)n);
    if (k < 1 || k > h->K) return fail(MMC_ERR_ARG, "k = %d is outside [1, %d] (the head has %d classes)", k, h->K, h->K);
    if (n == 0) return MMC_OK;
    if (!patches) return fail(MMC_ERR_ARG, "patches is NULL");
    if (!idx || !scores) return fail(MMC_ERR_ARG, "idx/scores is NULL");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(h->device));
    int r = h->cls_feats.reserve((n < CLASSIFY_CHUNK ? n : CLASSIFY_CHUNK) * h->input_dim);
    if (r) return r;
    const size_t psz = (size_t)MMC_PATCH * MMC_PATCH * 3;
    const uint8_t* in = static_cast<const uint8_t*>(patches);
    for (int64_t off = 0; off < n; off += CLASSIFY_CHUNK) {
        const int64_t cur = (n - off) < CLASSIFY_CHUNK ? (n - off) : CLASSIFY_CHUNK;
        if ((r = mmc_backbone_extract(bb, in + (size_t)off * psz, cur, h->cls_feats.p, flags & MMC_IN_HOST, st))) return r;
        if ((r = mmc_head_topk(h, h->cls_feats.p, cur, k, idx + (size_t)off * k, scores + (size_t)off * k, nullptr, flags & MMC_OUT_HOST, st)))
            return r;
    }
    return MMC_OK;
}

extern "C" int mmc_classify_patches_views(mmc_backbone* bb, mmc_head* h, const void* patches, int64_t n_points, int G, int k, int32_t* idx,
                                          float* scores, unsigned flags, void* hip_stream)
{
    if (G < 1 || G > VIEWS_MAX) return fail(MMC_ERR_ARG, "G = %d views per point is outside [1, %d]", G, VIEWS_MAX);
    if (k < 1) return fail(MMC_ERR_ARG, "k = %d must be at least 1", k);
    if (!bb) return fail(MMC_ERR_ARG, "backbone handle is NULL");
    if (!h) return fail(MMC_ERR_ARG, "head handle is NULL");
    if (mmc_backbone_device(bb) != h->device)
        return fail(MMC_ERR_ARG, "backbone lives on device %d, head on device %d", mmc_backbone_device(bb), h->device);
    if (mmc_feature_dim(bb) != h->input_dim)
        return fail(MMC_ERR_ARG, "backbone feature_dim %d != head input_dim %d", mmc_feature_dim(bb), h->input_dim);
    if (n_points < 0) return fail(MMC_ERR_ARG, "n_points = %lld is negative", (long long)n_points);
    if (k > h->K) return fail(MMC_ERR_ARG, "k = %d is outside [1, %d] (the head has %d classes)", k, h->K, h->K);
    if (n_points == 0) return MMC_OK;
    if (!patches) return fail(MMC_ERR_ARG, "patches is NULL");
    if (!idx || !scores) return fail(MMC_ERR_ARG, "idx/scores is NULL");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipSetDevice(h->device));
    const int64_t chunk = CLASSIFY_CHUNK / G * G, n = n_points * G;   // patches: whole points only
    int r = h->cls_feats.reserve((n < chunk ? n : chunk) * h->input_dim);
    if (r) return r;
    const size_t psz = (size_t)MMC_PATCH * MMC_PATCH * 3;
    const uint8_t* in = static_cast<const uint8_t*>(patches);
    for (int64_t off = 0; off < n; off += chunk) {
        const int64_t cur = (n - off) < chunk ? (n - off) : chunk, p0 = off / G;
        if ((r = mmc_backbone_extract(bb, in + (size_t)off * psz, cur, h->cls_feats.p, flags & MMC_IN_HOST, st))) return r;
        if ((r = mmc_head_topk_views(h, h->cls_feats.p, cur / G, G, k, idx + (size_t)p0 * k, scores + (size_t)p0 * k, nullptr,
                                     flags & MMC_OUT_HOST, st)))
            return r;
    }
    return MMC_OK;
}
