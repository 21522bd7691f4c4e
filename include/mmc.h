/*
 * mmc.h -- C ABI of libmermaid_mi355.so: the MI355X (gfx950) implementation of the
 * PySpacer EfficientNet patch feature-extraction path of data-mermaid/mermaid-classifier.
 *
 * The reference has no FFI; its "plugin API" for this path is a Python class contract
 * plus three file artifacts.  Every entry point below names the reference
 * interface it replaces.  Plain C: no exceptions cross the boundary, every call returns an
 * int status (0 = MMC_OK) and mmc_last_error() returns a thread-local message.
 * All buffers are caller-owned; handles are opaque; streams are explicit (hipStream_t
 * passed as void*, NULL = the default stream).  No torch types appear here.
 */
#ifndef MMC_H
#define MMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMC_OK 0
#define MMC_ERR_ARG 1      /* bad argument / shape (ValueError on the Python side) */
#define MMC_ERR_WEIGHTS 2  /* packed weights blob malformed (KeyError/ValueError) */
#define MMC_ERR_HIP 3      /* HIP runtime failure (RuntimeError) */
#define MMC_ERR_NOMEM 4

#define MMC_ARCH_B0 0   /* efficientnet-b0: the network pyspacer's EfficientNetExtractor builds (the reference path) */
#define MMC_ARCH_B4 1   /* efficientnet-b4 (width 1.4, depth 1.8) on 224x224 patches: BASELINE.json configs[4]; not in the
                         * reference; fused expand+depthwise kernels plus the shape-generic squeeze-excite / project / head kernels, feature_dim 1792 */

/* memory-kind flags for mmc_backbone_extract / mmc_head_predict / mmc_head_topk / mmc_classify_patches / mmc_crop_patches */
#define MMC_IN_DEVICE 0u
#define MMC_IN_HOST 1u   /* `patches`/`feats`/`image` is host memory: staged with hipMemcpyAsync */
#define MMC_OUT_DEVICE 0u
#define MMC_OUT_HOST 2u  /* outputs are host memory; the call synchronises the stream before returning */

#define MMC_FEATURE_DIM_B0 1280
#define MMC_FEATURE_DIM_B4 1792
#define MMC_PATCH 224

typedef struct mmc_backbone mmc_backbone;
typedef struct mmc_head mmc_head;

/* ---- library ------------------------------------------------------------------------ */
const char* mmc_last_error(void);
int mmc_version(void);          /* ABI version, currently 1 */
int mmc_device_count(void);     /* number of visible HIP devices (0 when none) */

/* ---- backbone ------------------------------------------------------------------------
 * Replaces: EfficientNetExtractor.load_weights(stream) + net.to(device).eval()
 *   (reference scripts/build_feature_bucket.py:402-413) and
 *   net.extract_features(batch) (scripts/build_feature_bucket.py:430-437), including the
 *   per-patch transformation() (ToTensor + Normalize, :420-423), which is folded into the
 *   stem kernel: the library takes raw u8 HWC patches.
 *
 * `packed` is the blob produced by mermaid_classifier_amd.weights.pack_backbone():
 *   header  { char magic[4]="MMCW"; u32 version=1; u32 arch; u32 n_tensors; }
 *   table   n_tensors x { u64 offset; u64 nbytes; }          (offsets from blob start, 256-B aligned)
 *   tensors in the fixed order documented in mermaid_classifier_amd/weights.py
 *   (BN folded: fp16 GEMM weights in MFMA-row-permuted [Np][Kp] layout, fp32 biases,
 *    fp32 depthwise taps [k*k][C], fp32 squeeze-excite matrices).
 * The blob is copied to device memory; the caller may free it after the call.
 * `max_batch` bounds the activation workspace (patches processed per internal pass).
 */
int mmc_backbone_create(const void* packed, size_t nbytes, int arch, int device, int max_batch,
                        mmc_backbone** out);
/* The same with `flags`.  MMC_PRECISION_FP8 (MMC_ARCH_B4 only; BASELINE.json configs[4], not in the reference): the squeeze-excite
 * gated project convs of the 7x7 stage (env MMC_FP8_MAXH=14: of the 14x14 stages too) run on OCP e4m3 operands
 * (v_mfma_scale_f32_16x16x128_f8f6f4, fp32 accumulation): weights quantised at create time with one scale per output channel,
 * activations in the kernel with one scale per pixel.  Everything else stays fp16 storage / fp32 accumulation.  Accuracy is that of
 * the operand format, not the fp16 gates: feature cosine >= 0.997 against the fp32 oracle on image-like patches (the floor the
 * tests hold it to, and the one INTEGRATION.md states; measured 0.9982 - 0.9996). */
#define MMC_PRECISION_FP8 1u
int mmc_backbone_create_ex(const void* packed, size_t nbytes, int arch, int device, int max_batch, unsigned flags,
                           mmc_backbone** out);
/* fp32 -> OCP e4m3fn bytes (round to nearest even, saturating at +-448): the encoding the fp8 weights are stored in.  Host code,
 * no device needed; exported so that tests can check it against an independent implementation. */
int mmc_fp8_e4m3_encode(const float* in, uint8_t* out, size_t n);
void mmc_backbone_destroy(mmc_backbone* bb);
int mmc_feature_dim(const mmc_backbone* bb);            /* 1280 for B0, 1792 for B4 */
int mmc_backbone_max_batch(const mmc_backbone* bb);
/* A pass is split into this many sub-batches that run concurrently on internal HIP streams (forked from and
 * joined to `hip_stream`); env MMC_LANES overrides the default of 2.  Results do not depend on it. */
int mmc_backbone_lanes(const mmc_backbone* bb);
size_t mmc_backbone_workspace_bytes(const mmc_backbone* bb);

/* patches: n x 224 x 224 x 3 u8 (HWC, RGB).  out_features: n x feature_dim fp32, row i = patch i.
 * flags: MMC_IN_HOST | MMC_OUT_HOST select host pointers; default both device pointers.
 * Asynchronous on `hip_stream` unless MMC_OUT_HOST is set.  One pass at a time per handle (the reference's forward path
 * is single-threaded: scripts/build_feature_bucket.py, "one extractor instance per process"): concurrent calls on one
 * handle are serialised by a per-handle mutex, and a call that comes in on a different stream than the previous one first
 * waits (on the device) for that call's work, because the workspace is shared.  For concurrency create one handle per
 * stream.
 * When the same (patches, out_features, n) combination comes in repeatedly the pass is captured into a HIP graph
 * once and replayed on `hip_stream` afterwards (env MMC_GRAPH=0 disables); results are identical either way.  The 32
 * most recently used combinations keep their graph.  A combination whose graph was evicted runs as plain launches from
 * then on (it is not captured a second time), and after 32 evictions -- one full turnover of the cache -- no further
 * combination is captured: a caller that cycles through more buffers than the cache holds pays plain launches, never a
 * capture per call. */
int mmc_backbone_extract(mmc_backbone* bb, const void* patches, int64_t n, float* out_features,
                         unsigned flags, void* hip_stream);

/* Debug hook for the graph cache above: stats[0] = graphs captured so far, stats[1] = graphs evicted so far,
 * stats[2] = graphs cached now.  (No reference counterpart: the reference has no launch graphs.) */
int mmc_backbone_graph_stats(mmc_backbone* bb, int64_t stats[3]);

/* Debug/parity hook: copy one intermediate activation of the LAST internal pass to host.
 * name: "stem", "b<i>.expand", "b<i>.dw", "b<i>.gate", "b<i>.out".  fp16 NHWC tensors are returned
 * as fp32 NHWC; gates as fp32 (n,C).  `capacity` = number of floats available in `out`;
 * *n_written receives the element count.  Requires MMC_KEEP_ACTIVATIONS=1 at create time
 * (separate buffers per layer); used only by the parity tests. */
int mmc_backbone_read_activation(mmc_backbone* bb, const char* name, float* out, size_t capacity,
                                 size_t* n_written);

/* Kernel timing hook for bench.py: runs `iters` passes over `n` resident patches and returns the
 * HIP-event elapsed milliseconds of every launch ("<layer>|<kernel instantiation>"), measured on `hip_stream`.
 * Sub-batches (see mmc_backbone_lanes) are run one after the other here, so each layer appears once per lane
 * with ceil(n / lanes) patches.
 * names/ms arrays have `cap` slots; *n_out receives the number filled. */
int mmc_backbone_profile(mmc_backbone* bb, const void* patches_dev, int64_t n, float* out_features_dev,
                         void* hip_stream, char (*names)[64], float* ms, int* launches, int cap, int* n_out);

/* ---- GPU crop front-end ---------------------------------------------------------------
 * Replaces: pyspacer crop_patches(image, rowcols, 224) as called by FeatureExtractor.__call__
 *   (reached from scripts/build_feature_bucket.py:775 and
 *    mermaid_classifier/pyspacer/annotation.py:241): reflect-pad by 224, slice 224x224 around
 *   each (row,col).  Implemented as index arithmetic on the resident image (no padded copy).
 * image: H x W x 3 u8; rowcols: n x 2 int32 (row, col); patches_out: n x 224 x 224 x 3 u8 (device).
 * Points must lie inside the image: host points (MMC_IN_HOST) outside it are rejected with MMC_ERR_ARG; device-resident
 * points cannot be inspected by the host and are clamped into the image by the kernel (never an out-of-bounds read).
 * With MMC_IN_HOST and few points on a big image (n * 150528 * 6 <= image bytes -- the reference's data: 10-25 points on a
 * 27 MP image) the patches are cut on the host (same index arithmetic, up to 4 threads, into a pinned ring slot) and only
 * they are uploaded; otherwise the image is uploaded and crop_kernel cuts them.  Same bytes either way.  The host image is
 * fully consumed before the call returns; the upload is asynchronous on `hip_stream`.  Env MMC_CROP_HOST=0/1 forces a path. */
int mmc_crop_patches(const void* image, int height, int width, const int32_t* rowcols, int64_t n,
                     void* patches_out_dev, unsigned flags, int device, void* hip_stream);

/* ---- patch views -----------------------------------------------------------------------
 * No reference counterpart (the reference cuts one fixed window per point): the eight orientations of a patch and a 2x context
 * crop, so that a frozen backbone can be shown a point several ways (averaged by mmc_head_topk_views, or appended to a
 * training set as extra rows).
 * A view is an integer v in 0..15 with r = v & 3, f = (v >> 2) & 1, z = (v >> 3) & 1.  For a point (row, col):
 *   base patch B (224 x 224 x 3 u8)
 *     z = 0: the patch of mmc_crop_patches, with its bytes.
 *     z = 1: the 448 x 448 window Wn of rows row-224 .. row+223 and columns col-224 .. col+223, indexed with numpy 'reflect'
 *            (i < 0 -> -i, i >= n -> 2(n-1)-i; one reflection suffices because both image dimensions must exceed 224), reduced
 *            2:1 per channel in integers:
 *            B[y,x,c] = (Wn[2y,2x,c] + Wn[2y,2x+1,c] + Wn[2y+1,2x,c] + Wn[2y+1,2x+1,c] + 2) >> 2.
 *   orientation
 *     P = np.rot90(B[:, ::-1] if f else B, k=r, axes=(0, 1)).
 * View 0 is the patch of mmc_crop_patches.
 *
 * mmc_crop_patches_views: patch i is view views[i] of point i (a caller who wants G views of a point lists it G times).
 * `views` (n codes, or NULL = all 0) lives where `rowcols` lives: host memory under MMC_IN_HOST, else device memory.  Host codes
 * above 15 are rejected with MMC_ERR_ARG naming the index; device codes are masked to 4 bits by the kernel (as device points are
 * clamped).  Everything else -- the point checks, the choice between the host cut and upload + kernel, streams -- is as in
 * mmc_crop_patches, and the three routes give the same bytes for every view. */
#define MMC_VIEWS_MAX 16   /* view codes 0 .. 15; also the most rows (views) per point of mmc_head_topk_views */
int mmc_crop_patches_views(const void* image, int height, int width, const int32_t* rowcols, int64_t n,
                           const uint8_t* views /* n codes, NULL = all 0 */, void* patches_out_dev,
                           unsigned flags, int device, void* hip_stream);

/* ---- calibrated MLP head -------------------------------------------------------------
 * Replaces: CalibratedHead.forward (mermaid_classifier/pyspacer/inference/head.py:66-89) as run by
 *   Predictor.predict_proba (mermaid_classifier/pyspacer/inference/loader.py:30-35).
 * W[l]: (dims[l+1], dims[l]) row-major fp32 (torch nn.Linear layout); b[l]: (dims[l+1]);
 * dims has n_layers+1 entries, dims[n_layers] == K; a, bcal: (K) Platt parameters.  All host pointers.
 */
int mmc_head_create(const float* const* W, const float* const* b, const int* dims, int n_layers,
                    const float* a, const float* bcal, int K, int device, mmc_head** out);
void mmc_head_destroy(mmc_head* h);
int mmc_head_input_dim(const mmc_head* h);
int mmc_head_num_classes(const mmc_head* h);
/* feats: n x input_dim fp32; proba: n x K fp32; argmax: n int32 (may be NULL). */
int mmc_head_predict(mmc_head* h, const float* feats, int64_t n, float* proba, int32_t* argmax,
                     unsigned flags, void* hip_stream);

/* The k best classes per row instead of (or next to) the probabilities.
 * Replaces: mermaid_classifier/pyspacer/annotation.py:251-261 (predict_proba + per-point sorted(...)[:k]): row i of idx / scores
 *   holds the class indices and calibrated probabilities of sorted(zip(labels, proba_i), key=itemgetter(1), reverse=True)[:k] --
 *   score descending and, the sort being stable, equal scores in class order; k is the reference's predictions_per_point
 *   (annotation.py:231-233).  The probabilities are those of mmc_head_predict, bit for bit (same launches for the Linear layers, same
 *   calibration arithmetic); the selection runs in the calibration kernel, so nothing but n x k indices and scores has to leave the device.
 * feats: n x input_dim fp32; idx: n x k int32; scores: n x k fp32; proba: n x K fp32 or NULL.  1 <= k <= K.
 * flags: MMC_IN_HOST for feats, MMC_OUT_HOST for idx / scores / proba together.  Asynchronous on `hip_stream` unless MMC_OUT_HOST is set.
 * Rows with NaN features still get k distinct classes in [0, K); their order is unspecified (as Python's sorted leaves it). */
int mmc_head_topk(mmc_head* h, const float* feats, int64_t n, int k,
                  int32_t* idx /* n x k */, float* scores /* n x k */, float* proba /* n x K or NULL */,
                  unsigned flags, void* hip_stream);

/* ---- patches -> labels in one call ------------------------------------------------------
 * Replaces: the device work of AnnotationRun.__init__ (mermaid_classifier/pyspacer/annotation.py:241-261): extractor(image, rowcols)
 *   -> get_array per point -> predict_proba -> sorted(...)[:k], for patches already cut (mmc_crop_patches cuts them).
 * patches (n x 224 x 224 x 3 u8) -> backbone -> head -> top-k on one stream; features stay in a device buffer owned by
 * the head handle (grown on demand, stable between calls so the backbone's graph cache keeps hitting): no allocation per call in
 * the steady state.  More than 4096 patches are worked through in chunks of 4096, so the same (patches chunk, feature buffer, n)
 * combinations recur and the graph cache documented at mmc_backbone_extract applies.  The handles must live on one device and
 * mmc_feature_dim must equal mmc_head_input_dim.  flags: MMC_IN_HOST for patches, MMC_OUT_HOST for idx / scores (the only
 * data copied back); asynchronous unless MMC_OUT_HOST is set.  Same bits as mmc_backbone_extract + mmc_head_topk. */
int mmc_classify_patches(mmc_backbone* bb, mmc_head* h, const void* patches, int64_t n, int k,
                         int32_t* idx, float* scores, unsigned flags, void* hip_stream);

/* ---- the mean over a point's views, then top-k ---------------------------------------------
 * Rows p*G .. p*G+G-1 of feats (or patches) are the G views of point p, 1 <= G <= 16.  Per point and class the value is
 *   m = (v_0 + v_1 + ... + v_{G-1}) / (float)G      in fp32, summed left to right in view order,
 * with v_g the probability mmc_head_predict writes for that row, bit for bit.  The k best classes of m are chosen as mmc_head_topk
 * chooses them (score descending, equal scores in class order, k distinct classes even for NaN rows); with G = 1 the outputs have
 * the bits of mmc_head_topk / mmc_classify_patches.  idx, scores: n_points x k; proba: the n_points x K means, or NULL.
 * Internal chunks hold whole points only (the head's row chunk and the 4096-patch chunk are rounded down to multiples of G).
 * Flags, streams, the feature buffer and the graph-cache behaviour are those of mmc_head_topk / mmc_classify_patches. */
int mmc_head_topk_views(mmc_head* h, const float* feats /* (n_points*G) x input_dim, point-major */, int64_t n_points, int G, int k,
                        int32_t* idx /* n_points x k */, float* scores /* n_points x k */, float* proba /* n_points x K or NULL */,
                        unsigned flags, void* hip_stream);
int mmc_classify_patches_views(mmc_backbone* bb, mmc_head* h, const void* patches /* (n_points*G) x 224x224x3 */,
                               int64_t n_points, int G, int k, int32_t* idx, float* scores, unsigned flags, void* hip_stream);

/* ---- MLP classifier training on precomputed feature vectors --------------------------------
 * Replaces: the arithmetic of TorchMLPClassifier.partial_fit (mermaid_classifier/pyspacer/torch_classifier.py:226-303)
 *   as driven by the trainer's batch loop (mermaid_classifier/pyspacer/trainer.py:138-145): per mini-batch
 *   logits -> F.cross_entropy(weight=class_weight) + (0.5*alpha/mb)*sum(W^2) -> backward -> torch.optim.Adam.step().
 * The host side keeps what the reference keeps on the host: classes_/label lookup, Glorot initialisation (torch RNG, so
 * the same random_state gives the same initial weights), the shuffle order, loss_curve_/n_iter_ bookkeeping.
 * W[l]: (dims[l+1], dims[l]) row-major fp32, b[l]: (dims[l+1]) -- the initial parameters (host pointers);
 * class_weight: K floats in classes_ order or NULL; Adam moments start at zero, step count at 0.
 * Hyper-parameters are doubles because torch derives its fp32 scalars (1 - beta, lr / bias_correction, alpha / mb) from
 * python floats: (float)(1.0 - 0.9) is not 1.0f - 0.9f. */
typedef struct mmc_trainer mmc_trainer;
int mmc_trainer_create(const float* const* W, const float* const* b, const int* dims, int n_layers, double lr, double beta1,
                       double beta2, double eps, double alpha, const float* class_weight, int device, mmc_trainer** out);
void mmc_trainer_destroy(mmc_trainer* t);
/* One pass over n samples ALREADY IN VISITING ORDER (the caller applies the shuffle, torch_classifier.py:251-257):
 * X n x dims[0] fp32 and y n int32 class indices, host pointers; mini-batches of `batch_size` rows (last one ragged),
 * one Adam step each.  *avg_loss = sum(loss_i * mb_i) / n, the value the reference appends to loss_curve_ (:293-300).
 * Synchronises `hip_stream` before returning. */
int mmc_trainer_partial_fit(mmc_trainer* t, const float* X, const int32_t* y, int64_t n, int batch_size, double* avg_loss,
                            void* hip_stream);
/* The same with the visiting order applied on the device: X / y in their natural order plus `order` (n int64 row indices:
 * position i of the pass visits row order[i]); NULL order = mmc_trainer_partial_fit.  Needs dims[0] % 4 == 0. */
int mmc_trainer_partial_fit_ordered(mmc_trainer* t, const float* X, const int32_t* y, const int64_t* order, int64_t n,
                                    int batch_size, double* avg_loss, void* hip_stream);
/* Current parameters to host buffers shaped like the create-time ones. */
int mmc_trainer_get_params(mmc_trainer* t, float* const* W, float* const* b);
/* Adam moments (which = 0: exp_avg, 1: exp_avg_sq) and step count, read (set = 0) or written (set = 1): what the
 * reference pickles as the optimizer state dict (torch_classifier.py:404-415). */
int mmc_trainer_adam_state(mmc_trainer* t, int which, int set, float* const* W, float* const* b, long long* step);
/* Raw logits of the current parameters: X n x dims[0] host -> logits n x K host (the softmax / float64 renormalisation of
 * _forward_probs, torch_classifier.py:332-376, stays on the host; mmc_calibrator_add_features / mmc_trainer_evaluate below do it on
 * the device). */
int mmc_trainer_logits(mmc_trainer* t, const float* X, int64_t n, float* logits, void* hip_stream);
/* The loss formulation of the trainer's steps: label smoothing, focal modulation and a logit prior, each a per-trainer option.
 * Extends: the F.cross_entropy(weight=class_weight) of a step (torch_classifier.py:278), the only loss the reference has, to what its
 *   research reports point at next (docs/research/hidden-layer-experiments.md:119, docs/research/balancing-experiments.md:96-100, 142).
 * With logits z (the last Linear's output), t = y_i, class weights w (ones when none), logit_prior o (zeros when NULL),
 *   eps = label_smoothing and gamma = focal_gamma, a mini-batch's data term is
 *     u      = z + o                                   (fp32 add; inside the loss only)
 *     logp_c = u_c - max u - log sum_c exp(u_c - max u),  p_t = exp(logp_t),  nll = -logp_t,  q = 1 - p_t,  m = q^gamma  (gamma = 0: m = 1)
 *     l_i    = (1 - eps) w_t m nll + (eps / K) sum_c w_c (-logp_c)
 *     L      = sum_i l_i / sum_i w[y_i]                 (+ the L2 term, unchanged)
 *   gamma = 0: torch's F.cross_entropy(weight=w, label_smoothing=eps) exactly; eps = 0, gamma > 0: the weighted focal loss
 *   (Lin et al. 2017) over the weight sum; o: the logit-adjusted loss (Menon et al. 2021).  The gradient written is the derivative of
 *   L: with g = 1 / sum_i w[y_i], W = sum_c w_c and f = m + gamma p_t q^(gamma-1) nll,
 *     dL/dz_c = g [ (1 - eps) w_t f (p_c - [c == t]) + (eps / K) (p_c W - w_c) ].
 *   The kernel's fp32 scalars are (float)(1.0 - eps), (float)(eps / K), (float)gamma and W as the float of the double sum of the fp32
 *   weights in class order (K without weights); q is sum_{c != t} e_c / sum_c e_c, so rows whose p_t rounds to 1 or to 0 give finite
 *   losses and gradients.  Evaluation, calibration, mmc_trainer_logits and export read the raw logits: none of the three options.
 * Allowed between passes.  Checked before anything changes: a NULL trainer, label_smoothing outside [0, 1), focal_gamma other than 0 or
 *   [1, 8] (below 1, q^(gamma-1) is unbounded at saturated rows), a non-finite logit_prior entry (K floats in classes_ order, host, copied)
 *   -> MMC_ERR_ARG, and the trainer is as it was.  (0, 0, NULL) restores the plain loss.
 * Bits: all defaults run the kernel instantiation, and give the bits, of a trainer this was never called on; any other setting runs the
 *   general instantiation, whose row sums have a fixed order (no atomics), so passes stay bit-reproducible, solo and grouped alike. */
int mmc_trainer_set_loss(mmc_trainer* t, double label_smoothing, double focal_gamma, const float* logit_prior /* K or NULL */);
/* The loss stage of a step on caller logits: logits n x K fp32 and y n class indices (host) -> dlogits n x K, the gradient of the
 * data term above, and row_loss n, the per-row terms l_i g (host).  It launches the step's own kernel with the trainer's class
 * weights and loss options and g = 1 / sum of w[y_i] over these n rows, as a step derives it -- for callers who bring their own
 * logits, and for checking the loss stage per element.  Parameters, moments and step count are not touched.
 * Checked before anything is launched: NULL arguments, n outside [1, 16384], a label outside [0, K), a zero total weight
 * -> MMC_ERR_ARG.  Synchronises `hip_stream` before returning.  Same bits as the loss stage of a step on the same rows. */
int mmc_trainer_loss_gradient(mmc_trainer* t, const float* logits, const int32_t* y, int64_t n, float* dlogits, float* row_loss,
                              void* hip_stream);

/* ---- evaluation and Platt calibration of the trained classifier ------------------------------------------------------
 * Replaces the host steps the reference's MermaidTrainer takes after partial_fit, all fed there by predict_proba:
 *   mmc_trainer_evaluate: _calc_acc_batched (mermaid_classifier/pyspacer/trainer.py:295-307) and
 *     _calc_acc_and_log_loss_batched (:309-342) -- accuracy_score and sklearn.metrics.log_loss(labels=classes_) of predict_proba;
 *   mmc_calibrator_*: _calibrate_in_batches (:344-396) -- sklearn.calibration._fit_calibrator(clf, predict_proba, y, classes_,
 *     "sigmoid"): one Platt sigmoid per class (objective and start point of _sigmoid_calibration; damped Newton in fp64 on the
 *     device).  The calibrated model is then served by mmc_head_* with a / b.
 * The probabilities are those of mmc_trainer_logits + _forward_probs (fp32 softmax, float64 renormalisation); they stay on the
 * device (fp32, class-major).  Host pointers throughout; every call synchronises `hip_stream` before returning.
 * Labels y are class indices in [0, K).  Results are bit-reproducible; the fit does not depend on how the rows are split over calls. */
typedef struct mmc_calibrator mmc_calibrator;
int mmc_calibrator_create(int K, int device, mmc_calibrator** out);          /* K >= 3 (CalibratedHead is multiclass only) */
void mmc_calibrator_destroy(mmc_calibrator* c);
/* rows of X (host, n x dims[0] fp32) through t's current parameters; probabilities stay on the device */
int mmc_calibrator_add_features(mmc_calibrator* c, mmc_trainer* t, const float* X, const int32_t* y, int64_t n, void* hip_stream);
/* caller-computed scores (host, n x K float64, row-major), e.g. another model's predict_proba / decision values; stored as fp32,
 * so non-finite scores and |score| > FLT_MAX are rejected */
int mmc_calibrator_add_scores(mmc_calibrator* c, const double* scores, const int32_t* y, int64_t n, void* hip_stream);
/* per-class Platt slope / intercept (K doubles each) over every row added so far: calibrated p_k = 1 / (1 + exp(a_k s + b_k)),
 * as _SigmoidCalibration.predict; iterations: K int32 (Newton trial points evaluated per class, at most 100) or NULL */
int mmc_calibrator_fit(mmc_calibrator* c, double* a, double* b, int32_t* iterations, void* hip_stream);
/* sums over the n rows: correct argmax count and sum of -log(clip(p_y)); the caller divides (streams add up).
 * The per-row term is rounded to 2^-32 and summed exactly in int64; *sum_log_loss is that sum as a double, which adds up
 * exactly over calls only while the total stays below 2^21.  At most 2^25 rows per call. */
int mmc_trainer_evaluate(mmc_trainer* t, const float* X, const int32_t* y, int64_t n, int64_t* n_correct,
                         double* sum_log_loss, void* hip_stream);
/* The same with the log-loss sum as the int64 it is computed in (units of 2^-32): integer sums over calls are exact for any
 * split of the rows.  (No reference counterpart; what the Python evaluate() accumulates.) */
int mmc_trainer_evaluate_q32(mmc_trainer* t, const float* X, const int32_t* y, int64_t n, int64_t* n_correct,
                             int64_t* sum_log_loss_q32, void* hip_stream);

/* ---- device-resident labelled feature sets: train, evaluate and calibrate without re-uploading a split ---------------------
 * Replaces: the per-epoch streaming of MermaidTrainer.__call__ (mermaid_classifier/pyspacer/trainer.py:138-168): there
 *   labels.train.load_data_in_batches(batch_size, random_seed=epoch) (:141-145) re-reads the train split from disk every epoch, and
 *   _calc_acc_batched (:295-307), _calc_acc_and_log_loss_batched (:309-342) and _calibrate_in_batches (:344-396) re-read ref / val,
 *   because a CPU box cannot hold N x dim floats (settings.training_batch_size sizes the batches from free RAM).  An MI355X holds a
 *   production split once (5 KB per row of 288 GB): a set is filled once -- from host rows, or from device rows such as
 *   mmc_backbone_extract's output, which then never visit the host -- and every later pass, evaluation and calibration reads it in place.
 * Storage: fp32 rows, row-major, and int32 class indices on the device, with a host mirror of the labels (argument checks, class-weight
 *   sums).  Capacity grows geometrically with a device-to-device copy; `reserve_rows` > 0 allocates up front and avoids the growth.  A
 *   failed allocation returns MMC_ERR_NOMEM and leaves the set as it was.
 * Every call synchronises `hip_stream` before returning.  One caller at a time per handle; a set must outlive the calls that read it. */
typedef struct mmc_featureset mmc_featureset;
int     mmc_featureset_create(int dim, int n_classes, int device, int64_t reserve_rows, mmc_featureset** out);
void    mmc_featureset_destroy(mmc_featureset* fs);
int64_t mmc_featureset_rows(const mmc_featureset* fs);   /* 0 for NULL */
int     mmc_featureset_dim(const mmc_featureset* fs);    /* 0 for NULL */
/* X: n x dim fp32, host (MMC_IN_HOST) or device memory on the set's device; y: n class indices in [0, n_classes), always host */
int mmc_featureset_append(mmc_featureset* fs, const float* X, const int32_t* y, int64_t n, unsigned flags, void* hip_stream);
/* rows [first, first+n) back to host buffers (either may be NULL): tests, export, debugging */
int mmc_featureset_read(mmc_featureset* fs, int64_t first, int64_t n, float* X, int32_t* y, void* hip_stream);

/* mmc_trainer_partial_fit_ordered (one epoch's clf.partial_fit, trainer.py:145) on rows that are resident: position i of the pass
 * visits row visit[i] of the set (visit == NULL: rows 0..rows-1 in order, n == rows).  The only upload is `visit`, 8 bytes per row.
 * The visited rows and labels are gathered into the trainer's mini-batch staging in chunks of whole mini-batches, each chunk followed
 * by its steps on the same stream; the steps launch the kernels of the host-fed pass on the same values, so parameters, Adam moments
 * and *avg_loss have the bits of mmc_trainer_partial_fit_ordered on the same rows.  Any feature width (16-byte lanes when dim % 4 == 0,
 * dwords otherwise).  Env MMC_TRAIN_CHUNK_ROWS, read at every call, bounds the chunk: its size is the largest multiple of the
 * mini-batch size not above the bound, and at least one mini-batch; default MMC_TRAIN_CHUNK_ROWS_DEFAULT rows (84 MB of staging at
 * 1280 columns).  Results do not depend on it.  A value that is not a positive integer is MMC_ERR_ARG.
 * Everything is checked before anything is launched -- visit[i] in [0, rows), the set's dim / n_classes / device against the
 * trainer's, a mini-batch of zero total class weight, the env value -- so a rejected pass leaves parameters, moments and step
 * count as they were. */
#define MMC_TRAIN_CHUNK_ROWS_DEFAULT 16384
int mmc_trainer_partial_fit_set(mmc_trainer* t, mmc_featureset* fs, const int64_t* visit, int64_t n, int batch_size,
                                double* avg_loss, void* hip_stream);
/* A sweep's pass: mmc_trainer_partial_fit_set for `count` trainers over one set, in the launches of one pass.
 * Replaces: S runs of the epoch body of MermaidTrainer.__call__ (mermaid_classifier/pyspacer/trainer.py:138-145), one per configuration
 *   of a hyper-parameter sweep -- what docs/research/hidden-layer-experiments.md (architectures x learning rates) and
 *   docs/research/balancing-experiments.md (15 configurations screened, 3 confirmed) ran as separate processes.  One Adam step of one
 *   head is some 30 small launches that leave most of the device idle; here step s of the pass is issued once for every member that
 *   still has a step s, each kind of launch once with the member as a grid dimension, on `hip_stream` alone.
 * For every member m the call does what mmc_trainer_partial_fit_set(trainers[m], fs, visit[m], n[m], batch_size[m], &avg_loss[m],
 *   hip_stream) does: same parameters, Adam moments, step count and avg_loss[m], bit for bit (that call is this one with a single
 *   member: the same kernels, and no reduction's decomposition depends on the group), independent of MMC_TRAIN_CHUNK_ROWS.  The members stay ordinary trainers: every
 *   other mmc_trainer_* / mmc_calibrator_* call and later solo passes work on them unchanged.
 * Members may differ in depth, widths, optimizer hyper-parameters, class weights, step count so far, n, visiting order and mini-batch
 *   size (so they finish at different steps); they share dims[0], the class count and the device with the set.
 * Everything is checked, and every member's buffers are reserved, before the first launch: NULL arrays, count outside
 *   [1, MMC_TRAINER_GROUP_MAX], a NULL member, one handle twice, and per member whatever mmc_trainer_partial_fit_set rejects (the
 *   message names the member) return MMC_ERR_ARG; a failed allocation returns MMC_ERR_NOMEM.  Either way no member's parameters,
 *   moments or step count change.  avg_loss (count doubles, or NULL) is zeroed on failure whenever count is in range. */
#define MMC_TRAINER_GROUP_MAX 16
int mmc_trainer_group_partial_fit_set(mmc_trainer* const* trainers, int count, mmc_featureset* fs, const int64_t* const* visit,
                                      const int64_t* n, const int* batch_size, double* avg_loss, void* hip_stream);
/* mmc_trainer_evaluate_q32 (trainer.py:295-342) on rows [first, first+n) of the set: the forward and the labels read the set, the
 * per-chunk int64 totals add up on the device, and the call makes one 16-byte device-to-host copy and one synchronisation.  The sums
 * are integers, so they equal the host-fed call's on the same rows for any first / n, and add up exactly over any split.  n is bounded
 * only by what the int64 total holds: a row adds at most -log(DBL_EPSILON) * 2^32 < 36.05 * 2^32, so MMC_EVALUATE_SET_MAX_ROWS
 * (< 2^31 / 36.05) rows per call cannot overflow it. */
#define MMC_EVALUATE_SET_MAX_ROWS 59000000
int mmc_trainer_evaluate_set_q32(mmc_trainer* t, mmc_featureset* fs, int64_t first, int64_t n,
                                 int64_t* n_correct, int64_t* sum_log_loss_q32, void* hip_stream);
/* mmc_calibrator_add_features (trainer.py:344-396) on rows [first, first+n) of the set: same probabilities, labels copied device to
 * device, one synchronisation. */
int mmc_calibrator_add_set(mmc_calibrator* c, mmc_trainer* t, mmc_featureset* fs, int64_t first, int64_t n, void* hip_stream);
/* Class-wise evaluation of the uncalibrated classifier: mmc_trainer_evaluate_q32 / mmc_trainer_evaluate_set_q32 that also keep each
 * row's (true class, prediction) pair, as a K x K table of int64 counts.
 * Replaces: per epoch, the confusion-matrix groups of MetricsCoordinator -- compute_precision_recall_f1 and
 *   compute_balanced_accuracy_mcc (mermaid_classifier/pyspacer/metrics/classification.py:171-302) -- which the reference runs once,
 *   after training, on the host.  The balancing study ranks configurations by balanced_accuracy and f1_macro
 *   (docs/research/balancing-experiments.md:17-19, 43) and finds them moving apart from accuracy over the epochs (:67, 82;
 *   hidden-layer-experiments.md:20-28); with the table per epoch the Python side (metrics.ClassScores) computes them every epoch.
 * confusion[g * K + est] = the rows with true class g whose prediction is est: the argmax of the renormalised probabilities, first
 *   index on ties (numpy.argmax) -- the argmax *n_correct is counted from.  Exact integers (64-bit integer atomics on the device):
 *   the table does not depend on row order, chunking or how the rows are split over calls, and the caller adds the tables of
 *   several calls.  Its trace is *n_correct and row g sums to the number of labels g.  (A row whose probabilities are all NaN has no
 *   argmax: it counts as wrong and enters no cell.)
 * *n_correct and *sum_log_loss_q32 carry the bits of mmc_trainer_evaluate_q32 / mmc_trainer_evaluate_set_q32 on the same rows; the
 *   arguments, checks and row limits are theirs, and confusion == NULL is MMC_ERR_ARG as well.  The device table lives in the
 *   trainer's scratch (grown on demand, freed with the handle); it is zeroed on the stream at the start of a call and accumulated
 *   over the call's chunks.  The _set form makes one device-to-host copy (totals and table) and one synchronisation per call; the
 *   host-fed form one synchronisation per 16 384-row chunk, as mmc_trainer_evaluate_q32.
 * A rejected call launches nothing and zeroes *n_correct, *sum_log_loss_q32 (when not NULL) and, when `t` is not NULL, the table. */
int mmc_trainer_evaluate_classes(mmc_trainer* t, const float* X, const int32_t* y, int64_t n, int64_t* n_correct,
                                 int64_t* sum_log_loss_q32, int64_t* confusion /* K*K */, void* hip_stream);
int mmc_trainer_evaluate_classes_set(mmc_trainer* t, mmc_featureset* fs, int64_t first, int64_t n, int64_t* n_correct,
                                     int64_t* sum_log_loss_q32, int64_t* confusion /* K*K */, void* hip_stream);

/* ---- regularisers: dropout and mixup in the trainer's steps, per trainer ------------------------------------------------------
 * Extends: the step of TorchMLPClassifier.partial_fit (torch_classifier.py:226-303), which has no stochastic regulariser, by what
 *   docs/research/hidden-layer-experiments.md (over-fitting onset at epoch 29; "loss formulation or feature representation") asks of a
 *   trainer of larger heads.  No counterpart in the reference.  Everything here defaults to off; with the defaults a pass launches the
 *   kernels, and gives the bits, of a trainer none of this was ever called on.
 * Masks.  Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85; round
 *   c' = [hi(M1 c2)^c1^k0, lo(M1 c2), hi(M0 c0)^c3^k1, lo(M0 c0)], key bumped after each of 10 rounds).  Element (m, n) of site s at
 *   step t -- m the row inside the mini-batch, N = dims[s] the unpadded width, site 0 the input and site l the output of layer l - 1
 *   (l = 1 .. n_layers - 1; the logits never drop) -- has e = m N + n (64 bit), counter (lo32 e, hi32 e, lo32 t, s), key (lo32 seed,
 *   hi32 seed), and is KEPT iff word 0 of the output >= thresh = (uint32)floor(p 2^32) (double).  t is the trainer's Adam step count
 *   before the step, so mmc_trainer_adam_state(set = 1) positions the mask sequence too.  Kept values become v * scale, one fp32
 *   multiply by scale = (float)(1.0 / (1.0 - p)); dropped values become +0.0f.  A mask depends on seed, step, site and position only.
 * Dropout.  Forward: H(l+1) = mask_{l+1}(relu(H(l) W(l)^T + b(l))) for hidden layers; backward: dZ(l) = (dZ(l+1) W(l)) * scale where
 *   H(l) > 0, else 0 (a dropped activation is stored as +0: no stored mask).  Input dropout applies mask_0 to the trainer's staged
 *   copy of the mini-batch, after mixing; the caller's rows and a feature set's rows are never written.  Works on every pass, host-fed
 *   or resident, solo or grouped.  Eval-mode forwards (mmc_trainer_logits, mmc_trainer_evaluate*, mmc_calibrator_add_*,
 *   mmc_logitcal_add_*, mmc_trainer_loss_gradient) see none of it; inverted dropout needs no rescaling at inference.
 * p_input, p_hidden finite in [0, 0.9], else MMC_ERR_ARG and the trainer is as it was; a p whose thresh is 0 is off; (0, 0, any seed)
 *   restores the plain step.  Allowed between passes. */
int mmc_trainer_set_dropout(mmc_trainer* t, double p_input, double p_hidden, uint64_t seed);
/* Mixup on resident passes: mmc_trainer_partial_fit_set / mmc_trainer_group_partial_fit_set with a mixing plan.  partner: n int64
 *   rows of the set; lam: one fp32 in [0, 1] per mini-batch, ceil(n / mb) entries (mb = min(batch_size, n)).  Position i of the pass,
 *   in mini-batch s, reads a = visit[i] (or i) and b = partner[i]; with oml = 1.0f - lam[s] its row is
 *     x[k] = lam Xa[k] + oml Xb[k]        two rounded fp32 products and one rounded add, no fma: numpy fp32 gives the same bits
 *   and its loss  l_i = lam l(z_i, ya) + oml l(z_i, yb)  with l the trainer's own row term before normalisation (the plain weighted CE or
 *   mmc_trainer_set_loss's form), one softmax and two targets.  The normaliser is g = (float)(1 / sum_i (lam w[ya_i] + oml w[yb_i])),
 *   summed in double in row order (lam and oml as the doubles of their fp32 values), and dlogits = g (lam dl(ya) + oml dl(yb)).
 *   The result does not depend on MMC_TRAIN_CHUNK_ROWS.
 * NULL partner and NULL lam: the unmixed call, bit for bit.  In the group form partner / lam are arrays of `count` pointers (or both
 *   NULL); a member whose two entries are NULL is not mixed.
 * Checked before the first launch, on top of the unmixed call's checks: only one of partner / lam given, partner[i] outside the set,
 *   lam NaN or outside [0, 1], a mini-batch whose mixed weight sum is not positive -> MMC_ERR_ARG, and no member's parameters, moments
 *   or step count change. */
int mmc_trainer_partial_fit_set_mixed(mmc_trainer* t, mmc_featureset* fs, const int64_t* visit, const int64_t* partner, const float* lam,
                                      int64_t n, int batch_size, double* avg_loss, void* hip_stream);
int mmc_trainer_group_partial_fit_set_mixed(mmc_trainer* const* trainers, int count, mmc_featureset* fs, const int64_t* const* visit,
                                            const int64_t* const* partner, const float* const* lam, const int64_t* n,
                                            const int* batch_size, double* avg_loss, void* hip_stream);
/* mmc_trainer_loss_gradient for the mixed loss stage: targets y and y2 per row and one lam for all n rows; g as above over these
 * rows.  Same checks (y2 like y; lam NaN or outside [0, 1] -> MMC_ERR_ARG).  For checking the mixed loss stage per element. */
int mmc_trainer_loss_gradient_mixed(mmc_trainer* t, const float* logits, const int32_t* y, const int32_t* y2, float lam, int64_t n,
                                    float* dlogits, float* row_loss, void* hip_stream);

/* ---- optimiser options: learning-rate schedule, gradient-norm clipping, averaged (EMA) weights, per trainer -----------------------
 * Extends: the torch.optim.Adam step of TorchMLPClassifier.partial_fit (torch_classifier.py:226-303), one constant learning rate
 *   and nothing else, by the usual remedies for what docs/research/hidden-layer-experiments.md reports of it: early-step instability at
 *   lr = 1e-3 (warm-up, a bound on the gradient norm) and a validation loss that turns up from epoch 29 (decay, averaged weights).
 *   No counterpart in the reference and no measured gain.  Everything here defaults to off; with the defaults a step launches the
 *   kernels, and gives the bits, of a trainer none of this was ever called on.  Each option is the trainer's own: the members of a
 *   grouped pass may differ in all of them, and a member computes the bits it computes alone.  Allowed between passes.  A rejected
 *   call (MMC_ERR_ARG) leaves parameters, moments, step count and every option as they were.
 * Schedule.  With s the 1-based Adam step being taken (the step count after the increment), lr the create-time learning rate,
 *   r = final_ratio, all in double:
 *     w    = warmup_steps > 0 ? min(1, s / warmup_steps) : 1
 *     u    = clamp((s - warmup_steps) / max(1, total_steps - warmup_steps), 0, 1)
 *     d    = 1                                     MMC_LR_CONSTANT (total_steps and final_ratio are not read)
 *          = 1 - (1 - r) u                         MMC_LR_LINEAR
 *          = r + (1 - r) 0.5 (1 + cos(pi u))       MMC_LR_COSINE   (pi the double nearest it; cos is the C library's)
 *     lr_s = lr w d                                (left to right)
 *   and the step's step_size is (float)(lr_s / (1 - beta1^s)).  A pure function of the step count: a trainer resumed through
 *   mmc_trainer_adam_state continues the schedule; no state, no device work.  Rejected: an unknown kind, warmup_steps < 0,
 *   total_steps <= warmup_steps for a decaying kind, final_ratio outside [0, 1].  (MMC_LR_CONSTANT, 0, 0, 0) is the constant rate.
 *   mmc_trainer_lr_at gives lr_s of the trainer for any step and mmc_lr_schedule_at the same function of explicit arguments; both
 *   are host code and launch nothing.
 * Clipping.  max_norm = 0: off; otherwise positive and finite (as fp32 too).  After the backward stage of a step the squares of every
 *   gW[l] and gb[l] of the member are summed -- gW includes the L2 term alpha / mb W, so this is the norm
 *   torch.nn.utils.clip_grad_norm_ sees on the reference's loss: per tensor 256 partial sums (block j of 256 takes the elements
 *   i = 256 j + tid + 65536 k in order of k, one fused multiply-add each, then a binary tree over the 256 threads), then one
 *   workgroup adds the 2L x 256 partials (thread i takes partials i, i + 256, ... in order; the same tree) and forms, in fp32 with
 *   nothing fused,
 *     norm = sqrtf(total),   coef = fminf(1.0f, (float)max_norm / (norm + 1e-6f))
 *   The Adam stage reads coef from device memory and uses g * coef (one rounding) wherever it read g; coef == 1.0f leaves the step's
 *   bits alone.  No float atomics, no host synchronisation, and a member's partials do not depend on who trains beside it.
 *   A non-finite norm gives what torch gives with error_if_nonfinite=False and is not hidden: norm = +inf -> coef = 0 (finite
 *   gradient elements become 0, infinite ones NaN), norm = NaN -> coef = NaN (torch's clamp hands a NaN on) and every parameter of
 *   the member becomes NaN.  mmc_trainer_grad_norms copies the pre-clip norms of the last pass's steps, in step order, into out
 *   (at most `capacity`) and sets *steps to their number (0 when the last pass did not clip).
 * Averaged weights.  decay = 0: off; otherwise in (0, 1).  Turning it on allocates a shadow of every W[l], b[l], initialised with the
 *   current parameters (so it is usable from step 0 and needs no bias correction); calling it again while on changes the decay and
 *   keeps the shadow; turning it off frees the shadow and selects MMC_WEIGHTS_RAW.  After a step's parameter update every element takes
 *     s = s + om_d (p_new - s),   om_d = (float)(1.0 - decay)         two rounded fp32 operations after the subtraction, nothing fused
 *   mmc_trainer_ema_state reads (set = 0) or writes (set = 1) the shadow, buffers shaped like mmc_trainer_get_params's; MMC_ERR_ARG
 *   without a shadow.  mmc_trainer_eval_weights chooses what the eval-mode forward reads -- mmc_trainer_logits, every
 *   mmc_trainer_evaluate*, mmc_calibrator_add_*, mmc_logitcal_add_* -- MMC_WEIGHTS_RAW (default) or MMC_WEIGHTS_AVERAGED
 *   (MMC_ERR_ARG without a shadow).  Training steps always read and write the raw weights, and mmc_trainer_get_params /
 *   mmc_trainer_adam_state keep returning the raw weights and their moments.
 * mmc_trainer_optimizer_options reads the options back (any pointer may be NULL). */
#define MMC_LR_CONSTANT 0
#define MMC_LR_LINEAR 1
#define MMC_LR_COSINE 2
#define MMC_WEIGHTS_RAW 0
#define MMC_WEIGHTS_AVERAGED 1
int mmc_trainer_set_lr_schedule(mmc_trainer* t, int kind, long long warmup_steps, long long total_steps, double final_ratio);
int mmc_trainer_lr_at(mmc_trainer* t, long long step, double* lr);
int mmc_lr_schedule_at(double lr, int kind, long long warmup_steps, long long total_steps, double final_ratio, long long step,
                       double* out);
int mmc_trainer_set_grad_clip(mmc_trainer* t, double max_norm);
int mmc_trainer_grad_norms(mmc_trainer* t, float* out, int capacity, int* steps);
int mmc_trainer_set_ema(mmc_trainer* t, double decay);
int mmc_trainer_ema_state(mmc_trainer* t, int set, float* const* W, float* const* b);
int mmc_trainer_eval_weights(mmc_trainer* t, int which);
int mmc_trainer_optimizer_options(mmc_trainer* t, int* lr_kind, long long* warmup_steps, long long* total_steps, double* final_ratio,
                                  double* max_norm, double* ema_decay, int* eval_which);

/* ---- group-robust training: per-row weights and group DRO in the loss stage of resident passes, per trainer -----------------------
 * Extends: the loss of TorchMLPClassifier.partial_fit (torch_classifier.py:226-303), whose only weighting is one weight per class, by
 *   what docs/research/balancing-experiments.md:141 leaves open: per-source accuracy from 0.434 to 0.940 and "per-source rebalancing"
 *   as the next lever.  No counterpart in the reference and no measured gain.  Group DRO is Algorithm 1 of Sagawa et al. 2020
 *   ("Distributionally robust neural networks for group shifts").  Both sit in the loss stage alone: the forward, the backward GEMMs,
 *   L2, clipping, EMA, the schedule, dropout and mmc_trainer_set_loss's formulations are untouched and compose with them; evaluation,
 *   calibration and export never see them.  With nothing set a pass launches the kernels, and gives the bits, of a trainer none of
 *   this was ever called on; in a group the members without weights or groups keep their kernels.
 * Notation.  A mini-batch has positions i = 0..M-1; w are the class weights (ones without); l_i and dl_i/dz are the trainer's own row
 *   term and its logit gradient before normalisation (the plain weighted CE or mmc_trainer_set_loss's form); r_i >= 0 is the row's
 *   fp32 weight (1 without row weights); the row mass is v_i = (double)r_i (double)w[y_i].
 * Row weights only.  g = (float)(1 / sum_i v_i), summed in double on the host in position order.  The row's normaliser is
 *   s_i = r_i g, one rounded fp32 product, and takes the place of 1 / sum_i w[y_i] in the row's formulas: dlogits_i = s_i dl_i,
 *   row_loss_i = s_i l_i, the operations in the unweighted kernel's order.  A pass whose weights are all 1.0f has the bits of
 *   mmc_trainer_partial_fit_set.
 * Group DRO.  mmc_trainer_set_group_dro(t, G, eta): G = n_groups in [1, MMC_DRO_MAX_GROUPS], eta in [0, 10]; n_groups = 0 turns it
 *   off; any call resets q to uniform.  The trainer holds logq[G] in double on the device, sum_a exp(logq_a) = 1, across steps and
 *   passes.  Position i carries a group a_i in [0, G).  Per step, nothing waiting on the host:
 *     1. the loss stage runs with normaliser r_i (g = 1): R_i = r_i l_i, D_i = r_i dl_i, fp32
 *     2. V_a = sum_{i in a} v_i in double on the host in position order, uploaded with the pass for every step and group
 *     3. S_a = sum_{i in a} R_i in double on the device, in an order that is a function of M and G alone: the rows go in tiles of
 *        2048; with NS = 16 / ceil(G / 64), slice s of a tile is its rows [s per, (s + 1) per), per = ceil(tile rows / NS); a slice
 *        adds its rows in position order, tile after tile, and the slices' sums are added in slice order.  No atomics.
 *     4. L_a = S_a / V_a for the groups with V_a > 0; the others (absent, or present without mass) have no loss this step
 *     5. logq_a = logq_a + eta L_a for those (two roundings); then logq_a -= mx + log(sum_b exp(logq_b - mx)), mx the maximum, the sum
 *        over all G in index order
 *     6. c_i = (float)(exp(logq_{a_i}) / V_{a_i}), or 0 where V = 0
 *     7. dlogits_i = c_i D_i, row_loss_i = c_i R_i: one fp32 multiply per element
 *     8. the step's loss is the unchanged sum of the row losses plus the L2 term: sum_a q_a L_a with the updated q, as in the paper
 *   eta = 0 never moves q: each present group counts 1 / G, a static group-balanced loss.
 * mmc_trainer_group_dro_state reads logq (set = 0) or writes it (set = 1) for a resume: a state that is normalised already
 *   (|log sum_a exp(logq_a)| <= 2^-40, what a read returns) is taken as it is, so the resumed trainer continues on the same bits;
 *   anything else is renormalised as in 5.  MMC_ERR_ARG without group DRO, or for an entry that is not finite.
 * The _weighted passes.  row_weight (n fp32) and row_group (n int32) are indexed by position of the pass, like partner; either may be
 *   NULL, both NULL is the unweighted call, bit for bit.  In the group form each is an array of `count` pointers, or NULL; a member
 *   whose two entries are NULL takes the plain kernels.  row_group needs mmc_trainer_set_group_dro(n_groups > 0) on that trainer;
 *   the plain and mixed entry points on such a trainer run as ever and leave q alone, and so does a pass with row weights only.
 *   There is no entry point for mixup with weights.  The results do not depend on MMC_TRAIN_CHUNK_ROWS, and a member of a group
 *   matches its solo pass bit for bit, logq included.
 * Checked before the first launch and before any member changes, on top of the unweighted call's checks: a weight that is negative
 *   or not finite, a group outside [0, n_groups), row_group on a trainer without group DRO, a mini-batch whose total mass is zero
 *   (no groups) or in which no group has mass (groups), eta or n_groups out of range -> MMC_ERR_ARG; parameters, moments, step
 *   count and logq stay as they were.
 * mmc_trainer_loss_gradient_weighted runs the stage's own kernels on caller logits, n in [1, 16384] rows taken as one mini-batch.
 *   With row_group it takes log q explicitly (log_q_in, used as given), returns the updated one in log_q_out and, when group_loss
 *   is not NULL, L_a (NaN for a group without loss); without row_group eta, n_groups and the three arrays are not read.  It does
 *   not touch the trainer's own distribution.  Same checks. */
#define MMC_DRO_MAX_GROUPS 1024
int mmc_trainer_set_group_dro(mmc_trainer* t, int n_groups, double eta);
int mmc_trainer_group_dro_state(mmc_trainer* t, int set, double* log_q /* n_groups */);
int mmc_trainer_partial_fit_set_weighted(mmc_trainer* t, mmc_featureset* fs, const int64_t* visit, const float* row_weight /* n or NULL */,
                                         const int32_t* row_group /* n or NULL */, int64_t n, int batch_size, double* avg_loss,
                                         void* hip_stream);
int mmc_trainer_group_partial_fit_set_weighted(mmc_trainer* const* trainers, int count, mmc_featureset* fs, const int64_t* const* visit,
                                               const float* const* row_weight, const int32_t* const* row_group, const int64_t* n,
                                               const int* batch_size, double* avg_loss, void* hip_stream);
int mmc_trainer_loss_gradient_weighted(mmc_trainer* t, const float* logits, const int32_t* y, const float* row_weight,
                                       const int32_t* row_group, const double* log_q_in, double eta, int n_groups, int64_t n,
                                       float* dlogits, float* row_loss, double* log_q_out, double* group_loss /* n_groups, NaN where none */,
                                       void* hip_stream);

/* ---- taxonomy-aware loss: level-marginal terms and soft labels in the loss stage, per trainer ---------------------------------------
 * Extends: the loss of TorchMLPClassifier.partial_fit (torch_classifier.py:226-303), which treats the K classes as unrelated symbols,
 *   by the two remedies of Bertinetto et al. 2020 ("Making better mistakes"): one loss term per level of the label hierarchy, and
 *   soft labels spread over taxonomic neighbours.  docs/research/hidden-layer-experiments.md section 5 names the loss formulation as
 *   the next lever; no counterpart in the reference and no measured gain on reef data.  Both sit in the loss stage alone: forward,
 *   backward GEMMs, L2, clipping, EMA, the schedule, dropout, row weights and group DRO are untouched and compose with them;
 *   evaluation, early stopping, calibration and export never see them.  With nothing set a pass launches the kernels, and gives the
 *   bits, of a trainer this was never called on; in a group the members without a hierarchy keep their kernels.
 * Notation.  u = z + prior (one fp32 add; u = z without a prior), p = softmax(u), t the row's true class, w_t its class weight (1
 *   without class weights), s_i the row's normaliser exactly as the other loss kernels form it: inv_wsum, or rw[row] * inv_wsum (one
 *   rounded product) on the row-weighted route.
 * Level terms.  L = n_levels in [1, MMC_HIER_MAX_LEVELS]; level_of_class[l][c] is the int32 node id g_l(c) of class c at level l.  Two
 *   classes share a node of level l iff their ids are equal and non-negative; a negative id is "no node at this level".  Each level has
 *   a weight lam_l >= 0, finite, given as a double and used as (float).  With P_l = sum_{c : g_l(c) = g_l(t)} p_c the row adds
 *     h_i       = w_t sum_l lam_l (-log P_l)
 *     dh_i/dz_c = w_t sum_l lam_l (p_c - [g_l(c) = g_l(t)] p_c / P_l)
 *   over the levels at which t has a node; the others add nothing.
 * Soft labels (optional).  soft_targets is a K x K fp32 matrix T, row t the target distribution of true class t: every entry >= 0 and
 *   finite, every row summing to 1 within 1e-5 (summed in double).  With T the base term of the row is
 *     b_i       = w_t (-sum_c T[t,c] logp_c)
 *     db_i/dz_c = w_t (p_c sum_c' T[t,c'] - T[t,c])
 *   with the row sum of T as stored (a lane-strided fp32 sum), not an assumed 1.  Without T the base term is mmc_trainer_set_loss's
 *   general form, which at its defaults is the plain weighted cross-entropy.
 * The row.  l_i = (base + h_i) s_i; dlogits is its gradient, row_loss[row] = l_i.  Group DRO's R_i is this whole row loss.
 * Finiteness.  Every output is finite on any finite row, a true node whose every member underflows against the row maximum and a node
 *   that holds all the probability included: each level takes its own maximum m_l over the node's members, forms
 *   -log P_l = (mx + lse) - (m_l + log sum exp(u_c - m_l)) and p_c / P_l = exp((u_c - m_l) - log sum ...), the softmax inside the
 *   node; nothing divides by a sum that can underflow.
 * mmc_trainer_set_hierarchy copies the ids and T to the device once.  n_levels = 0 with soft_targets NULL restores the default.
 *   MMC_ERR_ARG, the trainer left as it was: n_levels outside [0, MMC_HIER_MAX_LEVELS]; a NULL array that n_levels needs; a weight
 *   that is negative or not finite (as a float too); an entry of T that is negative or not finite; a row of T off 1 by more than
 *   1e-5; soft_targets on a trainer with label_smoothing != 0 or focal_gamma != 0 -- and mmc_trainer_set_loss with either on a trainer
 *   that has soft_targets: whichever of the two setters comes second refuses.  Smoothing, focal modulation and the prior compose
 *   with level terms: the base is the general form and the level terms are added.
 * A mixed (mixup) pass takes no hierarchy: mmc_trainer_loss_gradient_mixed on such a trainer, and mmc_trainer_partial_fit_set_mixed /
 *   mmc_trainer_group_partial_fit_set_mixed for a member that has one and is given a partner array, return MMC_ERR_ARG before any
 *   member changes.  mmc_trainer_loss_gradient and mmc_trainer_loss_gradient_weighted run the hierarchy's kernel on caller logits.
 *   A member of a group matches its solo pass bit for bit, and the results do not depend on MMC_TRAIN_CHUNK_ROWS. */
#define MMC_HIER_MAX_LEVELS 4
int mmc_trainer_set_hierarchy(mmc_trainer* t, int n_levels, const int32_t* level_of_class /* [n_levels][K], or NULL when n_levels == 0 */,
                              const double* level_weight /* [n_levels] */, const float* soft_targets /* [K][K], or NULL */);

/* ---- batch normalisation: between every hidden Linear and its ReLU, per trainer; folded into the Linear stack for evaluation ---------
 * Extends: the head of TorchMLPClassifier (torch_classifier.py:53-76, Linear -> ReLU -> ... -> Linear), whose deeper forms need a
 *   small step (docs/research/hidden-layer-experiments.md sections 2 and 3).  The meaning is torch.nn.BatchNorm1d's; no counterpart
 *   in the reference and no measured gain on reef data.  One switch normalises every hidden layer; the last layer never is.
 * Training forward.  Hidden layer l, mini-batch of mb rows, column j, Z = H_l W_l^T + b_l (the step's GEMM, bias epilogue):
 *     mu_j = mean_m Z[m][j];  v_j = mean_m (Z[m][j] - mu_j)^2 (biased, two passes);  rstd_j = 1 / sqrt(v_j + eps)
 *     xhat = (Z - mu_j) rstd_j;  H_{l+1} = relu(gamma_j xhat + beta_j)
 * Running statistics, after each step: rm = (1 - mom) rm + mom mu;  rv = (1 - mom) rv + mom v mb / (mb - 1) (unbiased).  They start
 *   at 0 and 1.  The scalars are the floats of eps, mom, 1 - mom and mb / (mb - 1), each formed in double.
 * Backward, from dA, the gradient w.r.t. gamma xhat + beta (what the step's masked dZ launch leaves):
 *     g_beta_j = sum_m dA;  g_gamma_j = sum_m dA xhat;  dZ = (gamma_j rstd_j / mb) ((mb dA - g_beta_j) - xhat g_gamma_j)
 * Every column sum runs in an order that is a function of (mb, N) alone: rows in four quarters of ceil(mb / 4), each on four chains
 *   in row order, (s0 + s1) + (s2 + s3), the quarters as (p0 + p1) + (p2 + p3).  No atomics; nothing is fused.
 * Parameters.  gamma starts at 1 and beta at 0; both are Adam parameters (the trainer's betas, eps, schedule and clipping: their
 *   gradients are part of the clipped norm) and not part of the L2 term.  The bias b_l of a normalised layer cancels exactly, so it
 *   is frozen: its gradient is zero-filled once and no column sum writes it, and Adam's update of it is 0 / eps: bit-unchanged.
 * Evaluation reads the folded stack: s_j = gamma_j / sqrt(rv_j + eps), W'_l[j][:] = s_j W_l[j][:], b'_l[j] = beta_j + s_j (b_l[j] - rm_j),
 *   refreshed lazily by the first eval-mode forward after a step; relu(W' x + b') is the frozen-statistics layer, so mmc_trainer_logits,
 *   the evaluation and calibration entry points and mmc_trainer_folded_params see one plain Linear / ReLU stack.
 * mmc_trainer_set_batch_norm: enable != 0 with eps > 0 (finite, as a float too) and 0 < momentum <= 1; enable = 0 restores the plain
 *   trainer, its launches and its bits (eps and momentum are then not read).  MMC_ERR_ARG, the trainer left as it was: a bad scalar;
 *   a trainer with hidden dropout (p_hidden > 0; input dropout composes) or with averaged weights -- and mmc_trainer_set_dropout
 *   with p_hidden > 0 or mmc_trainer_set_ema with a decay on a normalised trainer: whichever setter comes second refuses; a trainer
 *   whose Adam eps is 0.  Enabling again keeps the state and moves the two scalars.
 * A pass of a normalised trainer in which a mini-batch (the last one included) holds fewer than 2 rows returns MMC_ERR_ARG before
 *   anything is uploaded or launched: weights, moments and step count are unchanged.
 * Everything in the loss stage, the schedule, clipping, input dropout and mixup compose untouched.  A normalised member trains
 *   beside plain ones in a group; group equals solo, host-fed equals resident, and MMC_TRAIN_CHUNK_ROWS changes nothing, bit for bit.
 * mmc_trainer_batch_norm_state reads (set = 0) or writes the per-hidden-layer arrays: n_layers - 1 pointers each, entry l of
 *   dims[l + 1] floats.  mmc_trainer_folded_params is mmc_trainer_get_params of the folded stack (of a trainer without the option:
 *   that call itself).  mmc_trainer_norm_stage runs the step's two kernels on caller arrays Z, dA [mb][dims[layer + 1]], mb in
 *   [2, 16384], with the trainer's current gamma / beta of hidden layer `layer`; batch_var is the biased v; dA NULL runs the forward
 *   alone.  It touches neither the running statistics nor any other state. */
int mmc_trainer_set_batch_norm(mmc_trainer* t, int enable, double eps, double momentum);
int mmc_trainer_batch_norm_state(mmc_trainer* t, int set, float* const* gamma, float* const* beta, float* const* running_mean,
                                 float* const* running_var, float* const* adam_m_gamma, float* const* adam_v_gamma,
                                 float* const* adam_m_beta, float* const* adam_v_beta);
int mmc_trainer_folded_params(mmc_trainer* t, float* const* W, float* const* b);
int mmc_trainer_norm_stage(mmc_trainer* t, int layer, const float* Z, const float* dA, int64_t mb, float* H, float* dZ, float* g_gamma,
                           float* g_beta, float* batch_mean, float* batch_var, void* hip_stream);

/* ---- validation of a calibrated head --------------------------------------------------------------------------------
 * Replaces: what MermaidTrainer.__call__ computes after the calibration (mermaid_classifier/pyspacer/trainer.py:267-293:
 *   evaluate_classifier on val, ValResults, acc, the previous models' accuracies) and the per-row reductions the metrics make of the
 *   N x K probability matrix that MetricsCoordinator._precompute_probabilities builds on the host (metrics/coordinator.py:59-76):
 *   the rank of the true class (_compute_topk_mrr, metrics/ranking.py:42-65) and its clipped probability (the per-sample log-loss,
 *   metrics/probability.py:43-49).  The probabilities never leave the device and are never written: with v the row's calibrated
 *   values (the bits of mmc_head_predict: same launches for the Linear layers, same calibration arithmetic) and g its true class,
 *     est[i]    = the first maximum of v (numpy.argmax);   score[i] = v[est]
 *     p_true[i] = v[g]
 *     rank[i]   = the 1-based position of g in numpy.argsort(-v, kind="stable"): score descending and EQUAL SCORES IN CLASS ORDER.
 *                 The reference's np.argsort(-proba) (ranking.py:55) leaves the order of exactly equal probabilities undefined; the
 *                 rule here is the one mmc_head_topk and annotation.py:253-255 use.
 *   and, over the rows of the call, as exact integers that depend on neither row order nor on how rows are split over calls (the
 *   caller adds the totals of several calls):
 *     totals[0] rows the call went through       totals[1] rows with est == g
 *     totals[2] rows of an unknown class         totals[3] rows with a non-finite calibrated value
 *     totals[4] sum of round(-log(clip((double)p_true, 1e-15, 1.0)) * 2^32): probability.py:49 in 2^-32 fixed point
 *     confusion[g * K + est] (K x K, or NULL)    rank_hist[rank - 1] (K, or NULL)
 * y[i] is a class index of the head, or -- with label_map (n_labels entries in [-1, K)) -- an index into label_map, which gives the
 *   head's class or -1 for a class this head does not know.  An unknown row counts in totals[2] only: it is never correct and is left
 *   out of confusion, rank_hist and the loss sum; its rank is 0 and its p_true 0.  A row with a NaN (or infinite) calibrated value
 *   still gets est in [0, K) and rank in [1, K] from the key order, counts in totals[3] and is left out of totals[1], confusion,
 *   rank_hist and the loss sum.  Its neighbours are unaffected.
 * feats: n x input_dim fp32, host memory (flags = MMC_IN_HOST) or memory on the head's device.  y, label_map and every output are
 *   host pointers; est / score / rank / p_true (n each), confusion and rank_hist may each be NULL.  Only 16 bytes per row and the
 *   integer tables come back.  The call synchronises `hip_stream` before returning.  The _set form reads rows [first, first + n) and
 *   their labels where they lie; the set's class count must be K, or n_labels when a map is given.
 * Everything is checked before the first launch: NULL handles, n < 0 (n == 0 is MMC_OK with zeroed totals), y[i] outside [0, K) (or
 *   [0, n_labels) with a map), map entries outside [-1, K), the set's width / device / class count, first / n outside the set, and
 *   n > MMC_EVALUATE_SET_MAX_ROWS (a row adds at most -log(1e-15) * 2^32 < 36.05 * 2^32 to the int64 loss total).
 * Staging for labels, per-row outputs and totals belongs to the head handle, grows on demand and is freed with the handle: a
 *   repeated call allocates nothing.  One caller at a time per handle. */
#define MMC_EVAL_TOTALS 5
int mmc_head_evaluate(mmc_head* h, const float* feats, const int32_t* y, int64_t n, const int32_t* label_map, int n_labels,
                      int32_t* est, float* score, int32_t* rank, float* p_true, int64_t totals[MMC_EVAL_TOTALS],
                      int64_t* confusion /* K*K or NULL */, int64_t* rank_hist /* K or NULL */, unsigned flags, void* hip_stream);
int mmc_head_evaluate_set(mmc_head* h, mmc_featureset* fs, int64_t first, int64_t n, const int32_t* label_map, int n_labels,
                          int32_t* est, float* score, int32_t* rank, float* p_true, int64_t totals[MMC_EVAL_TOTALS],
                          int64_t* confusion /* K*K or NULL */, int64_t* rank_hist /* K or NULL */, void* hip_stream);

/* ---- grouped validation: cover, per-source, reliability --------------------------------------------------------------
 * Replaces: the whole-split passes of MetricsCoordinator.compute_and_log_all (mermaid_classifier/pyspacer/metrics/coordinator.py)
 *   that mmc_head_evaluate's totals cannot answer and that otherwise need every row back on the host:
 *     compute_cover (metrics/cover.py:44-72)            per-image class counts, then per-class bias / RMSE / MAE / R^2 over images
 *     compute_per_source (metrics/per_source.py:88-140) accuracy, balanced accuracy, macro P/R/F1, cross-branch rate per data source
 *     _adaptive_ece (metrics/calibration.py:32-79)      equal-mass bins over the sorted confidences
 *     metrics/probability.py:43-60, calibration.py:139-140   per-category log-loss, accuracy and mean confidence
 * The call is mmc_head_evaluate(_set) -- same arguments, and est / score / rank / p_true / totals / confusion / rank_hist come back
 * with the same bits -- followed by one more pass over the call's rows on the device.
 * Group inputs (host):
 *   image_offsets[n_images + 1]  image i owns rows [image_offsets[i], image_offsets[i+1]) of the call (cover.py:34-36 relies on the
 *                                same contiguity); image_offsets[0] = 0, strictly increasing (no empty image: the reference would
 *                                divide by zero), image_offsets[n_images] = n
 *   source_of_image[n_images]    in [0, n_sources); NULL or n_sources = 0: no per-source table
 *   n_bins                       in [1, MMC_GROUPED_MAX_BINS]
 * A row is SCORED exactly when mmc_head_evaluate adds it to confusion: its class is known and all its calibrated values are finite.
 * Unscored rows enter none of the tables below; an image's point count is its number of scored rows; an image without a scored row is
 * left out of the cover sums.  With g the true class of a scored row (outputs are host pointers, each may be NULL):
 *   support[g], nll_q32[g], score_q32[g]   K each: rows, sum of round(-log(clip(p_true, 1e-15, 1)) * 2^32) (the term of totals[4]) and
 *                                sum of llrint((double)score * 2^32), per true class.  Integer atomics: order-free, and any class ->
 *                                category grouping follows on the host by integer adds.
 *   source_confusion[(s * K + g) * K + est]   n_sources x K x K.  n_sources * K * K <= MMC_GROUPED_MAX_SOURCE_CELLS.
 *   cover_sums[c * MMC_COVER_SUMS + j]   with t = true_cnt[i][c] / points[i] and p = pred_cnt[i][c] / points[i] in fp64 over the
 *                                *n_images_used images with points > 0 (the int32 count tables live in the handle's scratch:
 *                                n_images * K <= MMC_GROUPED_MAX_COVER_CELLS):
 *                                  j = 0 sum t    1 sum p    2 sum (p - t)    3 sum (p - t)^2    4 sum |p - t|    5 min t    6 max t
 *                                  7 sum (t - tbar)^2, tbar = sum t / n_images_used, from a second pass over the resident table
 *                                max t > min t is the reference's true_col.std() > 0 gate.  Sums, not means; no float atomics:
 *                                per-workgroup partials reduced in a fixed order that depends on n_images alone, so a repeated call
 *                                returns the same bits.
 *   bin_count, bin_correct, bin_conf_q32, bin_conf_min, bin_conf_max   n_bins each.  Every scored row gets the 31-bit key
 *                                (bits(score) << 1) | (est == g); the rows are taken in key order -- the reference's order of
 *                                np.argsort(confidences), with equal scores wrong before right where the reference leaves the order
 *                                undefined -- and bin b holds the sorted positions [b * n_scored / n_bins, (b + 1) * n_scored /
 *                                n_bins) (integer division: np.linspace(0, n, n_bins + 1, dtype=int)).  Per bin: rows, rows with
 *                                est == g, sum of llrint((double)score * 2^32), and the scores of its first and last key.  Found by a
 *                                radix select of the edge keys and one binned-sum pass, without sorting; equal-key rows are split
 *                                between bins by integer position arithmetic.  An empty bin (n_scored < n_bins) has count 0 and 0 in
 *                                every column.
 * One call covers a whole split, n <= MMC_EVALUATE_SET_MAX_ROWS: the cover second pass and the global order do not merge across calls.
 * Everything is checked before the first launch -- the checks of mmc_head_evaluate(_set), and: image_offsets NULL, not starting at 0,
 *   not strictly increasing or not ending at n; n_images < 1 or > n; source_of_image[i] outside [0, n_sources); n_sources < 0; n_bins
 *   outside [1, MMC_GROUPED_MAX_BINS]; either cap exceeded -- and a rejected call returns MMC_ERR_ARG with nothing launched and every
 *   output whose size the arguments determine zeroed (the bin tables only for a valid n_bins, source_confusion only within its cap).
 *   n == 0 with n_images == 0 is MMC_OK with zeroed outputs.
 * Scratch (4 B of key per row, the count tables, the select histograms, the slabs) belongs to the head handle, grows on demand and is
 *   freed with it.  The call synchronises `hip_stream` once, at the end. */
#define MMC_GROUPED_MAX_BINS 64
#define MMC_GROUPED_MAX_SOURCE_CELLS 67108864LL  /* 2^26 */
#define MMC_GROUPED_MAX_COVER_CELLS 268435456LL  /* 2^28 */
#define MMC_COVER_SUMS 8
int mmc_head_evaluate_grouped(mmc_head* h, const float* feats, const int32_t* y, int64_t n, const int32_t* label_map, int n_labels,
                              int32_t* est, float* score, int32_t* rank, float* p_true, int64_t totals[MMC_EVAL_TOTALS],
                              int64_t* confusion /* K*K or NULL */, int64_t* rank_hist /* K or NULL */,
                              const int64_t* image_offsets, int64_t n_images, const int32_t* source_of_image, int n_sources, int n_bins,
                              int64_t* support, int64_t* nll_q32, int64_t* score_q32, int64_t* source_confusion,
                              double* cover_sums /* K*MMC_COVER_SUMS */, int64_t* n_images_used,
                              int64_t* bin_count, int64_t* bin_correct, int64_t* bin_conf_q32, float* bin_conf_min, float* bin_conf_max,
                              unsigned flags, void* hip_stream);
int mmc_head_evaluate_grouped_set(mmc_head* h, mmc_featureset* fs, int64_t first, int64_t n, const int32_t* label_map, int n_labels,
                                  int32_t* est, float* score, int32_t* rank, float* p_true, int64_t totals[MMC_EVAL_TOTALS],
                                  int64_t* confusion /* K*K or NULL */, int64_t* rank_hist /* K or NULL */,
                                  const int64_t* image_offsets, int64_t n_images, const int32_t* source_of_image, int n_sources, int n_bins,
                                  int64_t* support, int64_t* nll_q32, int64_t* score_q32, int64_t* source_confusion,
                                  double* cover_sums /* K*MMC_COVER_SUMS */, int64_t* n_images_used,
                                  int64_t* bin_count, int64_t* bin_correct, int64_t* bin_conf_q32, float* bin_conf_min, float* bin_conf_max,
                                  void* hip_stream);

/* ---- category validation: per-category reliability bins ----------------------------------------------------------------
 * Replaces: the second half of compute_calibration (mermaid_classifier/pyspacer/metrics/calibration.py:120-161): one _adaptive_ece
 *   table per top-level category, over the rows whose true class lies in that category, with the category's own bin count
 *   n_bins_cat = min(20, max(2, n // 10)) (calibration.py:137).  That needs the order of the scores inside each category, which the
 *   grouped call does not keep; without this call the only route is est / score per row back to the host and np.argsort per category.
 * The call is mmc_head_evaluate_grouped(_set) -- same arguments, and every per-row, evaluation and group output comes back with the same
 * bits -- followed by one more select per category on the device.  Extra arguments (host pointers):
 *   category_of_class[K]   int32 in [-1, n_categories): the category of each class of the head (the label map has been applied), -1 for
 *                          a class that belongs to no category
 *   n_categories           in [1, MMC_CATEGORY_MAX]
 * A row is SCORED exactly when mmc_head_evaluate adds it to confusion; unscored rows and rows of a class without a category enter no
 * category table.  With n_c the scored rows whose true class lies in category c (outputs, each may be NULL):
 *   cat_rows[c]            n_categories: n_c
 *   cat_n_bins[c]          n_categories: nb_c = min(MMC_CATEGORY_MAX_BINS, max(MMC_CATEGORY_MIN_BINS, n_c / MMC_CATEGORY_ROWS_PER_BIN))
 *                          for n_c > 0, else 0
 *   cat_bin_count, cat_bin_correct, cat_bin_conf_q32, cat_bin_conf_min, cat_bin_conf_max   [n_categories][MMC_CATEGORY_MAX_BINS]: per
 *                          category what bin_count ... bin_conf_max are for the whole split: the category's rows in the order of the
 *                          31-bit key (bits(score) << 1) | (est == g), bin b = sorted positions [b * n_c / nb_c, (b + 1) * n_c / nb_c),
 *                          equal-key rows split by integer position arithmetic.  Empty bins and the bins at index nb_c and above are 0
 *                          in every column.  Integer atomics only: the tables depend on neither row order, grid nor chunking.
 * Everything is checked before the first launch -- the checks of mmc_head_evaluate_grouped(_set), and: category_of_class NULL, an
 *   entry outside [-1, n_categories), n_categories outside [1, MMC_CATEGORY_MAX] -- and a rejected call returns MMC_ERR_ARG with nothing
 *   launched and every output whose size the arguments determine zeroed (the category tables only for a valid n_categories).  n == 0
 *   with n_images == 0 is MMC_OK with zeroed outputs.
 * Scratch (one more byte and one more 4 B key per row, one select state per category) belongs to the head handle, grows on demand and
 *   is freed with it.  The call synchronises `hip_stream` once, at the end. */
#define MMC_CATEGORY_MAX 64
#define MMC_CATEGORY_MAX_BINS 20     /* calibration.py:137: min(20, ...          */
#define MMC_CATEGORY_MIN_BINS 2      /* calibration.py:137:      ... max(2, ...   */
#define MMC_CATEGORY_ROWS_PER_BIN 10 /* calibration.py:137:            ... n // 10)) */
int mmc_head_evaluate_categories(mmc_head* h, const float* feats, const int32_t* y, int64_t n, const int32_t* label_map, int n_labels,
                                 int32_t* est, float* score, int32_t* rank, float* p_true, int64_t totals[MMC_EVAL_TOTALS],
                                 int64_t* confusion /* K*K or NULL */, int64_t* rank_hist /* K or NULL */,
                                 const int64_t* image_offsets, int64_t n_images, const int32_t* source_of_image, int n_sources, int n_bins,
                                 int64_t* support, int64_t* nll_q32, int64_t* score_q32, int64_t* source_confusion,
                                 double* cover_sums /* K*MMC_COVER_SUMS */, int64_t* n_images_used,
                                 int64_t* bin_count, int64_t* bin_correct, int64_t* bin_conf_q32, float* bin_conf_min, float* bin_conf_max,
                                 const int32_t* category_of_class /* K */, int n_categories, int64_t* cat_rows, int32_t* cat_n_bins,
                                 int64_t* cat_bin_count, int64_t* cat_bin_correct, int64_t* cat_bin_conf_q32, float* cat_bin_conf_min,
                                 float* cat_bin_conf_max, unsigned flags, void* hip_stream);
int mmc_head_evaluate_categories_set(mmc_head* h, mmc_featureset* fs, int64_t first, int64_t n, const int32_t* label_map, int n_labels,
                                     int32_t* est, float* score, int32_t* rank, float* p_true, int64_t totals[MMC_EVAL_TOTALS],
                                     int64_t* confusion /* K*K or NULL */, int64_t* rank_hist /* K or NULL */,
                                     const int64_t* image_offsets, int64_t n_images, const int32_t* source_of_image, int n_sources, int n_bins,
                                     int64_t* support, int64_t* nll_q32, int64_t* score_q32, int64_t* source_confusion,
                                     double* cover_sums /* K*MMC_COVER_SUMS */, int64_t* n_images_used,
                                     int64_t* bin_count, int64_t* bin_correct, int64_t* bin_conf_q32, float* bin_conf_min, float* bin_conf_max,
                                     const int32_t* category_of_class /* K */, int n_categories, int64_t* cat_rows, int32_t* cat_n_bins,
                                     int64_t* cat_bin_count, int64_t* cat_bin_correct, int64_t* cat_bin_conf_q32, float* cat_bin_conf_min,
                                     float* cat_bin_conf_max, void* hip_stream);

/* ---- ranking validation: per-class ranks, hierarchical top-k -----------------------------------------------------------
 * Replaces: the parts of compute_ranking (mermaid_classifier/pyspacer/metrics/ranking.py) that need more than the overall rank
 *   histogram and that otherwise need the N x K probability matrix and np.argsort(-proba) on the host:
 *     per-category top-k / MRR (ranking.py:88-128)   the rank of the true class, broken down by true class
 *     hierarchical top-k (ranking.py:163-209)        per row the kmax best classes in order and the largest taxonomic similarity to
 *                                                    the true class among the first k of them
 * The call is mmc_head_evaluate(_set) -- same arguments, and est / score / rank / p_true / totals / confusion / rank_hist come back
 * with the same bits -- with one more kernel per chunk on the chunk's logits.  Extra arguments (host pointers):
 *   sim_level[g * K + c]   uint8, K x K, row = true class: the similarity of classes g and c as a level code in [0, n_levels).  Codes
 *                          are monotone in the similarity (the caller keeps the code -> value table), so the largest level is the
 *                          largest similarity.  NULL together with hier_hist: only class_rank_hist is made, no selection runs.
 *   n_levels               in [1, 256]
 *   kmax                   in [1, min(K, MMC_RANKED_MAX_K)]: selection rounds per row
 * A row is SCORED exactly when mmc_head_evaluate adds it to confusion; unscored rows enter neither table.  With g the true class of
 * a scored row (int64 counts, integer atomics: independent of row order and of how rows are split over chunks or calls):
 *   class_rank_hist[g * K + rank - 1]    K x K, or NULL.  Its column sums are rank_hist, its row sums the scored rows per class,
 *                                        class_rank_hist[g * K] = confusion[g * K + g].
 *   hier_hist[j * n_levels + m]          kmax x n_levels, or NULL: rows whose largest sim_level[g][c_i] over i <= j is m, where
 *                                        c_0, c_1, ... are the row's classes in the order of mmc_head_topk: score descending and EQUAL
 *                                        SCORES IN CLASS ORDER (the reference's np.argsort(-proba) leaves ties open).  Every row
 *                                        j sums to the number of scored rows.
 * Everything is checked before the first launch -- the checks of mmc_head_evaluate(_set), and: n_levels or kmax out of range, a
 *   sim_level entry >= n_levels, sim_level without hier_hist or the reverse -- and a rejected call returns MMC_ERR_ARG with nothing
 *   launched and totals / confusion / rank_hist / class_rank_hist zeroed (the K-sized ones only with a head handle), hier_hist when
 *   n_levels lies in [1, 256] and kmax in [1, MMC_RANKED_MAX_K].  n == 0 is MMC_OK with zeroed tables.
 * The uploaded levels and the device tables live in scratch that belongs to the head handle, grows on demand and is freed with it.
 *   The call synchronises `hip_stream` once, at the end. */
#define MMC_RANKED_MAX_K 16
int mmc_head_evaluate_ranked(mmc_head* h, const float* feats, const int32_t* y, int64_t n, const int32_t* label_map, int n_labels,
                             int32_t* est, float* score, int32_t* rank, float* p_true, int64_t totals[MMC_EVAL_TOTALS],
                             int64_t* confusion /* K*K or NULL */, int64_t* rank_hist /* K or NULL */,
                             const uint8_t* sim_level /* K*K or NULL */, int n_levels, int kmax,
                             int64_t* class_rank_hist /* K*K or NULL */, int64_t* hier_hist /* kmax*n_levels or NULL */,
                             unsigned flags, void* hip_stream);
int mmc_head_evaluate_ranked_set(mmc_head* h, mmc_featureset* fs, int64_t first, int64_t n, const int32_t* label_map, int n_labels,
                                 int32_t* est, float* score, int32_t* rank, float* p_true, int64_t totals[MMC_EVAL_TOTALS],
                                 int64_t* confusion /* K*K or NULL */, int64_t* rank_hist /* K or NULL */,
                                 const uint8_t* sim_level /* K*K or NULL */, int n_levels, int kmax,
                                 int64_t* class_rank_hist /* K*K or NULL */, int64_t* hier_hist /* kmax*n_levels or NULL */,
                                 void* hip_stream);

/* ---- cover estimation: counts, soft cover, EM prior adaptation -------------------------------------------------------------
 * Extends: compute_cover's predicted counts (mermaid_classifier/pyspacer/metrics/cover.py:49-60), which exist in the reference only
 *   as a validation metric, to the serving side: percent cover per image, transect or source, from the calibrated probabilities
 *   where they lie.  docs/research/hidden-layer-experiments.md section 5 names cover R^2 as the metric of record, and
 *   docs/research/balancing-experiments.md closes on a per-source accuracy range that balancing does not remove: the signature of
 *   label shift.  mmc_trainer_set_loss's logit_prior is the training-time half of the standard remedy; this is the test-time half
 *   (Saerens, Latinne and Decaestecker 2002): each group's class prior is re-estimated from its calibrated probabilities by EM, and
 *   cover and labels are read off the adapted posteriors.  No reference counterpart: THIS TEXT IS THE DEFINITION.
 * Rows are points.  v is a point's calibrated probability row with the bits mmc_head_predict writes; with G > 1 views per point, v
 *   is the mean m that mmc_head_topk_views writes.  Groups are contiguous: group g owns points [group_offsets[g], group_offsets[g+1])
 *   (group_offsets[0] = 0, never decreasing -- a group may be empty --, group_offsets[n_groups] = n).  A point is USABLE when all K
 *   values are finite; unusable points are counted in unusable[g] and enter nothing else.  n_g is the number of usable points of
 *   group g.  train_prior: K doubles, every entry > 0, summing to 1 within 1e-6; NULL means 1/K.
 * Per group (host pointers; count, soft_q32, prior: n_groups x K, unusable: n_groups):
 *   count[g*K + c]     int64: the usable points whose first maximum is c -- est of mmc_head_evaluate, cover.py's predicted count.
 *   soft_q32[g*K + c]  int64: the sum over the usable points of llrint((double)v[c] * 2^32).  Order-free and exact.
 *   prior[g*K + c]     fp64: pi_iters[c] of the EM that starts from pi_0 = train_prior and runs for t = 1 .. iters:
 *                        w      = pi_{t-1} / train_prior                                         in fp64
 *                        tq[c]  = (double)v[c] * w[c],  Z = sum_c tq[c]                          per usable point
 *                        q      = tq / Z when Z is finite and > 0, otherwise q = (double)v
 *                        pi_t[c] = (sum over the usable points of q[c] + strength * train_prior[c]) / (n_g + strength)
 *                      strength >= 0 is a Dirichlet pseudo-count (with strength = 0 a 25-point image collapses onto the classes it
 *                      shows).  A group with n_g = 0 keeps train_prior.
 *   Sum order: the order of the fp64 sums on the device is unspecified; it depends only on group_offsets and K, so a repeated call
 *   returns the same bits.  No float atomics are used.
 * Adapted top-k (idx / scores: n x k, host with MMC_OUT_HOST in flags, else on the device; both NULL: skipped, and k is ignored):
 *   q is computed from w = pi_iters / train_prior as above (for every point: an unusable point has a non-finite Z, so q = v),
 *   score = (float)q[c], and the k best classes are chosen by the key rule of mmc_head_topk: fp32 score descending (by bit pattern),
 *   equal scores in class order, k distinct classes even for unusable rows.
 * Everything is checked before the first launch: n < 0, n * K > MMC_COVER_MAX_CELLS, n_groups < 0 or n_groups * K >
 *   MMC_COVER_MAX_CELLS, offsets not starting at 0, decreasing or not ending at n (n_groups = 0 needs n = 0), a train_prior entry
 *   that is not a positive finite number or a sum off 1 by more than 1e-6, strength negative or not finite, iters outside
 *   [0, MMC_COVER_MAX_ITERS], idx without scores or the reverse, k outside [1, K] when they are given, NULL tables, G outside
 *   [1, MMC_VIEWS_MAX], the set's width / device / rows.  A rejected call returns MMC_ERR_ARG, launches nothing and zeroes every
 *   host output whose size the arguments determine (the tables when n_groups * K is within the cap; idx / scores when they are host
 *   memory and n, k are valid).  n = 0 is MMC_OK: zero counts, and train_prior in every row of prior.
 * mmc_cover_proba runs the stage on caller probabilities (n x K fp32, host with MMC_IN_HOST in flags, else on `device`): for
 *   probabilities made elsewhere, and for checking the stage per element.  Its scratch is kept per device for the life of the process.
 * mmc_head_cover / mmc_head_cover_set score feats ((n_points * G) x input_dim, host with MMC_IN_HOST, else on the head's device) or
 *   rows [first, first + n_points * G) of a feature set through the head's chunk loop -- the launches of mmc_head_predict (G = 1) or
 *   mmc_head_topk_views (G > 1), each chunk written straight into a resident n_points x K matrix -- and run the stage on it.  The
 *   matrix and the stage's scratch belong to the head handle, grow on demand and are freed with it: a repeated call allocates nothing.
 * Each call synchronises `hip_stream` once, at the end: uploads, chunks, the two launches of every EM iteration and the copies
 *   back are enqueued back to back.  One caller at a time per handle; mmc_cover_proba calls are serialised inside the library. */
#define MMC_COVER_MAX_ITERS 1000
#define MMC_COVER_MAX_CELLS 1073741824LL  /* 2^30: 4 GiB of resident probabilities */
int mmc_cover_proba(const float* proba /* n x K */, int64_t n, int K, const int64_t* group_offsets /* n_groups + 1 */, int64_t n_groups,
                    const double* train_prior /* K or NULL */, double strength, int iters, int64_t* count, int64_t* soft_q32,
                    int64_t* unusable, double* prior, int k, int32_t* idx /* n x k or NULL */, float* scores /* n x k or NULL */,
                    int device, unsigned flags, void* hip_stream);
int mmc_head_cover(mmc_head* h, const float* feats /* (n_points*G) x input_dim */, int64_t n_points, int G,
                   const int64_t* group_offsets, int64_t n_groups, const double* train_prior, double strength, int iters, int64_t* count,
                   int64_t* soft_q32, int64_t* unusable, double* prior, int k, int32_t* idx, float* scores, unsigned flags,
                   void* hip_stream);
int mmc_head_cover_set(mmc_head* h, mmc_featureset* fs, int64_t first, int64_t n_points, int G, const int64_t* group_offsets,
                       int64_t n_groups, const double* train_prior, double strength, int iters, int64_t* count, int64_t* soft_q32,
                       int64_t* unusable, double* prior, int k, int32_t* idx, float* scores, unsigned flags, void* hip_stream);

/* ---- feature transforms: moments, scatter, centre-and-project on a resident set -----------------------------------------------
 * Extends: the reference trains its MLP on the raw pooled activations (mermaid_classifier/pyspacer/trainer.py:118-145);
 *   docs/research/hidden-layer-experiments.md section 5 closes on "the next round of work should target loss formulation or feature
 *   representation rather than head architecture".  mmc_trainer_set_loss is the first half; these entries are what the second needs
 *   from the device: a fitted LINEAR transform of the features -- per-feature standardisation, PCA reduction, PCA whitening, on total
 *   or pooled within-class scatter -- fitted on one resident set and applied into another.  The eigen-decomposition of the dim x dim
 *   scatter is host work, and at calibration time the transform is folded into the first Linear layer
 *   (mermaid_classifier_amd/feature_transform.py), so heads, artifacts and predictors keep taking raw backbone features.
 *   No reference counterpart: THIS TEXT IS THE DEFINITION.  Whether any of these transforms improves accuracy or cover on reef data
 *   has not been measured.
 * All three read rows [first, first + n) of a set in place (n <= 2^31 - 1), on `hip_stream`, and synchronise it before returning (their
 *   device scratch is allocated per call and freed).  Outputs are host memory with MMC_OUT_HOST in flags, else memory of the set's
 *   device; centres / centre / T are host memory with MMC_IN_HOST, else on the set's device.  A rejected call (MMC_ERR_ARG) or a
 *   failed allocation (MMC_ERR_NOMEM) writes nothing.  n = 0 is MMC_OK: zeros (moments, scatter), nothing appended (transform).
 *   K = the set's class count, dim its width.
 * Determinism: no float atomics.  The result bits are a function of the rows' values and labels, first, n and dim -- never of the
 *   device, the CU count or the grid's dispatch order -- so a repeated call returns the same bits.
 *
 * mmc_featureset_moments: groups 0 .. K-1 are the classes, group K is every row of the range.
 *   counts[c]           int64, c < K: the rows with label c.
 *   mean[g*dim + j]     fp64: the sum of (double)x[j] over the group's rows, divided by the group's row count; 0 for an empty group.
 *   m2[g*dim + j]       fp64: the sum over the group's rows of d*d, d = (double)x[j] - mean[g*dim + j] (the fp64 mean above, so slot K
 *                       is about the global mean and a class slot about its own class mean); 0 for an empty group.
 *   Sum order: a group's rows in ascending order are cut into slabs of 256; a slab is summed in row order (m2 by fma(d, d, acc)), a
 *   group's slabs are added in ascending order.
 * mmc_featureset_scatter: scatter[j*dim + k] (dim x dim fp64, symmetric bit for bit)
 *     = sum over the rows of xc[j] * xc[k],   xc = fl32(x - c): the fp32 difference, ONE rounding,
 *   with c = centres[0 .. dim) when by_label = 0 (total scatter about one centre) and c = centres[y*dim .. (y+1)*dim), y the row's label,
 *   when by_label = 1 (centres is K x dim: pooled within-class scatter).  Rows are cut into chunks of MMC_SCATTER_CHUNK_ROWS consecutive
 *   rows; inside a chunk an element is one fp32 fmaf chain in row order (the exact-f32 MFMA), the chunk's fp32 value is then added to an
 *   fp64 accumulator.  The chunks are split over S = min(MMC_SCATTER_MAX_SPLITS, max(1, 512 / P), chunks) contiguous ranges, P = T (T + 1) / 2
 *   and T = ceil(dim / 128) -- a function of n and dim alone --, range s holding chunks [s * chunks / S, (s + 1) * chunks / S); a range's
 *   chunks are added in order and the S range sums are added in ascending order.  Element (j, k) is computed once for j <= k and copied
 *   to (k, j).  dim > MMC_SCATTER_MAX_DIM is MMC_ERR_ARG.  Scratch: S * P * 128 KiB (70 MiB at dim = 1280).
 * mmc_featureset_transform: appends n rows of width m to dst (dst's width must be m, its class count and device src's; dst = src is
 *   MMC_ERR_ARG): row i is  y[k] = sum over j of fl32(x[j] - centre[j]) * T[k*dim + j],  one fp32 fmaf chain over j ascending from 0
 *   (the rounding of every other fp32 GEMM here); T is m x dim.  The labels are copied with the rows.  dst grows as in
 *   mmc_featureset_append, and its row count moves last: a failed call leaves dst's rows and count as they were. */
#define MMC_SCATTER_CHUNK_ROWS 256
#define MMC_SCATTER_MAX_SPLITS 16
#define MMC_SCATTER_MAX_DIM 2048
int mmc_featureset_moments(mmc_featureset* fs, int64_t first, int64_t n, int64_t* counts /* K */, double* mean /* (K+1) x dim */,
                           double* m2 /* (K+1) x dim */, unsigned flags, void* hip_stream);
int mmc_featureset_scatter(mmc_featureset* fs, int64_t first, int64_t n, const float* centres /* dim, or K x dim with by_label */,
                           int by_label, double* scatter /* dim x dim */, unsigned flags, void* hip_stream);
int mmc_featureset_transform(mmc_featureset* src, int64_t first, int64_t n, const float* centre /* dim */, const float* T /* m x dim */,
                             int m, mmc_featureset* dst, unsigned flags, void* hip_stream);

/* ---- nearest neighbours: fused exact-f32 top-k between resident sets -----------------------------------------------------------
 * Extends: nothing in the reference.  Three questions its data raises rest on "which rows are close to which": point labels are noisy
 *   (a row whose neighbours from OTHER images mostly carry another label is the first candidate for review);
 *   docs/research/balancing-experiments.md closes on a per-source accuracy floor that "may motivate a per-source feature-extraction
 *   review", and a kNN classifier on the raw features is the standard probe for that; near-duplicate rows between train and validation
 *   splits inflate every validation number.  The host algebra is mermaid_classifier_amd/neighbors.py.
 *   No reference counterpart: THIS TEXT IS THE DEFINITION.  No gain on reef data has been measured.
 * For every query row i of rows [q_first, q_first + nq) of `query`: the k best eligible rows of rows [b_first, b_first + nb) of `base`
 *   (the same set is allowed, overlapping ranges too).  Equal dim, same device; the nq x nb score matrix is never stored.
 * Score of query row q and base row b, in fp32; larger is better for all three metrics:
 *   d        one fmaf chain over the dim columns in ascending order, from +0 (the exact-f32 MFMA: the rounding of every other fp32
 *            GEMM here)
 *   DOT      d
 *   COSINE   (d * rq) * rb       r = fl32(1 / sqrt(ss)), ss = the fp64 sum of (double)x * x over the row's columns in ascending order
 *                                (fma chain); r = 0 when ss is not > 0 (a zero row)
 *   L2       -fmaf(-2, d, sq + sb)   s = fl32(ss): minus the squared distance
 *   A score of -0 is keyed and returned as +0.
 * Order: score descending, equal scores by ascending base row; NaN below every number (returned as 0x7FC00000).  The device orders
 *   64-bit keys (w << 32) | (0xFFFFFFFF - j), j the row relative to b_first and w the score word: 0 = no entry, 1 = NaN, else the fp32
 *   bits with the sign bit set for a score >= 0 and every bit inverted for a score < 0 (-inf -> 0x007FFFFF, +inf -> 0xFF800000).  The
 *   keys of a query are distinct, the k largest of a set under a total order are unique: the output bits depend on the rows, dim, k and
 *   metric only -- never on tiles, splits, chunks, the grid or the device.  No float atomics, no cross-workgroup flags.
 * Eligibility, applied BEFORE selection: base row b_first + j is out for query i when both group arrays are given and
 *   q_group[i] == b_group[j] (e.g. image ids: points of one image overlap), and, under MMC_KNN_EXCLUDE_SELF (query == base only), when
 *   it is row q_first + i itself.  Both group arrays or neither; they are host memory with MMC_IN_HOST in flags, else device memory.
 * Outputs (nq x k, host memory with MMC_OUT_HOST, else on the sets' device): index relative to b_first, best first; score; label
 *   (may be NULL) = the base row's stored class index.  Where fewer than k rows are eligible the tail holds index -1, score -inf,
 *   label -1; nb = 0 fills everything with that.  nq = 0 is MMC_OK and writes nothing.
 * MMC_ERR_ARG, nothing written: ranges outside their set or longer than 2^31 - 1, k outside [1, MMC_KNN_MAX_K], unequal dim or device,
 *   an unknown metric or flag, EXCLUDE_SELF on two different sets, one group array without the other, NULL index / score.
 * Work: one workgroup owns a tile of MMC_KNN_TILE_ROWS query rows and one contiguous range of base tiles; the base tiles T_b =
 *   ceil(nb / 128) are split over S = min(MMC_KNN_MAX_SPLITS, T_b, max(1, 1024 / T_q)) ranges, T_q = ceil(min(nq, MMC_KNN_CHUNK_ROWS) / 128)
 *   -- a function of nq and nb alone --, range s holding tiles [s * T_b / S, (s + 1) * T_b / S); a second launch merges the S lists per
 *   query.  Queries are walked in chunks of MMC_KNN_CHUNK_ROWS, so the per-call scratch (allocated and freed inside the call) is at most
 *   36 MiB + 12 bytes per base row, whatever nq.  Runs on `hip_stream` and synchronises it before returning. */
#define MMC_KNN_MAX_K 32
#define MMC_KNN_DOT 0
#define MMC_KNN_COSINE 1
#define MMC_KNN_L2 2
#define MMC_KNN_EXCLUDE_SELF 4u  /* flag; only legal when query == base */
#define MMC_KNN_TILE_ROWS 128
#define MMC_KNN_CHUNK_ROWS 8192
#define MMC_KNN_MAX_SPLITS 16
int mmc_featureset_knn(mmc_featureset* query, int64_t q_first, int64_t nq, mmc_featureset* base, int64_t b_first, int64_t nb, int k,
                       int metric, const int32_t* q_group /* nq or NULL */, const int32_t* b_group /* nb or NULL */,
                       int32_t* index /* nq x k */, float* score /* nq x k */, int32_t* label /* nq x k or NULL */, unsigned flags,
                       void* hip_stream);

/* ---- logit calibration: temperature, bias and vector scaling of the trained head's logits -----------------------------------------
 * Extends: the reference's balancing study closes on "Platt-scaling parameters or temperature scaling on top of it should be
 *   investigated" (docs/research/balancing-experiments.md:142).  mmc_trainer_set_loss's logit_prior is the training-time half of that
 *   line; this is the test-time half.  The Platt stage above is linear in the softmax probability, not in the logit, and cannot undo a
 *   plain over-confident softmax; the remedies below are affine in the logits z and fold exactly into the last Linear layer
 *   (mermaid_classifier_amd/logit_scaling.py: LogitScaling.fold), so every consumer of a head keeps working, the Platt stage on top.
 *   No reference counterpart: THIS TEXT IS THE DEFINITION.  No gain on reef data has been measured.
 * Inputs: N stored rows of raw logits z_n (fp32, as mmc_trainer_logits gives them) with labels y_n; parameters a, c (K doubles each).
 *   All arithmetic is float64 on the fp32 inputs.
 *     u_nk  = a_k z_nk + c_k
 *     lse_n = max_k u_nk + log sum_k exp(u_nk - max_k u_nk)        p_nk = exp(u_nk - lse_n)
 *     F(a,c) = sum_n (lse_n - u_n,y_n)  +  (l2 N / 2) (|a - 1|^2 + |c|^2)              l2 >= 0
 *   With theta = (a, c) in R^2K and r = p - onehot(y), the gradient of the data term is g_a = sum_n z_n (.) r_n, g_c = sum_n r_n; with
 *   v_n = [z_n (.) p_n ; p_n] its Hessian is H = D - sum_n v_n v_n^T, D diagonal plus the a_k-c_k coupling: D_aa[k] = sum z^2 p,
 *   D_cc[k] = sum p, D_ac[k] = sum z p.
 * Modes pick a subspace of theta:
 *   TEMPERATURE  a = s 1, c = 0: one parameter s = 1 / T; gradient sum_k g_a[k], Hessian sum_kl H_aa[k,l]
 *   BIAS         a = 1, c free               VECTOR   both free
 *   F is convex in every mode.  Two cases have no finite minimiser:
 *   absent classes   a class with no stored row has dF/dc_k = sum_n p_nk > 0 everywhere.  In BIAS and VECTOR such classes are frozen
 *                    at the identity (a_k = 1, c_k = 0), left out of the active parameters and reported in `frozen`, whatever l2 is.
 *   separable rows with l2 = 0   the fit ends at the tolerance or at the trial cap and returns the last accepted, finite iterate with
 *                    converged = 0 / 1; never NaN or inf.
 * mmc_logitcal_stats: one pass over the store (csrc/logit_scaling.hip).  Rows are cut into blocks of MMC_LOGITCAL_BLOCK_ROWS in
 *   stored order; a block's sums run in a fixed order, the blocks' partials are folded in block order; no float atomics.  The Hessian
 *   is accumulated in fp64 (v_mfma_f64_16x16x4_f64 over 16 x 16 tiles of the upper triangle) and returned symmetric bit for bit.  The
 *   row maximum is subtracted before exp: |a_k z_nk| in the thousands gives finite results.  The bits of every output depend on the
 *   stored logits, labels, K, a, c and N only -- not on how the rows were split over add_* calls, on the device or on the environment;
 *   hess = NULL gives the nll_sum / grad bits of the call with a Hessian.
 * mmc_logitcal_fit: damped Newton on the active parameters from the identity (csrc/logit_newton.h, host, float64).  d solves
 *   (H + lambda tau I) d = -g by Cholesky, tau = trace(H) / dim, H and g with the ridge: Levenberg damping with a multiple of the
 *   IDENTITY, which keeps every step orthogonal to the null direction c -> c + t 1 (nothing frozen), so c stays zero-mean from c = 0.
 *   lambda starts at 1e-3 (x 8 while the factorisation fails).  A trial point theta + d is accepted iff F there is finite and <= F;
 *   then lambda <- max(lambda / 8, 1e-12), else lambda <- 8 lambda.  Stops when max|g_active| / N <= tol (converged = 1) or after
 *   max_trials trial points (converged = 0).  Trial points are evaluated without the Hessian, accepted points once more with it.
 *   Outputs: a, cc (K each), frozen (K or NULL), the MEAN data term (sum / N) at the identity and at the returned point, the number
 *   of trial points.
 * Every call synchronises `hip_stream` before it returns.  MMC_ERR_ARG, with nothing launched: a NULL handle or output, K outside
 *   [2, MMC_LOGITCAL_MAX_CLASSES], a mode outside the three, l2 < 0, tol <= 0, max_trials outside [1, 1000], non-finite a / cc /
 *   logits, a label outside [0, K), a trainer / set / device mismatch, fit or stats with no rows.  mmc_logitcal_create writes
 *   *out = NULL first on every error path. */
#define MMC_LOGITCAL_MAX_CLASSES 128
#define MMC_LOGITCAL_BLOCK_ROWS 1024
#define MMC_LOGITCAL_TEMPERATURE 0
#define MMC_LOGITCAL_BIAS 1
#define MMC_LOGITCAL_VECTOR 2
typedef struct mmc_logitcal mmc_logitcal;
int mmc_logitcal_create(int K, int device, mmc_logitcal** out);
void mmc_logitcal_destroy(mmc_logitcal* c);
int64_t mmc_logitcal_rows(const mmc_logitcal* c);
/* raw logits of t's current parameters; they stay on the device (fp32) */
int mmc_logitcal_add_features(mmc_logitcal* c, mmc_trainer* t, const float* X, const int32_t* y, int64_t n, void* hip_stream);
int mmc_logitcal_add_set(mmc_logitcal* c, mmc_trainer* t, mmc_featureset* fs, int64_t first, int64_t n, void* hip_stream);
/* caller's logits (host, n x K fp32, finite) */
int mmc_logitcal_add_logits(mmc_logitcal* c, const float* logits, const int32_t* y, int64_t n, void* hip_stream);
/* data term, gradient (2K: a then c), Hessian (2K x 2K row-major, or NULL), per-class row counts (K, or NULL) at (a, cc) */
int mmc_logitcal_stats(mmc_logitcal* c, const double* a, const double* cc, double* nll_sum, double* grad, double* hess,
                       int64_t* counts, void* hip_stream);
int mmc_logitcal_fit(mmc_logitcal* c, int mode, double l2, double tol, int max_trials, double* a, double* cc, uint8_t* frozen /* K or NULL */,
                     double* nll_before, double* nll_after, int32_t* trials, int32_t* converged, void* hip_stream);

/* ---- multi-GPU: the gather of the sharded path --------------------------------------------------------------------
 * The path shards by patches (contiguous blocks of the row range per rank, weights replicated, no exchange during compute);
 * its one exchange step is the all-gather of the ranks' (n_r, 1280) feature blocks.  Replaces: nothing in the reference's
 * code -- it scales out as one job per source id (scripts/launch_processing.py:59-66, 199-233) and the matrices meet on S3;
 * SURVEY.md section 8(b) sketches this entry.  The Python package does the same through torch.distributed
 * (mermaid_classifier_amd/dist.py: FeatureGatherer); these entries give a non-Python host the same step through this
 * header alone.  One process per GPU; librccl is resolved at the first call (dlopen: the copy the process already has,
 * else ROCm's; MMC_RCCL_LIBRARY overrides), so single-GPU users never load it.
 *   mmc_dist_unique_id  rank 0 makes the 128-byte id and hands it to the other ranks out of band (file, env, TCP, MPI)
 *   mmc_dist_create     collective: every rank calls it with the same id, its rank, the world size and its device
 *   mmc_gather_features collective, asynchronous on `hip_stream`: local = this rank's n_local x dim fp32 block (device),
 *                       all = sum(counts) x dim (device) on EVERY rank, rank r's block at row sum(counts[0..r));
 *                       counts = host array of `world` block heights, or NULL when every rank holds n_local rows. */
#define MMC_DIST_ID_BYTES 128
typedef struct mmc_dist mmc_dist;
int mmc_dist_unique_id(unsigned char id[MMC_DIST_ID_BYTES]);
int mmc_dist_create(const unsigned char id[MMC_DIST_ID_BYTES], int rank, int world, int device, mmc_dist** out);
void mmc_dist_destroy(mmc_dist* d);
int mmc_gather_features(mmc_dist* d, const float* local, int64_t n_local, int dim, const int64_t* counts, float* all,
                        void* hip_stream);

/* ---- head ensembles --------------------------------------------------------------------------
 * An ensemble is M members, 1 <= M <= MMC_ENSEMBLE_MAX: existing mmc_head handles on one device with the same input_dim and the
 * same K <= MMC_ENSEMBLE_MAX_CLASSES (their depths and hidden widths are free: a sweep holds different architectures).  The
 * ensemble borrows the heads -- they must outlive it and stay usable on their own; its activations, logits and staging are its own.
 * A point is G consecutive rows, 1 <= G <= MMC_VIEWS_MAX, as in mmc_head_topk_views.  Per point and class, in fp32:
 *   v_{j,g} = the probability mmc_head_predict of member j writes for view row g, bit for bit
 *   m_j     = (v_{j,0} + ... + v_{j,G-1}) / (float)G      summed left to right in view order (the views definition)
 *   e       = (m_0 + ... + m_{M-1}) / (float)M            summed left to right in member order
 * With M = 1, e has the bits of mmc_head_topk_views; with M = 1 and G = 1 those of mmc_head_topk.  The k best classes of e are
 * chosen as mmc_head_topk chooses them: score descending, equal scores in class order, k distinct classes even for NaN rows.
 * Per point also MMC_ENSEMBLE_STATS floats, with H(p) = -sum_c p_c log p_c in nats and a class with p_c == 0 adding 0:
 *   stats[0] = H(e)                    the predictive entropy
 *   stats[1] = (1/M) sum_j H(m_j)      the expected member entropy
 *   stats[2] = stats[0] - stats[1]     the mutual information between prediction and member: the members' disagreement.  It is >= 0
 *                                      in exact arithmetic (Jensen); it is stored as computed and rounding can leave it just below 0
 * and votes (int32): the members whose own first-maximum class of m_j equals the ensemble's best class.  The entropy sums are
 * accumulated in double (lane-strided partials, a fixed butterfly, members in order) and rounded to fp32 once; there are no
 * atomics, so the bits depend on the logits, M, G and K only.  A row with NaN features has NaN stats.
 * The Linear layers of all members run as one launch per layer index, each output with the bits of the member's own launches; the
 * mean, the selection and the stats run in one kernel, and nothing rows x K is written unless proba is asked for.
 * Chunking: internal chunks hold mmc_ensemble_chunk_rows rows -- the largest multiple of G with M x rows inside one head's chunk
 * of 65536 rows -- so a point is never split; chunking changes no bit.  Flags, streams, the feature buffer and the 4096-patch
 * chunks of mmc_ensemble_classify_patches behave as in mmc_head_topk_views / mmc_classify_patches_views.
 * mmc_ensemble_evaluate / _set: the contract of mmc_head_evaluate / mmc_head_evaluate_set on e (G = 1): est, score, rank, p_true per
 * row, the MMC_EVAL_TOTALS totals, confusion and rank_hist by the same rules (label map, unknown and non-finite rows, integer
 * atomics: independent of grid and chunking), plus stats and votes per row (host pointers, like the other per-row outputs).
 * Errors: MMC_ERR_ARG with a message, before anything is launched or written, for a count outside [1, MMC_ENSEMBLE_MAX], a NULL
 * member, members that differ in K, input_dim or device, K > MMC_ENSEMBLE_MAX_CLASSES, G or k out of range, NULL required pointers,
 * and whatever mmc_head_evaluate / mmc_head_evaluate_set reject. */
#define MMC_ENSEMBLE_MAX 16
#define MMC_ENSEMBLE_MAX_CLASSES 2048
#define MMC_ENSEMBLE_STATS 3
typedef struct mmc_ensemble mmc_ensemble;
int mmc_ensemble_create(mmc_head* const* members, int count, mmc_ensemble** out);
void mmc_ensemble_destroy(mmc_ensemble* e);
int mmc_ensemble_size(const mmc_ensemble* e);
int mmc_ensemble_num_classes(const mmc_ensemble* e);
int mmc_ensemble_input_dim(const mmc_ensemble* e);
int mmc_ensemble_chunk_rows(const mmc_ensemble* e, int G);   /* rows per internal chunk, a multiple of G; 0 for a bad argument */
int mmc_ensemble_topk(mmc_ensemble* e, const float* feats /* (n_points*G) x input_dim, point-major */, int64_t n_points, int G, int k,
                      int32_t* idx /* n_points x k */, float* scores /* n_points x k */, float* proba /* n_points x K or NULL */,
                      float* stats /* n_points x MMC_ENSEMBLE_STATS or NULL */, int32_t* votes /* n_points or NULL */,
                      unsigned flags, void* hip_stream);
int mmc_ensemble_classify_patches(mmc_backbone* bb, mmc_ensemble* e, const void* patches /* (n_points*G) x 224x224x3 */,
                                  int64_t n_points, int G, int k, int32_t* idx, float* scores, float* stats /* or NULL */,
                                  int32_t* votes /* or NULL */, unsigned flags, void* hip_stream);
int mmc_ensemble_evaluate(mmc_ensemble* e, const float* feats, const int32_t* y, int64_t n, const int32_t* label_map, int n_labels,
                          int32_t* est, float* score, int32_t* rank, float* p_true, float* stats /* n x MMC_ENSEMBLE_STATS or NULL */,
                          int32_t* votes /* n or NULL */, int64_t* totals, int64_t* confusion, int64_t* rank_hist, unsigned flags,
                          void* hip_stream);
int mmc_ensemble_evaluate_set(mmc_ensemble* e, mmc_featureset* fs, int64_t first, int64_t n, const int32_t* label_map, int n_labels,
                              int32_t* est, float* score, int32_t* rank, float* p_true, float* stats, int32_t* votes, int64_t* totals,
                              int64_t* confusion, int64_t* rank_hist, void* hip_stream);

/* ---- distillation: per-row soft targets in the loss stage of resident passes; a head ensemble distilled into one head ---------------
 * Extends: the loss of TorchMLPClassifier.partial_fit (torch_classifier.py:226-303), whose targets are hard labels, and the soft-label
 *   form of "taxonomy-aware loss", whose targets are keyed by class (K x K), by targets keyed by row (N x K): the distillation loss of
 *   Hinton et al. 2015 ("Distilling the knowledge in a neural network").  It lets an mmc_ensemble, which no artifact format carries,
 *   be trained into one Linear -> ReLU -> ... -> Linear head.  No counterpart in the reference and no measured gain on reef data.  It
 *   sits in the loss stage alone: forward, backward GEMMs, L2, clipping, EMA, the schedule, dropout, batch normalisation, class
 *   weights, the logit prior, smoothing and focal modulation (in b_i only), row weights and group DRO are untouched and compose with
 *   it; evaluation, early stopping, calibration and export never see it.  With nothing set a pass launches the kernels, and gives the
 *   bits, of a trainer this was never called on; in a group the members without targets keep their kernels.
 * A target set is an N x K fp32 matrix of per-row class distributions on one device; row i belongs to row i of a feature set.  It
 *   never holds an invalid row.  A row is valid when every entry is finite and >= 0 and its sum, taken in double in class order, is
 *   within 1e-3 of 1 (a condition, not a measurement: a normalised fp32 row of K <= 2048 classes is off by about (K + 8) 2^-24).
 *   Both fill routes write the new rows past the committed row count, validate them on the device (one wave per row, the first bad
 *   row reduced with an integer atomic minimum), read one result back and commit the rows only if none is invalid; otherwise
 *   MMC_ERR_ARG names the first bad row and why ("row 17: entry 5 = nan ...", "row 17 sums to 0.93 ...") and the row count stays.
 *   mmc_targetset_append numbers the row within the rows of that call (row 0 is P's first row, wherever it would have landed in
 *   the set); mmc_ensemble_predict_set numbers it by row of the feature set.
 *   Growth allocates the new buffer first: a refused call changes nothing.  rows x K is at most MMC_TARGETSET_MAX_CELLS, checked
 *   arithmetically before anything is allocated.
 * mmc_targetset_append takes n x K rows from host (MMC_IN_HOST) or device (MMC_IN_DEVICE) memory; mmc_targetset_read writes rows
 *   [first, first + n) to host memory.  mmc_ensemble_predict_set appends n rows: row j is the ensemble mean e ("head ensembles") of
 *   set row first + j at G = 1, with the bits mmc_ensemble_topk writes into proba for that row, made in the ensemble's own chunks
 *   straight into the target set; an ensemble of one member gives mmc_head_predict's bits.  A feature row whose NaN reaches a member's
 *   logits (a hidden ReLU is fmaxf(., 0) and drops it) makes a NaN target row, so the fill is refused, the bad row named by its set row.
 * mmc_trainer_set_distillation(t, alpha, temperature): alpha in [0, 1], temperature tau in [0.25, 64]; alpha = 0 restores the default.
 * Notation (that of "group-robust training" and "taxonomy-aware loss").  u = z + prior, w the class weights, t = y_i, s_i the row's
 *   normaliser exactly as the other loss kernels form it (inv_wsum, or rw[row] * inv_wsum, or r_i with groups); b_i and db_i/dz the
 *   trainer's own row term and gradient before normalisation, formed operation for operation as the general form of
 *   mmc_trainer_set_loss (at its defaults the plain weighted cross-entropy: b_i = (1.0f w_t) nll).  q_i is row rho(i) of the target
 *   set, rho(i) = visit[pos] where the pass has a visiting order, else pos, pos the position in the pass; the row is read in place.
 *     tau = 1:   qt = q_i as stored (not renormalised: its fp32 sum stands where 1 would), pt = softmax(u), the hard term's own
 *     tau != 1:  qt_c = q_c^(1/tau) / sum_c' q_c'^(1/tau), formed as exp(g_c - mg - log sum exp(g_c' - mg)) with g_c = logf(q_c) it,
 *                it = (float)(1 / tau), over the classes with q_c > 0; an entry of 0 stays 0.  pt = softmax(u it), with its own
 *                maximum and sum.
 *     k_i        = -sum_c qt_c log pt_c                     a class with qt_c == 0 adds 0
 *     l_i        = s_i [ (1 - alpha) b_i + alpha tau^2 w_t k_i ]
 *     dl_i/dz_c  = s_i [ (1 - alpha) db_i/dz_c + alpha tau w_t (pt_c sum_c' qt_c' - qt_c) ]
 *   with (float)(1 - alpha), (float)(alpha tau) and (float)(alpha tau^2) made from doubles on the host and multiplied by w_t in the
 *   kernel.  The reported loss is the sum of l_i plus the L2 term: the cross-entropy form, which includes the teacher's entropy, not
 *   the KL divergence.  Every output is finite on any finite logits row and any valid target row.
 * The _distill passes are the _weighted passes with one more argument.  ts == NULL is mmc_trainer_partial_fit_set_weighted, bit for
 *   bit.  In the group form `targets` is an array of `count` pointers, or NULL; a member whose entry is NULL runs exactly as in the
 *   _weighted call; members may share one set (it is only read) or use different ones.  The results do not depend on
 *   MMC_TRAIN_CHUNK_ROWS, a member of a group matches its solo pass bit for bit, and a pass is bit-reproducible.  The plain, mixed
 *   and weighted entry points on a trainer with distillation set run as ever.
 * Checked before the first launch and before any member changes, on top of the _weighted call's checks: a target set whose K is not
 *   the trainer's, whose row count is not the feature set's, or that lives on another device; targets on a trainer with alpha == 0
 *   ("needs mmc_trainer_set_distillation(alpha > 0)"); targets on a trainer with a hierarchy -> MMC_ERR_ARG.  Distillation and
 *   mmc_trainer_set_hierarchy (levels or soft labels) exclude each other: whichever setter comes second refuses.  Mixup with
 *   targets is refused by construction: no entry point takes a mixing plan and a target set (the Python surface raises ValueError).  alpha or temperature out of range or NaN -> MMC_ERR_ARG, the trainer left as it was.
 * mmc_trainer_loss_gradient_distill runs the stage's own kernel on caller logits and caller target rows q (n x K, host), n in
 *   [1, 16384] rows taken as one mini-batch, position i reading row i; row_weight may be NULL.  The rows of q pass the same validity
 *   rule first (a bad row is numbered within q).  mmc_trainer_loss_gradient_distill_weighted is mmc_trainer_loss_gradient_weighted
 *   with the same q: its arguments, checks and outputs, groups and the explicit log q included, so that group DRO over the distilled
 *   stage (normaliser r_i, then dro_update_kernel / row_scale_kernel on its row_loss / dlogits) can be checked per element; with
 *   row_group NULL it is mmc_trainer_loss_gradient_distill, bit for bit. */
#define MMC_TARGETSET_MAX_CELLS 1073741824LL  /* 2^30: 4 GiB of resident targets */
typedef struct mmc_targetset mmc_targetset;
int mmc_targetset_create(int K, int device, int64_t reserve_rows, mmc_targetset** out);
void mmc_targetset_destroy(mmc_targetset* ts);
int64_t mmc_targetset_rows(const mmc_targetset* ts);
int mmc_targetset_num_classes(const mmc_targetset* ts);
int mmc_targetset_append(mmc_targetset* ts, const float* P /* n x K */, int64_t n, unsigned flags, void* hip_stream);
int mmc_targetset_read(mmc_targetset* ts, int64_t first, int64_t n, float* P /* n x K, host */, void* hip_stream);
int mmc_ensemble_predict_set(mmc_ensemble* e, mmc_featureset* fs, int64_t first, int64_t n, mmc_targetset* ts, void* hip_stream);
int mmc_trainer_set_distillation(mmc_trainer* t, double alpha, double temperature);
int mmc_trainer_partial_fit_set_distill(mmc_trainer* t, mmc_featureset* fs, mmc_targetset* ts /* or NULL */, const int64_t* visit,
                                        const float* row_weight /* n or NULL */, const int32_t* row_group /* n or NULL */, int64_t n,
                                        int batch_size, double* avg_loss, void* hip_stream);
int mmc_trainer_group_partial_fit_set_distill(mmc_trainer* const* trainers, int count, mmc_featureset* fs,
                                              mmc_targetset* const* targets /* count pointers, or NULL */, const int64_t* const* visit,
                                              const float* const* row_weight, const int32_t* const* row_group, const int64_t* n,
                                              const int* batch_size, double* avg_loss, void* hip_stream);
int mmc_trainer_loss_gradient_distill(mmc_trainer* t, const float* logits, const int32_t* y, const float* q /* n x K, host */,
                                      const float* row_weight /* n or NULL */, int64_t n, float* dlogits, float* row_loss,
                                      void* hip_stream);
int mmc_trainer_loss_gradient_distill_weighted(mmc_trainer* t, const float* logits, const int32_t* y, const float* q /* n x K, host */,
                                               const float* row_weight, const int32_t* row_group, const double* log_q_in, double eta,
                                               int n_groups, int64_t n, float* dlogits, float* row_loss, double* log_q_out,
                                               double* group_loss /* n_groups, NaN where none */, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* MMC_H */
