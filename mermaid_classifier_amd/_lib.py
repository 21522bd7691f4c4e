"""ctypes binding of libmermaid_mi355.so (include/mmc.h).  There is no CPU fallback:
importing this module without the built library, or creating a handle without a HIP
device, raises."""

from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

_HERE = Path(__file__).resolve().parent
LIB_NAME = "libmermaid_mi355.so"
LIB_PATH = _HERE / LIB_NAME

MMC_OK, MMC_ERR_ARG, MMC_ERR_WEIGHTS, MMC_ERR_HIP, MMC_ERR_NOMEM = 0, 1, 2, 3, 4
MMC_PRECISION_FP8 = 1   # include/mmc.h: flags of mmc_backbone_create_ex
MMC_IN_HOST, MMC_OUT_HOST = 1, 2
MMC_IN_DEVICE = 0
MMC_EVAL_TOTALS = 5   # include/mmc.h: length of mmc_head_evaluate's totals
MMC_GROUPED_MAX_BINS, MMC_COVER_SUMS = 64, 8   # include/mmc.h: mmc_head_evaluate_grouped
MMC_GROUPED_MAX_SOURCE_CELLS, MMC_GROUPED_MAX_COVER_CELLS = 1 << 26, 1 << 28
MMC_CATEGORY_MAX, MMC_CATEGORY_MAX_BINS = 64, 20   # include/mmc.h: mmc_head_evaluate_categories
MMC_CATEGORY_MIN_BINS, MMC_CATEGORY_ROWS_PER_BIN = 2, 10   # calibration.py:137: n_bins_cat = min(20, max(2, n // 10))
MMC_RANKED_MAX_K = 16   # include/mmc.h: selection rounds of mmc_head_evaluate_ranked
MMC_TRAINER_GROUP_MAX = 16   # include/mmc.h: members of one mmc_trainer_group_partial_fit_set call
MMC_VIEWS_MAX = 16   # include/mmc.h MMC_VIEWS_MAX: view codes 0..15, and at most 16 views per point
MMC_COVER_MAX_ITERS, MMC_COVER_MAX_CELLS = 1000, 1 << 30   # include/mmc.h: cover estimation
MMC_SCATTER_CHUNK_ROWS, MMC_SCATTER_MAX_SPLITS, MMC_SCATTER_MAX_DIM = 256, 16, 2048   # include/mmc.h: feature transforms

MMC_KNN_MAX_K, MMC_KNN_DOT, MMC_KNN_COSINE, MMC_KNN_L2, MMC_KNN_EXCLUDE_SELF = 32, 0, 1, 2, 4   # include/mmc.h: nearest neighbours
MMC_KNN_TILE_ROWS, MMC_KNN_CHUNK_ROWS, MMC_KNN_MAX_SPLITS = 128, 8192, 16
MMC_LOGITCAL_MAX_CLASSES, MMC_LOGITCAL_BLOCK_ROWS = 128, 1024   # include/mmc.h: logit calibration
MMC_LOGITCAL_TEMPERATURE, MMC_LOGITCAL_BIAS, MMC_LOGITCAL_VECTOR = 0, 1, 2
MMC_ENSEMBLE_MAX, MMC_ENSEMBLE_MAX_CLASSES, MMC_ENSEMBLE_STATS = 16, 2048, 3   # include/mmc.h: head ensembles

# every symbol include/mmc.h declares (tests/test_abi.py checks the library exports them all)
SYMBOLS = [
    "mmc_last_error", "mmc_version", "mmc_device_count",
    "mmc_backbone_create", "mmc_backbone_create_ex", "mmc_fp8_e4m3_encode", "mmc_backbone_destroy", "mmc_feature_dim", "mmc_backbone_max_batch", "mmc_backbone_lanes",
    "mmc_backbone_workspace_bytes", "mmc_backbone_extract", "mmc_backbone_read_activation",
    "mmc_backbone_profile", "mmc_backbone_graph_stats", "mmc_crop_patches", "mmc_crop_patches_views",
    "mmc_head_create", "mmc_head_destroy", "mmc_head_input_dim", "mmc_head_num_classes", "mmc_head_predict", "mmc_head_topk", "mmc_classify_patches",
    "mmc_head_topk_views", "mmc_classify_patches_views",
    "mmc_trainer_create", "mmc_trainer_destroy", "mmc_trainer_partial_fit", "mmc_trainer_partial_fit_ordered", "mmc_trainer_get_params", "mmc_trainer_adam_state",
    "mmc_trainer_logits", "mmc_trainer_evaluate", "mmc_trainer_evaluate_q32", "mmc_trainer_set_loss", "mmc_trainer_loss_gradient",
    "mmc_calibrator_create", "mmc_calibrator_destroy", "mmc_calibrator_add_features", "mmc_calibrator_add_scores", "mmc_calibrator_fit",
    "mmc_featureset_create", "mmc_featureset_destroy", "mmc_featureset_rows", "mmc_featureset_dim", "mmc_featureset_append", "mmc_featureset_read",
    "mmc_trainer_partial_fit_set", "mmc_trainer_group_partial_fit_set", "mmc_trainer_evaluate_set_q32", "mmc_calibrator_add_set",
    "mmc_trainer_evaluate_classes", "mmc_trainer_evaluate_classes_set",
    "mmc_head_evaluate", "mmc_head_evaluate_set", "mmc_head_evaluate_grouped", "mmc_head_evaluate_grouped_set",
    "mmc_head_evaluate_categories", "mmc_head_evaluate_categories_set",
    "mmc_head_evaluate_ranked", "mmc_head_evaluate_ranked_set",
    "mmc_cover_proba", "mmc_head_cover", "mmc_head_cover_set",
    "mmc_featureset_moments", "mmc_featureset_scatter", "mmc_featureset_transform",
    "mmc_featureset_knn",
    "mmc_logitcal_create", "mmc_logitcal_destroy", "mmc_logitcal_rows", "mmc_logitcal_add_features", "mmc_logitcal_add_set",
    "mmc_logitcal_add_logits", "mmc_logitcal_stats", "mmc_logitcal_fit",
    "mmc_trainer_set_dropout", "mmc_trainer_partial_fit_set_mixed", "mmc_trainer_group_partial_fit_set_mixed", "mmc_trainer_loss_gradient_mixed",
    "mmc_trainer_set_lr_schedule", "mmc_trainer_lr_at", "mmc_lr_schedule_at", "mmc_trainer_set_grad_clip", "mmc_trainer_grad_norms",
    "mmc_trainer_set_ema", "mmc_trainer_ema_state", "mmc_trainer_eval_weights", "mmc_trainer_optimizer_options",
    "mmc_trainer_set_group_dro", "mmc_trainer_group_dro_state", "mmc_trainer_partial_fit_set_weighted",
    "mmc_trainer_group_partial_fit_set_weighted", "mmc_trainer_loss_gradient_weighted",
    "mmc_trainer_set_hierarchy",
    "mmc_trainer_set_batch_norm", "mmc_trainer_batch_norm_state", "mmc_trainer_folded_params", "mmc_trainer_norm_stage",
    "mmc_dist_unique_id", "mmc_dist_create", "mmc_dist_destroy", "mmc_gather_features",
    "mmc_ensemble_create", "mmc_ensemble_destroy", "mmc_ensemble_size", "mmc_ensemble_num_classes", "mmc_ensemble_input_dim",
    "mmc_ensemble_chunk_rows", "mmc_ensemble_topk", "mmc_ensemble_classify_patches", "mmc_ensemble_evaluate", "mmc_ensemble_evaluate_set",
    "mmc_targetset_create", "mmc_targetset_destroy", "mmc_targetset_rows", "mmc_targetset_num_classes", "mmc_targetset_append",
    "mmc_targetset_read", "mmc_ensemble_predict_set", "mmc_trainer_set_distillation", "mmc_trainer_partial_fit_set_distill",
    "mmc_trainer_group_partial_fit_set_distill", "mmc_trainer_loss_gradient_distill",
    "mmc_trainer_loss_gradient_distill_weighted",
]
# include/mmc.h, "optimiser options"
MMC_LR_CONSTANT, MMC_LR_LINEAR, MMC_LR_COSINE = 0, 1, 2
MMC_WEIGHTS_RAW, MMC_WEIGHTS_AVERAGED = 0, 1
MMC_DRO_MAX_GROUPS = 1024   # include/mmc.h, "group-robust training"
MMC_HIER_MAX_LEVELS = 4   # include/mmc.h, "taxonomy-aware loss"
MMC_TARGETSET_MAX_CELLS = 1 << 30   # include/mmc.h, "distillation"


class LibraryMissingError(ImportError):
    pass


def _load() -> C.CDLL:
    path = Path(os.environ.get("MMC_LIBRARY", LIB_PATH))
    if not path.is_file():
        raise LibraryMissingError(
            f"{path} not found: build it with `python -m mermaid_classifier_amd.build` "
            "(hipcc --offload-arch=gfx950). mermaid_classifier_amd has no CPU fallback.")
    # PyTorch-ROCm wheels bundle their own libamdhip64.so.  Two HIP runtimes in one process do not share
    # devices, so make sure torch's copy is the one already resident before our library resolves its
    # libamdhip64 dependency (otherwise /opt/rocm's would load first and torch tensors would live in a
    # different runtime than our kernels).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(str(path))
    vp, i32, i64, u32, sz = C.c_void_p, C.c_int, C.c_int64, C.c_uint, C.c_size_t
    fp = C.POINTER(C.c_float)
    lib.mmc_last_error.restype = C.c_char_p
    lib.mmc_last_error.argtypes = []
    lib.mmc_version.restype = i32
    lib.mmc_device_count.restype = i32
    lib.mmc_backbone_create.restype = i32
    lib.mmc_backbone_create.argtypes = [vp, sz, i32, i32, i32, C.POINTER(vp)]
    lib.mmc_backbone_create_ex.restype = i32
    lib.mmc_backbone_create_ex.argtypes = [vp, sz, i32, i32, i32, u32, C.POINTER(vp)]
    lib.mmc_fp8_e4m3_encode.restype = i32
    lib.mmc_fp8_e4m3_encode.argtypes = [vp, vp, sz]
    lib.mmc_backbone_destroy.restype = None
    lib.mmc_backbone_destroy.argtypes = [vp]
    lib.mmc_feature_dim.restype = i32
    lib.mmc_feature_dim.argtypes = [vp]
    lib.mmc_backbone_max_batch.restype = i32
    lib.mmc_backbone_max_batch.argtypes = [vp]
    lib.mmc_backbone_lanes.restype = i32
    lib.mmc_backbone_lanes.argtypes = [vp]
    lib.mmc_backbone_workspace_bytes.restype = sz
    lib.mmc_backbone_workspace_bytes.argtypes = [vp]
    lib.mmc_backbone_extract.restype = i32
    lib.mmc_backbone_extract.argtypes = [vp, vp, i64, vp, u32, vp]
    lib.mmc_backbone_read_activation.restype = i32
    lib.mmc_backbone_read_activation.argtypes = [vp, C.c_char_p, vp, sz, C.POINTER(sz)]
    lib.mmc_backbone_profile.restype = i32
    lib.mmc_backbone_profile.argtypes = [vp, vp, i64, vp, vp, vp, fp, C.POINTER(i32), i32, C.POINTER(i32)]
    lib.mmc_backbone_graph_stats.restype = i32
    lib.mmc_backbone_graph_stats.argtypes = [vp, C.POINTER(i64)]
    lib.mmc_crop_patches.restype = i32
    lib.mmc_crop_patches.argtypes = [vp, i32, i32, vp, i64, vp, u32, i32, vp]
    lib.mmc_crop_patches_views.restype = i32
    lib.mmc_crop_patches_views.argtypes = [vp, i32, i32, vp, i64, vp, vp, u32, i32, vp]
    lib.mmc_head_create.restype = i32
    lib.mmc_head_create.argtypes = [C.POINTER(fp), C.POINTER(fp), C.POINTER(i32), i32, fp, fp, i32, i32, C.POINTER(vp)]
    lib.mmc_head_destroy.restype = None
    lib.mmc_head_destroy.argtypes = [vp]
    lib.mmc_head_input_dim.restype = i32
    lib.mmc_head_input_dim.argtypes = [vp]
    lib.mmc_head_num_classes.restype = i32
    lib.mmc_head_num_classes.argtypes = [vp]
    lib.mmc_head_predict.restype = i32
    lib.mmc_head_predict.argtypes = [vp, vp, i64, vp, vp, u32, vp]
    lib.mmc_head_topk.restype = i32
    lib.mmc_head_topk.argtypes = [vp, vp, i64, i32, vp, vp, vp, u32, vp]
    lib.mmc_classify_patches.restype = i32
    lib.mmc_classify_patches.argtypes = [vp, vp, vp, i64, i32, vp, vp, u32, vp]
    lib.mmc_head_topk_views.restype = i32
    lib.mmc_head_topk_views.argtypes = [vp, vp, i64, i32, i32, vp, vp, vp, u32, vp]
    lib.mmc_classify_patches_views.restype = i32
    lib.mmc_classify_patches_views.argtypes = [vp, vp, vp, i64, i32, i32, vp, vp, u32, vp]
    f32 = C.c_float
    f64 = C.c_double
    lib.mmc_trainer_create.restype = i32
    lib.mmc_trainer_create.argtypes = [C.POINTER(fp), C.POINTER(fp), C.POINTER(i32), i32, f64, f64, f64, f64, f64, fp, i32, C.POINTER(vp)]
    lib.mmc_trainer_destroy.restype = None
    lib.mmc_trainer_destroy.argtypes = [vp]
    lib.mmc_trainer_partial_fit.restype = i32
    lib.mmc_trainer_partial_fit.argtypes = [vp, vp, vp, i64, i32, C.POINTER(C.c_double), vp]
    lib.mmc_trainer_partial_fit_ordered.restype = i32
    lib.mmc_trainer_partial_fit_ordered.argtypes = [vp, vp, vp, vp, i64, i32, C.POINTER(C.c_double), vp]
    lib.mmc_trainer_get_params.restype = i32
    lib.mmc_trainer_get_params.argtypes = [vp, C.POINTER(fp), C.POINTER(fp)]
    lib.mmc_trainer_adam_state.restype = i32
    lib.mmc_trainer_adam_state.argtypes = [vp, i32, i32, C.POINTER(fp), C.POINTER(fp), C.POINTER(C.c_longlong)]
    lib.mmc_trainer_logits.restype = i32
    lib.mmc_trainer_logits.argtypes = [vp, vp, i64, vp, vp]
    lib.mmc_trainer_set_loss.restype = i32
    lib.mmc_trainer_set_loss.argtypes = [vp, f64, f64, fp]
    lib.mmc_trainer_loss_gradient.restype = i32
    lib.mmc_trainer_loss_gradient.argtypes = [vp, vp, vp, i64, vp, vp, vp]
    lib.mmc_trainer_evaluate.restype = i32
    lib.mmc_trainer_evaluate.argtypes = [vp, vp, vp, i64, C.POINTER(i64), C.POINTER(f64), vp]
    lib.mmc_trainer_evaluate_q32.restype = i32
    lib.mmc_trainer_evaluate_q32.argtypes = [vp, vp, vp, i64, C.POINTER(i64), C.POINTER(i64), vp]
    lib.mmc_calibrator_create.restype = i32
    lib.mmc_calibrator_create.argtypes = [i32, i32, C.POINTER(vp)]
    lib.mmc_calibrator_destroy.restype = None
    lib.mmc_calibrator_destroy.argtypes = [vp]
    lib.mmc_calibrator_add_features.restype = i32
    lib.mmc_calibrator_add_features.argtypes = [vp, vp, vp, vp, i64, vp]
    lib.mmc_calibrator_add_scores.restype = i32
    lib.mmc_calibrator_add_scores.argtypes = [vp, vp, vp, i64, vp]
    lib.mmc_calibrator_fit.restype = i32
    lib.mmc_calibrator_fit.argtypes = [vp, vp, vp, vp, vp]
    lib.mmc_featureset_create.restype = i32
    lib.mmc_featureset_create.argtypes = [i32, i32, i32, i64, C.POINTER(vp)]
    lib.mmc_featureset_destroy.restype = None
    lib.mmc_featureset_destroy.argtypes = [vp]
    lib.mmc_featureset_rows.restype = i64
    lib.mmc_featureset_rows.argtypes = [vp]
    lib.mmc_featureset_dim.restype = i32
    lib.mmc_featureset_dim.argtypes = [vp]
    lib.mmc_featureset_append.restype = i32
    lib.mmc_featureset_append.argtypes = [vp, vp, vp, i64, u32, vp]
    lib.mmc_featureset_read.restype = i32
    lib.mmc_featureset_read.argtypes = [vp, i64, i64, vp, vp, vp]
    lib.mmc_trainer_partial_fit_set.restype = i32
    lib.mmc_trainer_partial_fit_set.argtypes = [vp, vp, vp, i64, i32, C.POINTER(C.c_double), vp]
    lib.mmc_trainer_group_partial_fit_set.restype = i32
    lib.mmc_trainer_group_partial_fit_set.argtypes = [C.POINTER(vp), i32, vp, C.POINTER(vp), C.POINTER(i64), C.POINTER(i32),
                                                      C.POINTER(C.c_double), vp]
    lib.mmc_trainer_evaluate_set_q32.restype = i32
    lib.mmc_trainer_evaluate_set_q32.argtypes = [vp, vp, i64, i64, C.POINTER(i64), C.POINTER(i64), vp]
    lib.mmc_calibrator_add_set.restype = i32
    lib.mmc_calibrator_add_set.argtypes = [vp, vp, vp, i64, i64, vp]
    lib.mmc_trainer_evaluate_classes.restype = i32
    lib.mmc_trainer_evaluate_classes.argtypes = [vp, vp, vp, i64, C.POINTER(i64), C.POINTER(i64), vp, vp]
    lib.mmc_trainer_evaluate_classes_set.restype = i32
    lib.mmc_trainer_evaluate_classes_set.argtypes = [vp, vp, i64, i64, C.POINTER(i64), C.POINTER(i64), vp, vp]
    lib.mmc_head_evaluate.restype = i32
    lib.mmc_head_evaluate.argtypes = [vp, vp, vp, i64, vp, i32, vp, vp, vp, vp, vp, vp, vp, u32, vp]
    lib.mmc_head_evaluate_set.restype = i32
    lib.mmc_head_evaluate_set.argtypes = [vp, vp, i64, i64, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    # the arguments of mmc_head_evaluate(_set), then image_offsets, n_images, source_of_image, n_sources, n_bins and the 11 group outputs
    grouped = [vp, i64, vp, i32, i32] + [vp] * 11
    lib.mmc_head_evaluate_grouped.restype = i32
    lib.mmc_head_evaluate_grouped.argtypes = [vp, vp, vp, i64, vp, i32, vp, vp, vp, vp, vp, vp, vp] + grouped + [u32, vp]
    lib.mmc_head_evaluate_grouped_set.restype = i32
    lib.mmc_head_evaluate_grouped_set.argtypes = [vp, vp, i64, i64, vp, i32, vp, vp, vp, vp, vp, vp, vp] + grouped + [vp]
    # the arguments of mmc_head_evaluate_grouped(_set), then category_of_class, n_categories and the 7 category outputs
    categories = grouped + [vp, i32] + [vp] * 7
    lib.mmc_head_evaluate_categories.restype = i32
    lib.mmc_head_evaluate_categories.argtypes = [vp, vp, vp, i64, vp, i32, vp, vp, vp, vp, vp, vp, vp] + categories + [u32, vp]
    lib.mmc_head_evaluate_categories_set.restype = i32
    lib.mmc_head_evaluate_categories_set.argtypes = [vp, vp, i64, i64, vp, i32, vp, vp, vp, vp, vp, vp, vp] + categories + [vp]
    # the arguments of mmc_head_evaluate(_set), then sim_level, n_levels, kmax, class_rank_hist, hier_hist
    ranked = [vp, i32, i32, vp, vp]
    lib.mmc_head_evaluate_ranked.restype = i32
    lib.mmc_head_evaluate_ranked.argtypes = [vp, vp, vp, i64, vp, i32, vp, vp, vp, vp, vp, vp, vp] + ranked + [u32, vp]
    lib.mmc_head_evaluate_ranked_set.restype = i32
    lib.mmc_head_evaluate_ranked_set.argtypes = [vp, vp, i64, i64, vp, i32, vp, vp, vp, vp, vp, vp, vp] + ranked + [vp]
    # group_offsets, n_groups, train_prior, strength, iters, count, soft_q32, unusable, prior, k, idx, scores
    cover = [vp, i64, vp, f64, i32, vp, vp, vp, vp, i32, vp, vp]
    lib.mmc_cover_proba.restype = i32
    lib.mmc_cover_proba.argtypes = [vp, i64, i32] + cover + [i32, u32, vp]
    lib.mmc_head_cover.restype = i32
    lib.mmc_head_cover.argtypes = [vp, vp, i64, i32] + cover + [u32, vp]
    lib.mmc_head_cover_set.restype = i32
    lib.mmc_head_cover_set.argtypes = [vp, vp, i64, i64, i32] + cover + [u32, vp]
    lib.mmc_featureset_moments.restype = i32
    lib.mmc_featureset_moments.argtypes = [vp, i64, i64, vp, vp, vp, u32, vp]
    lib.mmc_featureset_scatter.restype = i32
    lib.mmc_featureset_scatter.argtypes = [vp, i64, i64, vp, i32, vp, u32, vp]
    lib.mmc_featureset_transform.restype = i32
    lib.mmc_featureset_transform.argtypes = [vp, i64, i64, vp, vp, i32, vp, u32, vp]
    lib.mmc_featureset_knn.restype = i32
    lib.mmc_featureset_knn.argtypes = [vp, i64, i64, vp, i64, i64, i32, i32, vp, vp, vp, vp, vp, u32, vp]
    lib.mmc_logitcal_create.restype = i32
    lib.mmc_logitcal_create.argtypes = [i32, i32, C.POINTER(vp)]
    lib.mmc_logitcal_destroy.restype = None
    lib.mmc_logitcal_destroy.argtypes = [vp]
    lib.mmc_logitcal_rows.restype = i64
    lib.mmc_logitcal_rows.argtypes = [vp]
    lib.mmc_logitcal_add_features.restype = i32
    lib.mmc_logitcal_add_features.argtypes = [vp, vp, vp, vp, i64, vp]
    lib.mmc_logitcal_add_set.restype = i32
    lib.mmc_logitcal_add_set.argtypes = [vp, vp, vp, i64, i64, vp]
    lib.mmc_logitcal_add_logits.restype = i32
    lib.mmc_logitcal_add_logits.argtypes = [vp, vp, vp, i64, vp]
    lib.mmc_logitcal_stats.restype = i32
    lib.mmc_logitcal_stats.argtypes = [vp, vp, vp, C.POINTER(f64), vp, vp, vp, vp]
    lib.mmc_logitcal_fit.restype = i32
    lib.mmc_logitcal_fit.argtypes = [vp, i32, f64, f64, i32, vp, vp, vp, C.POINTER(f64), C.POINTER(f64), C.POINTER(i32), C.POINTER(i32), vp]
    lib.mmc_trainer_set_dropout.restype = i32
    lib.mmc_trainer_set_dropout.argtypes = [vp, f64, f64, C.c_uint64]
    lib.mmc_trainer_partial_fit_set_mixed.restype = i32
    lib.mmc_trainer_partial_fit_set_mixed.argtypes = [vp, vp, vp, vp, vp, i64, i32, C.POINTER(C.c_double), vp]
    lib.mmc_trainer_group_partial_fit_set_mixed.restype = i32
    lib.mmc_trainer_group_partial_fit_set_mixed.argtypes = [C.POINTER(vp), i32, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(i64),
                                                            C.POINTER(i32), C.POINTER(C.c_double), vp]
    lib.mmc_trainer_loss_gradient_mixed.restype = i32
    lib.mmc_trainer_loss_gradient_mixed.argtypes = [vp, vp, vp, vp, f32, i64, vp, vp, vp]
    ll = C.c_longlong
    lib.mmc_trainer_set_lr_schedule.restype = i32
    lib.mmc_trainer_set_lr_schedule.argtypes = [vp, i32, ll, ll, f64]
    lib.mmc_trainer_lr_at.restype = i32
    lib.mmc_trainer_lr_at.argtypes = [vp, ll, C.POINTER(f64)]
    lib.mmc_lr_schedule_at.restype = i32
    lib.mmc_lr_schedule_at.argtypes = [f64, i32, ll, ll, f64, ll, C.POINTER(f64)]
    lib.mmc_trainer_set_grad_clip.restype = i32
    lib.mmc_trainer_set_grad_clip.argtypes = [vp, f64]
    lib.mmc_trainer_grad_norms.restype = i32
    lib.mmc_trainer_grad_norms.argtypes = [vp, vp, i32, C.POINTER(i32)]
    lib.mmc_trainer_set_ema.restype = i32
    lib.mmc_trainer_set_ema.argtypes = [vp, f64]
    lib.mmc_trainer_ema_state.restype = i32
    lib.mmc_trainer_ema_state.argtypes = [vp, i32, C.POINTER(fp), C.POINTER(fp)]
    lib.mmc_trainer_eval_weights.restype = i32
    lib.mmc_trainer_eval_weights.argtypes = [vp, i32]
    lib.mmc_trainer_optimizer_options.restype = i32
    lib.mmc_trainer_optimizer_options.argtypes = [vp, C.POINTER(i32), C.POINTER(ll), C.POINTER(ll), C.POINTER(f64), C.POINTER(f64),
                                                  C.POINTER(f64), C.POINTER(i32)]
    lib.mmc_trainer_set_group_dro.restype = i32
    lib.mmc_trainer_set_group_dro.argtypes = [vp, i32, f64]
    lib.mmc_trainer_group_dro_state.restype = i32
    lib.mmc_trainer_group_dro_state.argtypes = [vp, i32, vp]
    lib.mmc_trainer_partial_fit_set_weighted.restype = i32
    lib.mmc_trainer_partial_fit_set_weighted.argtypes = [vp, vp, vp, vp, vp, i64, i32, C.POINTER(C.c_double), vp]
    lib.mmc_trainer_group_partial_fit_set_weighted.restype = i32
    lib.mmc_trainer_group_partial_fit_set_weighted.argtypes = [C.POINTER(vp), i32, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                                               C.POINTER(i64), C.POINTER(i32), C.POINTER(C.c_double), vp]
    lib.mmc_trainer_loss_gradient_weighted.restype = i32
    lib.mmc_trainer_loss_gradient_weighted.argtypes = [vp, vp, vp, vp, vp, vp, f64, i32, i64, vp, vp, vp, vp, vp]
    lib.mmc_trainer_set_hierarchy.restype = i32
    lib.mmc_trainer_set_hierarchy.argtypes = [vp, i32, vp, vp, vp]
    lib.mmc_trainer_set_batch_norm.restype = i32
    lib.mmc_trainer_set_batch_norm.argtypes = [vp, i32, f64, f64]
    lib.mmc_trainer_batch_norm_state.restype = i32
    lib.mmc_trainer_batch_norm_state.argtypes = [vp, i32] + [C.POINTER(fp)] * 8
    lib.mmc_trainer_folded_params.restype = i32
    lib.mmc_trainer_folded_params.argtypes = [vp, C.POINTER(fp), C.POINTER(fp)]
    lib.mmc_trainer_norm_stage.restype = i32
    lib.mmc_trainer_norm_stage.argtypes = [vp, i32, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]
    lib.mmc_dist_unique_id.restype = i32
    lib.mmc_dist_unique_id.argtypes = [vp]
    lib.mmc_dist_create.restype = i32
    lib.mmc_dist_create.argtypes = [vp, i32, i32, i32, C.POINTER(vp)]
    lib.mmc_dist_destroy.restype = None
    lib.mmc_dist_destroy.argtypes = [vp]
    lib.mmc_gather_features.restype = i32
    lib.mmc_gather_features.argtypes = [vp, vp, i64, i32, vp, vp, vp]
    lib.mmc_ensemble_create.restype = i32
    lib.mmc_ensemble_create.argtypes = [C.POINTER(vp), i32, C.POINTER(vp)]
    lib.mmc_ensemble_destroy.restype = None
    lib.mmc_ensemble_destroy.argtypes = [vp]
    for name in ("mmc_ensemble_size", "mmc_ensemble_num_classes", "mmc_ensemble_input_dim"):
        getattr(lib, name).restype = i32
        getattr(lib, name).argtypes = [vp]
    lib.mmc_ensemble_chunk_rows.restype = i32
    lib.mmc_ensemble_chunk_rows.argtypes = [vp, i32]
    lib.mmc_ensemble_topk.restype = i32
    lib.mmc_ensemble_topk.argtypes = [vp, vp, i64, i32, i32, vp, vp, vp, vp, vp, u32, vp]
    lib.mmc_ensemble_classify_patches.restype = i32
    lib.mmc_ensemble_classify_patches.argtypes = [vp, vp, vp, i64, i32, i32, vp, vp, vp, vp, u32, vp]
    # the arguments of mmc_head_evaluate(_set) with stats and votes behind p_true
    lib.mmc_ensemble_evaluate.restype = i32
    lib.mmc_ensemble_evaluate.argtypes = [vp, vp, vp, i64, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, vp]
    lib.mmc_ensemble_evaluate_set.restype = i32
    lib.mmc_ensemble_evaluate_set.argtypes = [vp, vp, i64, i64, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mmc_targetset_create.restype = i32
    lib.mmc_targetset_create.argtypes = [i32, i32, i64, C.POINTER(vp)]
    lib.mmc_targetset_destroy.restype = None
    lib.mmc_targetset_destroy.argtypes = [vp]
    lib.mmc_targetset_rows.restype = i64
    lib.mmc_targetset_rows.argtypes = [vp]
    lib.mmc_targetset_num_classes.restype = i32
    lib.mmc_targetset_num_classes.argtypes = [vp]
    lib.mmc_targetset_append.restype = i32
    lib.mmc_targetset_append.argtypes = [vp, vp, i64, u32, vp]
    lib.mmc_targetset_read.restype = i32
    lib.mmc_targetset_read.argtypes = [vp, i64, i64, vp, vp]
    lib.mmc_ensemble_predict_set.restype = i32
    lib.mmc_ensemble_predict_set.argtypes = [vp, vp, i64, i64, vp, vp]
    lib.mmc_trainer_set_distillation.restype = i32
    lib.mmc_trainer_set_distillation.argtypes = [vp, f64, f64]
    # the arguments of the _weighted passes with the target set (one, or `count` pointers) behind the feature set
    lib.mmc_trainer_partial_fit_set_distill.restype = i32
    lib.mmc_trainer_partial_fit_set_distill.argtypes = [vp, vp, vp, vp, vp, vp, i64, i32, C.POINTER(C.c_double), vp]
    lib.mmc_trainer_group_partial_fit_set_distill.restype = i32
    lib.mmc_trainer_group_partial_fit_set_distill.argtypes = [C.POINTER(vp), i32, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                                              C.POINTER(vp), C.POINTER(i64), C.POINTER(i32), C.POINTER(C.c_double), vp]
    lib.mmc_trainer_loss_gradient_distill.restype = i32
    lib.mmc_trainer_loss_gradient_distill.argtypes = [vp, vp, vp, vp, vp, i64, vp, vp, vp]
    # the arguments of mmc_trainer_loss_gradient_weighted with the target rows behind y
    lib.mmc_trainer_loss_gradient_distill_weighted.restype = i32
    lib.mmc_trainer_loss_gradient_distill_weighted.argtypes = [vp, vp, vp, vp, vp, vp, vp, f64, i32, i64, vp, vp, vp, vp, vp]
    return lib


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        _lib = _load()
    return _lib


def check(status: int) -> None:
    """Translate a status code into the Python exception the reference's callers expect
    (ValueError for bad shapes/URIs, RuntimeError for device problems)."""
    if status == MMC_OK:
        return
    msg = lib().mmc_last_error().decode("utf-8", "replace")
    if status in (MMC_ERR_ARG, MMC_ERR_WEIGHTS):
        raise ValueError(msg)
    if status == MMC_ERR_NOMEM:
        raise MemoryError(msg)
    raise RuntimeError(msg)
