"""mermaid_classifier_amd -- MI355X (gfx950) implementation of the PySpacer EfficientNet patch
feature-extraction path of data-mermaid/mermaid-classifier, behind the reference's own
extractor / predictor interfaces.  Importing the package is cheap; the HIP library is loaded on
first use and its absence is an error (there is no CPU fallback)."""

from .extractor import EfficientNetExtractor, build_extractor_class, resolve_device, verify_device_numerics  # noqa: F401
from .inference import ManifestError, Predictor, load_predictor, SCHEMA_VERSION, TASK_NAME  # noqa: F401
from .backbone import ALL_ORIENTATIONS, Backbone, check_views, crop_patches_device, FEATURE_DIM  # noqa: F401
from .classify import PointClassifier, PointPredictions  # noqa: F401
from .calibration import CalibratedMLP, ParityError, calibrate, evaluate, evaluate_classes, export_artifact  # noqa: F401
from .class_scores import ClassScores  # noqa: F401
from .featureset import FeatureSet  # noqa: F401
from .training import epoch_loop, train_and_validate, train_classifier  # noqa: F401
from .sweep import SweepConfig, partial_fit_rows_group, rank_sweep, sweep_loop, train_sweep  # noqa: F401
from .sampling import class_counts, effective_number_weights, group_balance_weights, logit_adjustment, mixup_plan, row_batches, subsample_rows, subsample_targets  # noqa: F401
from .validation import Validation, previous_accuracies, validate  # noqa: F401
from .metrics import CoverStats, GroupedValidation, Reliability, SourceStats, category_bins, grouped_validate  # noqa: F401
from .taxonomy import TaxonomicScores, hierarchy_levels, soft_labels  # noqa: F401
from .ranking import RankedValidation, ranking_validate, similarity_levels  # noqa: F401
from .cover import CoverEstimate, estimate_cover, prior_from_labels  # noqa: F401
from .feature_transform import FeatureTransform  # noqa: F401
from .logit_scaling import LogitScaling, fit_logit_scaling  # noqa: F401
from .optim import fold_batch_norm  # noqa: F401
from .neighbors import KnnValidation, Neighbors, audit_labels, knn_validate, near_duplicates, nearest  # noqa: F401
from .ensemble import EnsembleValidation, HeadEnsemble, Uncertainty, ensemble_validate, export_ensemble, load_ensemble  # noqa: F401
from .distill import TargetSet, distill, teacher_targets  # noqa: F401

__all__ = [
    "EfficientNetExtractor", "build_extractor_class", "resolve_device", "verify_device_numerics",
    "ManifestError", "Predictor", "load_predictor", "SCHEMA_VERSION", "TASK_NAME",
    "Backbone", "crop_patches_device", "FEATURE_DIM", "check_views", "ALL_ORIENTATIONS",
    "PointClassifier", "PointPredictions",
    "CalibratedMLP", "ParityError", "calibrate", "evaluate", "export_artifact",
    "FeatureSet", "epoch_loop", "train_classifier", "train_and_validate",
    "SweepConfig", "partial_fit_rows_group", "sweep_loop", "train_sweep", "rank_sweep",
    "evaluate_classes", "ClassScores",
    "class_counts", "effective_number_weights", "logit_adjustment", "subsample_targets", "subsample_rows", "row_batches", "mixup_plan", "group_balance_weights",
    "Validation", "validate", "previous_accuracies",
    "grouped_validate", "GroupedValidation", "CoverStats", "SourceStats", "Reliability",
    "ranking_validate", "RankedValidation", "similarity_levels",
    "category_bins", "TaxonomicScores", "hierarchy_levels", "soft_labels",
    "estimate_cover", "CoverEstimate", "prior_from_labels",
    "FeatureTransform",
    "LogitScaling", "fit_logit_scaling", "fold_batch_norm",
    "nearest", "Neighbors", "knn_validate", "KnnValidation", "audit_labels", "near_duplicates",
    "HeadEnsemble", "Uncertainty", "ensemble_validate", "EnsembleValidation", "export_ensemble", "load_ensemble",
    "TargetSet", "teacher_targets", "distill",
]
