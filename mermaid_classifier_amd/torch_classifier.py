"""TorchMLPClassifier with the training arithmetic on the MI355X.

Host-side mirror of reference ``mermaid_classifier/pyspacer/torch_classifier.py`` (class ``TorchMLPClassifier``,
the sklearn-``MLPClassifier`` subset the trainer drives through ``partial_fit``,
``mermaid_classifier/pyspacer/trainer.py:118-145``): same constructor arguments, same ``partial_fit`` / ``fit`` /
``predict`` / ``predict_proba`` / ``classes_`` / ``loss_curve_`` / ``n_iter_`` / ``get_params`` / ``set_params`` /
pickling behaviour and the same errors.  What stays on the host is what the reference keeps in numpy / Python: label
lookup, the shuffle order (numpy ``default_rng(random_state)``, :139-157), Glorot initialisation (torch's CPU generator
under ``torch.manual_seed(random_state)``, so equal seeds give equal initial weights, :176-184), softmax + float64
renormalisation of ``_forward_probs`` (:332-376).  Forward, weighted cross-entropy, L2 term, backward and Adam run in
``libmermaid_mi355.so`` (``mmc_trainer_*``, csrc/trainer.hip).  No CPU fallback.

Taken as they are from the reference (the sklearn-protocol shell a drop-in has to reproduce; argument checks, defaults
and error strings included): ``__init__`` (:95-136, the argument validation and attribute names), ``_resolve_batch_size``
(:138-141), ``_seed_rng`` (:143-157), ``_labels_to_indices`` (:159-173), ``_build_class_weight_vector`` (the reference's
``_build_class_weight_tensor``, :192-214, minus the tensor construction), ``get_params`` / ``set_params`` (:380-408) and the input checks at the top of ``partial_fit`` /
``_forward_probs``.  Written here, with no counterpart there: ``_initial_parameters`` (host Glorot draw handed to the
device), ``_create_trainer``, the device half of ``partial_fit`` (``mmc_trainer_partial_fit_ordered``), ``_forward_probs``'s
logits call (``mmc_trainer_logits``), ``parameters`` / ``_module`` / ``_adam_state`` (state read back through the C ABI),
``__getstate__`` / ``__setstate__`` (the pickle carries host copies of weights and Adam moments), ``_release``,
``partial_fit_rows`` (``partial_fit`` over rows of a device-resident ``FeatureSet``: ``mmc_trainer_partial_fit_set``) and its
two halves ``_begin_rows_pass`` / ``_end_pass``, which ``sweep.partial_fit_rows_group`` puts around one grouped call; and the loss
formulation -- ``label_smoothing`` / ``focal_gamma`` / ``logit_prior``, ``_check_loss_scalars``, ``_build_logit_prior_vector``
(``mmc_trainer_set_loss``) -- whose defaults are the reference's weighted cross-entropy; and the regularisers -- ``dropout`` /
``input_dropout`` / ``mixup_alpha`` / ``regularizer_seed``, ``_check_regularizers``, ``_regularizer_seed_value``, ``_mix_plan``
(``mmc_trainer_set_dropout``, ``mmc_trainer_partial_fit_set_mixed``) -- whose defaults leave the step as it is; and the optimiser
options -- ``lr_schedule`` / ``warmup_steps`` / ``schedule_steps`` / ``final_lr_ratio`` / ``max_grad_norm`` / ``ema_decay``,
``_apply_optimizer_options``, ``raw_parameters`` / ``averaged_parameters`` / ``use_weights``, ``grad_norms_``
(``mmc_trainer_set_lr_schedule``, ``mmc_trainer_set_grad_clip``, ``mmc_trainer_set_ema``) -- again off by default; and the
taxonomy-aware loss -- ``class_levels`` / ``level_weights`` / ``soft_targets``, ``_build_hierarchy_arrays``
(``mmc_trainer_set_hierarchy``) -- off by default too; and batch normalisation -- ``batch_norm`` / ``batch_norm_eps`` /
``batch_norm_momentum``, ``batch_norm_state`` (``mmc_trainer_set_batch_norm``, ``mmc_trainer_folded_params``) -- off by default as well.
"""

from __future__ import annotations

import ctypes as C
import warnings
from collections.abc import Sequence
from typing import Any, List

import numpy as np

from . import _lib
from .optim import LR_KINDS, check_batch_norm, check_optimizer_options
from .backbone import _current_stream_ptr, _device_index

_EXPECTED_FP_DRIFT_TOL = 1e-4   # torch_classifier.py:45-50


def _ptr_array(arrays: List[np.ndarray]):
    fp = C.POINTER(C.c_float)
    return (fp * len(arrays))(*[a.ctypes.data_as(fp) for a in arrays])


def _check_loss_scalars(label_smoothing, focal_gamma) -> None:
    """The ranges ``mmc_trainer_set_loss`` accepts (include/mmc.h)."""
    if isinstance(label_smoothing, bool) or not isinstance(label_smoothing, (int, float, np.integer, np.floating)) \
            or not 0.0 <= float(label_smoothing) < 1.0:
        raise ValueError(f"label_smoothing must lie in [0, 1), got {label_smoothing!r}.")
    if isinstance(focal_gamma, bool) or not isinstance(focal_gamma, (int, float, np.integer, np.floating)) \
            or not (float(focal_gamma) == 0.0 or 1.0 <= float(focal_gamma) <= 8.0):
        raise ValueError(f"focal_gamma must be 0 or lie in [1, 8], got {focal_gamma!r}.")


def _check_regularizers(dropout, input_dropout, mixup_alpha, regularizer_seed) -> None:
    """The ranges ``mmc_trainer_set_dropout`` accepts (include/mmc.h), a non-negative finite ``mixup_alpha`` and a seed of 64 bits."""
    for name, p in (("dropout", dropout), ("input_dropout", input_dropout)):
        if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)) or not 0.0 <= float(p) <= 0.9:
            raise ValueError(f"{name} must lie in [0, 0.9], got {p!r}.")
    if isinstance(mixup_alpha, bool) or not isinstance(mixup_alpha, (int, float, np.integer, np.floating)) \
            or not (0.0 <= float(mixup_alpha) and np.isfinite(float(mixup_alpha))):
        raise ValueError(f"mixup_alpha must be a finite number >= 0, got {mixup_alpha!r}.")
    if regularizer_seed is not None and (isinstance(regularizer_seed, bool) or not isinstance(regularizer_seed, (int, np.integer))
                                         or not 0 <= int(regularizer_seed) < 2 ** 64):
        raise ValueError(f"regularizer_seed must be None or an integer in [0, 2**64), got {regularizer_seed!r}.")


def _check_group_dro(group_dro_eta, n_groups) -> None:
    """The ranges ``mmc_trainer_set_group_dro`` accepts (include/mmc.h): ``n_groups`` None or in [1, 1024], ``group_dro_eta`` in [0, 10]."""
    if isinstance(group_dro_eta, bool) or not isinstance(group_dro_eta, (int, float, np.integer, np.floating)) \
            or not 0.0 <= float(group_dro_eta) <= 10.0:
        raise ValueError(f"group_dro_eta must lie in [0, 10], got {group_dro_eta!r}.")
    if n_groups is not None and (isinstance(n_groups, bool) or not isinstance(n_groups, (int, np.integer))
                                 or not 1 <= int(n_groups) <= _lib.MMC_DRO_MAX_GROUPS):
        raise ValueError(f"n_groups must be None or an integer in [1, {_lib.MMC_DRO_MAX_GROUPS}], got {n_groups!r}.")


def check_distillation(distill_alpha, distill_temperature) -> None:
    """``distill_alpha`` in [0, 1] and ``distill_temperature`` in [0.25, 64] (include/mmc.h, "distillation"); ``ValueError``."""
    for name, v, lo, hi in (("distill_alpha", distill_alpha, 0.0, 1.0), ("distill_temperature", distill_temperature, 0.25, 64.0)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not lo <= float(v) <= hi:
            raise ValueError(f"{name} must be a number in [{lo:g}, {hi:g}]; got {v!r}")


def check_targets(clf, fs, targets):
    """``targets`` of a pass of ``clf`` over ``fs``: a ``TargetSet`` with one row per row of the set and the set's classes, on a
    classifier with ``distill_alpha > 0`` and no hierarchy or mixup.  ``ValueError`` before anything reaches the library."""
    if targets is None:
        return None
    from .distill import TargetSet
    if not isinstance(targets, TargetSet):
        raise ValueError(f"targets must be a TargetSet, got {type(targets).__name__}")
    if float(getattr(clf, "distill_alpha", 0.0)) == 0.0:
        raise ValueError("targets need a classifier with distill_alpha > 0.")
    if float(getattr(clf, "mixup_alpha", 0.0)) != 0.0:
        raise ValueError("mixup_alpha > 0 cannot be combined with targets.")
    if any(getattr(clf, k, None) is not None for k in ("class_levels", "soft_targets")):
        raise ValueError("targets cannot be combined with class_levels / soft_targets (the taxonomy-aware loss).")
    if len(targets) != len(fs):
        raise ValueError(f"targets hold {len(targets)} rows, the feature set {len(fs)}")
    if not np.array_equal(np.asarray(targets.classes), np.asarray(fs.classes)):
        raise ValueError("the targets' classes differ from the feature set's")
    return targets


def check_row_arrays(clf, n_rows: int, row_weight, row_group):
    """``row_weight`` / ``row_group`` of a pass of ``clf`` over a set of ``n_rows`` rows, indexed by row of the set -> them as
    contiguous float32 / int32 (or None).  ``ValueError``, before any device work: not 1D with ``n_rows`` entries, a dtype that is
    not real (weights) or integer (groups), a weight that is negative or not finite, a group outside ``[0, n_groups)``, ``row_group``
    on a classifier without ``n_groups``, either array on a classifier with ``mixup_alpha > 0``."""
    if row_weight is None and row_group is None:
        return None, None
    if float(getattr(clf, "mixup_alpha", 0.0)) != 0.0:
        raise ValueError("mixup_alpha > 0 cannot be combined with row_weight / row_group.")
    rw = rg = None
    if row_weight is not None:
        arr = np.asarray(row_weight)
        if arr.ndim != 1 or arr.shape[0] != n_rows:
            raise ValueError(f"row_weight must have one entry per row of the set ({n_rows}), got shape {arr.shape}")
        if arr.dtype == np.bool_ or not (np.issubdtype(arr.dtype, np.floating) or np.issubdtype(arr.dtype, np.integer)):
            raise ValueError(f"row_weight must be a real-valued array, got dtype {arr.dtype}")
        with np.errstate(over="ignore"):
            rw = np.ascontiguousarray(arr, dtype=np.float32)
        if not (np.isfinite(rw).all() and (rw >= 0).all()):
            raise ValueError("row_weight holds a weight that is negative or not finite (as float32).")
    if row_group is not None:
        n_groups = getattr(clf, "n_groups", None)
        if n_groups is None:
            raise ValueError("row_group needs a classifier with n_groups set.")
        arr = np.asarray(row_group)
        if arr.ndim != 1 or arr.shape[0] != n_rows:
            raise ValueError(f"row_group must have one entry per row of the set ({n_rows}), got shape {arr.shape}")
        if arr.dtype == np.bool_ or not np.issubdtype(arr.dtype, np.integer):
            raise ValueError(f"row_group must be an integer array, got dtype {arr.dtype}")
        if arr.size and (int(arr.min()) < 0 or int(arr.max()) >= int(n_groups)):
            raise ValueError(f"row_group holds a group outside [0, {int(n_groups)}).")
        rg = np.ascontiguousarray(arr, dtype=np.int32)
    return rw, rg


def by_position(arr, visit, n_samples: int):
    """An array indexed by row of the set -> indexed by position of the pass that visits ``visit`` (None: rows 0..n-1 in order)."""
    if arr is None:
        return None
    return np.ascontiguousarray(arr[:n_samples] if visit is None else arr[visit])


class TorchMLPClassifier:
    """See the module docstring; argument meaning as in the reference (torch_classifier.py:93-135).  Three arguments have no
    counterpart there, the loss formulation of ``mmc_trainer_set_loss`` (include/mmc.h): ``label_smoothing`` in [0, 1) with
    ``F.cross_entropy(label_smoothing=)``'s meaning, ``focal_gamma`` (0, or in [1, 8]: focal loss) and ``logit_prior``, a dict from
    label to a finite offset added to the logits inside the loss only (``sampling.logit_adjustment``); like ``class_weight`` it is
    resolved in ``classes_`` order at the first fit.  Training alone reads them: ``predict_proba``, evaluation, calibration and
    export see the raw logits.  The defaults train with the plain loss, bit for bit.

    Four more, keyword only, are the regularisers of include/mmc.h: ``dropout`` on the hidden activations and ``input_dropout`` on the
    feature rows (each in [0, 0.9]; ``mmc_trainer_set_dropout``, on every training path), ``mixup_alpha`` > 0 mixes every row of a
    ``partial_fit_rows`` pass with a partner of its mini-batch, ``lam ~ Beta(alpha, alpha)`` per mini-batch (``sampling.mixup_plan``;
    the host-fed ``partial_fit`` raises), and ``regularizer_seed`` seeds both (None: ``random_state``, or one draw from numpy's global
    RNG when that is None too).  Read when the trainer is created, like every other hyper-parameter.  Training alone sees them; the
    defaults leave every pass as it is, bit for bit.

    Six more, keyword only, are the optimiser options of include/mmc.h: ``lr_schedule`` ("constant" / "linear" / "cosine") with
    ``warmup_steps``, ``schedule_steps`` (the step at which the decay ends; a decaying schedule needs it by the first fit --
    ``train_classifier`` and ``train_sweep`` fill a None in) and ``final_lr_ratio`` in [0, 1]; ``max_grad_norm`` (None: off) clips the
    global gradient norm of every step, and ``grad_norms_`` then holds the last pass's pre-clip norms; ``ema_decay`` in (0, 1) keeps
    an exponential average of the weights.  With ``ema_decay > 0`` the classifier evaluates the AVERAGED weights: ``predict_proba``,
    ``parameters()`` and everything built on them (``calibration.evaluate`` / ``calibrate`` / ``export_artifact``,
    ``fit_logit_scaling``, early stopping's validation loss) see them, training goes on with the raw ones, ``raw_parameters()``
    returns those, and ``use_weights("raw")`` / ``use_weights("averaged")`` switches.  Everything with the defaults is as before.

    Two more, keyword only, are group DRO (include/mmc.h, "group-robust training"): ``n_groups`` (None: off; else in [1, 1024]) and
    ``group_dro_eta`` in [0, 10], the step of the groups' distribution q (0: a static group-balanced loss).  They act on the
    ``partial_fit_rows`` passes that are given ``row_group``; ``group_weights_`` holds q after such a pass and is pickled (as log q),
    so that a resumed classifier continues from it.  ``partial_fit_rows(row_weight=)`` needs neither.

    Three more, keyword only, are the taxonomy-aware loss (include/mmc.h, "taxonomy-aware loss"), keyed by label like ``class_weight``:
    ``class_levels``, a dict from label to a sequence of L <= 4 ints, the class's node at every level (None or a negative int: no
    node); ``level_weights``, L floats >= 0; ``soft_targets``, a dict from label to ``{label: mass}`` (a missing entry is 0; every row
    sums to 1), which replaces the one-hot base term and cannot be combined with ``label_smoothing`` / ``focal_gamma``.
    ``taxonomy.hierarchy_levels`` and ``taxonomy.soft_labels`` make the arrays.  Resolved in ``classes_`` order when the trainer is
    created; training alone reads them, and ``mixup_alpha > 0`` cannot be combined with them.

    Three more, keyword only, are batch normalisation (include/mmc.h, "batch normalisation"): ``batch_norm=True`` puts
    ``BatchNorm1d(eps=batch_norm_eps, momentum=batch_norm_momentum)`` between every hidden ``Linear`` and its ``ReLU`` while training.
    Evaluation reads the stack with the running statistics folded in: ``predict_proba``, ``parameters()`` and everything built on them
    (``_module``, ``calibration.evaluate`` / ``calibrate`` / ``export_artifact``, early stopping) see a plain ``Linear -> ReLU`` head;
    ``raw_parameters()`` returns the training weights and ``batch_norm_state()`` gamma, beta and the running statistics.  It cannot be
    combined with ``dropout > 0`` or ``ema_decay > 0`` (``input_dropout`` composes), and every mini-batch needs at least 2 rows."""

    _estimator_type = "classifier"

    def __init__(self, hidden_layer_sizes: Sequence[int] = (100,), activation: str = "relu", solver: str = "adam",
                 alpha: float = 0.0001, batch_size: int | str = "auto", learning_rate_init: float = 0.001,
                 max_iter: int = 200, shuffle: bool = True, random_state: int | None = None, tol: float = 1e-4,
                 beta_1: float = 0.9, beta_2: float = 0.999, epsilon: float = 1e-8,
                 class_weight: dict | None = None, device=0, *, label_smoothing: float = 0.0, focal_gamma: float = 0.0,
                 logit_prior: dict | None = None, dropout: float = 0.0, input_dropout: float = 0.0, mixup_alpha: float = 0.0,
                 regularizer_seed: int | None = None, lr_schedule: str = "constant", warmup_steps: int = 0,
                 schedule_steps: int | None = None, final_lr_ratio: float = 0.0, max_grad_norm: float | None = None,
                 ema_decay: float = 0.0, group_dro_eta: float = 0.0, n_groups: int | None = None,
                 class_levels: dict | None = None, level_weights: Sequence[float] | None = None, soft_targets: dict | None = None,
                 batch_norm: bool = False, batch_norm_eps: float = 1e-5, batch_norm_momentum: float = 0.1,
                 distill_alpha: float = 0.0, distill_temperature: float = 1.0):
        if activation != "relu":
            raise ValueError(f"TorchMLPClassifier only supports activation='relu', got {activation!r}.")
        if solver != "adam":
            raise ValueError(f"TorchMLPClassifier only supports solver='adam', got {solver!r}.")
        _check_loss_scalars(label_smoothing, focal_gamma)
        _check_regularizers(dropout, input_dropout, mixup_alpha, regularizer_seed)
        check_optimizer_options(lr_schedule, warmup_steps, schedule_steps, final_lr_ratio, max_grad_norm, ema_decay)
        _check_group_dro(group_dro_eta, n_groups)
        check_batch_norm(batch_norm, batch_norm_eps, batch_norm_momentum)
        check_distillation(distill_alpha, distill_temperature)
        self.hidden_layer_sizes = tuple(hidden_layer_sizes)
        self.activation = activation
        self.solver = solver
        self.alpha = alpha
        self.batch_size = batch_size
        self.learning_rate_init = learning_rate_init
        self.max_iter = max_iter
        self.shuffle = shuffle
        self.random_state = random_state
        self.tol = tol
        self.beta_1 = beta_1
        self.beta_2 = beta_2
        self.epsilon = epsilon
        self.class_weight = class_weight
        self.device = device
        self.label_smoothing = label_smoothing
        self.focal_gamma = focal_gamma
        self.logit_prior = logit_prior
        self.dropout = dropout
        self.input_dropout = input_dropout
        self.mixup_alpha = mixup_alpha
        self.regularizer_seed = regularizer_seed
        self.lr_schedule = lr_schedule
        self.warmup_steps = warmup_steps
        self.schedule_steps = schedule_steps
        self.final_lr_ratio = final_lr_ratio
        self.max_grad_norm = max_grad_norm
        self.ema_decay = ema_decay
        self.group_dro_eta = group_dro_eta
        self.n_groups = n_groups
        self.class_levels = class_levels
        self.level_weights = level_weights
        self.soft_targets = soft_targets
        self.batch_norm = batch_norm
        self.batch_norm_eps = batch_norm_eps
        self.batch_norm_momentum = batch_norm_momentum
        self.distill_alpha = distill_alpha
        self.distill_temperature = distill_temperature

    # ---- host bookkeeping, restated from the reference ------------------------------------------------------------
    def _resolve_batch_size(self, n_samples: int) -> int:
        if self.batch_size == "auto":
            return min(200, n_samples)
        return min(int(self.batch_size), n_samples)

    def _seed_rng(self) -> np.random.Generator:
        if self.random_state is not None:
            return np.random.default_rng(int(self.random_state))
        if not hasattr(self, "_none_rng"):
            self._none_rng = np.random.default_rng(np.random.randint(0, np.iinfo(np.int32).max))
        return self._none_rng

    def _labels_to_indices(self, y: np.ndarray) -> np.ndarray:
        y = np.asarray(y)
        idx = np.searchsorted(self.classes_, y)
        missing = idx >= len(self.classes_)
        if missing.any() or not np.array_equal(self.classes_[np.minimum(idx, len(self.classes_) - 1)], y):
            bad = set(np.asarray(y).tolist()) - set(self.classes_.tolist())
            raise ValueError(f"Labels {sorted(bad)} are not in classes_ {self.classes_.tolist()}."
                             f" Pass all classes to the first partial_fit call.")
        return idx

    def _build_class_weight_vector(self):
        if self.class_weight is None:
            return None
        weights = []
        for cls in self.classes_:
            if cls not in self.class_weight:
                bad = sorted(set(self.classes_.tolist()) - set(self.class_weight))
                raise ValueError(f"class_weight is missing weights for {bad!r}. Pass weights for every class in classes_.")
            w = float(self.class_weight[cls])
            if w < 0:
                raise ValueError(f"class_weight for {cls!r} is negative ({w!r}); weights must be >= 0.")
            weights.append(w)
        return np.asarray(weights, dtype=np.float32)

    def _build_logit_prior_vector(self):
        """``logit_prior`` in ``classes_`` order as float32, or None."""
        prior = getattr(self, "logit_prior", None)
        if prior is None:
            return None
        missing = [cls for cls in self.classes_.tolist() if cls not in prior]
        if missing:
            raise ValueError(f"logit_prior is missing offsets for {sorted(missing)!r}. Pass an offset for every class in classes_.")
        with np.errstate(over="ignore"):   # an offset beyond float32 becomes inf and is reported below
            vec = np.asarray([float(prior[cls]) for cls in self.classes_.tolist()], dtype=np.float64).astype(np.float32)
        if not np.isfinite(vec).all():
            bad = [cls for cls, v in zip(self.classes_.tolist(), vec) if not np.isfinite(v)]
            raise ValueError(f"logit_prior for {bad!r} is not finite.")
        return vec

    def _build_hierarchy_arrays(self):
        """``class_levels`` / ``level_weights`` / ``soft_targets`` in ``classes_`` order -> ``(levels [L][K] int32, weights [L] float64,
        T [K][K] float32)``, each None where not given; None when nothing is given.  What ``mmc_trainer_set_hierarchy`` takes."""
        levels_of = getattr(self, "class_levels", None)
        weights = getattr(self, "level_weights", None)
        soft = getattr(self, "soft_targets", None)
        if levels_of is None and weights is None and soft is None:
            return None
        classes = self.classes_.tolist()
        levels = lam = T = None
        if (levels_of is None) != (weights is None):
            raise ValueError("class_levels and level_weights go together: only "
                             f"{'class_levels' if weights is None else 'level_weights'} was given.")
        if levels_of is not None:
            missing = [cls for cls in classes if cls not in levels_of]
            if missing:
                raise ValueError(f"class_levels is missing nodes for {sorted(missing)!r}. Pass the nodes of every class in classes_.")
            lam = np.asarray([float(v) for v in weights], dtype=np.float64)
            n_levels = len(lam)
            if not 1 <= n_levels <= _lib.MMC_HIER_MAX_LEVELS:
                raise ValueError(f"level_weights must hold 1 to {_lib.MMC_HIER_MAX_LEVELS} weights, got {n_levels}.")
            if not (np.isfinite(lam).all() and (lam >= 0).all()):
                raise ValueError(f"level_weights must be finite and >= 0, got {lam.tolist()!r}.")
            levels = np.empty((n_levels, len(classes)), np.int32)
            for c, cls in enumerate(classes):
                nodes = list(levels_of[cls])
                if len(nodes) != n_levels:
                    raise ValueError(f"class_levels for {cls!r} has {len(nodes)} entries, level_weights {n_levels}.")
                levels[:, c] = [-1 if v is None or int(v) < 0 else int(v) for v in nodes]
        if soft is not None:
            missing = [cls for cls in classes if cls not in soft]
            if missing:
                raise ValueError(f"soft_targets is missing rows for {sorted(missing)!r}. Pass a row for every class in classes_.")
            index = {cls: c for c, cls in enumerate(classes)}
            T = np.zeros((len(classes), len(classes)), np.float32)
            for cls in classes:
                for other, mass in soft[cls].items():
                    if other not in index:
                        raise ValueError(f"soft_targets for {cls!r} names {other!r}, which is not in classes_.")
                    T[index[cls], index[other]] = float(mass)
            if not (np.isfinite(T).all() and (T >= 0).all()):
                raise ValueError("soft_targets holds a mass that is negative or not finite (as float32).")
            off = np.abs(T.astype(np.float64).sum(axis=1) - 1.0)
            if off.max() > 1e-5:
                raise ValueError(f"soft_targets for {classes[int(off.argmax())]!r} sums to {1.0 + off.max():.7g} off 1 by more than 1e-5.")
        if float(getattr(self, "mixup_alpha", 0.0)) != 0.0:
            raise ValueError("mixup_alpha > 0 cannot be combined with class_levels / soft_targets.")
        return levels, lam, T

    def _initial_parameters(self):
        """Glorot-uniform weights / zero biases drawn exactly as the reference's ``_MLPModule`` draws them
        (torch_classifier.py:53-76, 176-184): the Linear layers are constructed first (their default init consumes the
        generator), then re-initialised in order."""
        import torch
        import torch.nn as nn
        if self.random_state is not None:
            torch.manual_seed(int(self.random_state))
        sizes = [self.n_features_in_, *self.hidden_layer_sizes, len(self.classes_)]
        layers = [nn.Linear(i, o) for i, o in zip(sizes[:-1], sizes[1:])]
        for m in layers:
            nn.init.xavier_uniform_(m.weight)
            nn.init.zeros_(m.bias)
        return ([np.ascontiguousarray(m.weight.detach().numpy(), dtype=np.float32) for m in layers],
                [np.ascontiguousarray(m.bias.detach().numpy(), dtype=np.float32) for m in layers])

    def _create_trainer(self, weights, biases) -> None:
        lib = _lib.lib()
        self._dims = [int(weights[0].shape[1])] + [int(w.shape[0]) for w in weights]
        dims = (C.c_int * len(self._dims))(*self._dims)
        cw = self._class_weight_vector
        self._h = C.c_void_p()
        _lib.check(lib.mmc_trainer_create(_ptr_array(weights), _ptr_array(biases), dims, len(weights),
                                          float(self.learning_rate_init), float(self.beta_1), float(self.beta_2),
                                          float(self.epsilon), float(self.alpha),
                                          cw.ctypes.data_as(C.POINTER(C.c_float)) if cw is not None else None,
                                          _device_index(self.device), C.byref(self._h)))
        # the loss options are read here, like every other hyper-parameter; all defaults select the plain loss
        prior = getattr(self, "_logit_prior_vector", None)
        try:
            _lib.check(lib.mmc_trainer_set_loss(self._h, float(self.label_smoothing), float(self.focal_gamma),
                                                prior.ctypes.data_as(C.POINTER(C.c_float)) if prior is not None else None))
            hier = getattr(self, "_hierarchy_arrays", None)
            if hier is not None:
                levels, lam, T = hier
                _lib.check(lib.mmc_trainer_set_hierarchy(self._h, 0 if levels is None else len(lam),
                                                         None if levels is None else levels.ctypes.data,
                                                         None if levels is None else lam.ctypes.data,
                                                         None if T is None else T.ctypes.data))
            if float(self.dropout) != 0.0 or float(self.input_dropout) != 0.0:
                _lib.check(lib.mmc_trainer_set_dropout(self._h, float(self.input_dropout), float(self.dropout),
                                                       self._regularizer_seed_value()))
            self._apply_optimizer_options()
            if self._normalises():   # after dropout and the averaged weights: the second setter refuses the combination
                check_batch_norm(self.batch_norm, self.batch_norm_eps, self.batch_norm_momentum)
                _lib.check(lib.mmc_trainer_set_batch_norm(self._h, 1, float(self.batch_norm_eps), float(self.batch_norm_momentum)))
            if getattr(self, "n_groups", None) is not None:
                _check_group_dro(self.group_dro_eta, self.n_groups)
                _lib.check(lib.mmc_trainer_set_group_dro(self._h, int(self.n_groups), float(self.group_dro_eta)))
            self._apply_distillation()
        except Exception:
            self._release()
            raise

    def _apply_optimizer_options(self) -> None:
        """The optimiser options onto the trainer just created; a default makes no call.  The shadow of the averaged weights starts
        as the parameters the trainer was created with, and a classifier that averages evaluates the average."""
        lib = _lib.lib()
        check_optimizer_options(self.lr_schedule, self.warmup_steps, self.schedule_steps, self.final_lr_ratio, self.max_grad_norm,
                                self.ema_decay)
        if self.lr_schedule != "constant" or int(self.warmup_steps) != 0:
            if self.lr_schedule != "constant" and self.schedule_steps is None:
                raise ValueError(f"lr_schedule={self.lr_schedule!r} needs schedule_steps, the step at which the decay ends "
                                 f"(train_classifier / train_sweep fill it with nbr_epochs x the steps of an epoch).")
            _lib.check(lib.mmc_trainer_set_lr_schedule(self._h, LR_KINDS[self.lr_schedule], int(self.warmup_steps),
                                                       int(self.schedule_steps or 0), float(self.final_lr_ratio)))
        if self.max_grad_norm is not None:
            _lib.check(lib.mmc_trainer_set_grad_clip(self._h, float(self.max_grad_norm)))
        if float(self.ema_decay) != 0.0:
            _lib.check(lib.mmc_trainer_set_ema(self._h, float(self.ema_decay)))
            if getattr(self, "_eval_weights", "averaged") == "averaged":
                _lib.check(lib.mmc_trainer_eval_weights(self._h, _lib.MMC_WEIGHTS_AVERAGED))

    def _apply_distillation(self) -> None:
        """The distillation options onto the trainer just created; the default makes no call."""
        alpha = getattr(self, "distill_alpha", 0.0)
        check_distillation(alpha, getattr(self, "distill_temperature", 1.0))
        if float(alpha) != 0.0:
            _lib.check(_lib.lib().mmc_trainer_set_distillation(self._h, float(alpha), float(self.distill_temperature)))

    def _averages(self) -> bool:
        return float(getattr(self, "ema_decay", 0.0)) != 0.0

    def _normalises(self) -> bool:
        return bool(getattr(self, "batch_norm", False))

    def use_weights(self, which: str) -> "TorchMLPClassifier":
        """What evaluation reads from now on: "raw", the training weights, or "averaged" (``ema_decay > 0`` only; its default)."""
        if which not in ("raw", "averaged"):
            raise ValueError(f"which must be 'raw' or 'averaged', got {which!r}.")
        if which == "averaged" and not self._averages():
            raise ValueError("this classifier keeps no averaged weights (ema_decay is 0).")
        self._eval_weights = which
        if self._fitted():
            _lib.check(_lib.lib().mmc_trainer_eval_weights(self._h, _lib.MMC_WEIGHTS_AVERAGED if which == "averaged"
                                                           else _lib.MMC_WEIGHTS_RAW))
        return self

    def _read_grad_norms(self) -> None:
        """``grad_norms_``: the pre-clip gradient norm of every step of the pass just made (clipping on only)."""
        if getattr(self, "max_grad_norm", None) is None:
            return
        lib, steps = _lib.lib(), C.c_int(0)
        _lib.check(lib.mmc_trainer_grad_norms(self._h, None, 0, C.byref(steps)))
        out = np.empty(steps.value, np.float32)
        if steps.value:
            _lib.check(lib.mmc_trainer_grad_norms(self._h, out.ctypes.data, steps.value, C.byref(steps)))
        self.grad_norms_ = out

    def _read_group_weights(self) -> None:
        """``group_weights_``: q of the groups after the pass just made (``n_groups`` set only); ``_group_logq`` is what is pickled."""
        if getattr(self, "n_groups", None) is None:
            return
        logq = np.empty(int(self.n_groups), np.float64)
        _lib.check(_lib.lib().mmc_trainer_group_dro_state(self._h, 0, logq.ctypes.data))
        self._group_logq = logq
        self.group_weights_ = np.exp(logq)

    def _regularizer_seed_value(self) -> int:
        """The seed of the dropout masks and the mixing plans: ``regularizer_seed``, else ``random_state``, else one draw from numpy's
        global RNG, kept (and pickled) so that a classifier keeps one mask sequence for its lifetime."""
        if self.regularizer_seed is not None:
            return int(self.regularizer_seed)
        if self.random_state is not None:
            return int(self.random_state) % 2 ** 64
        if getattr(self, "_regularizer_seed_drawn", None) is None:
            self._regularizer_seed_drawn = int(np.random.randint(0, np.iinfo(np.int32).max))
        return self._regularizer_seed_drawn

    def _mix_plan(self, visit, n_samples: int, batch_size: int):
        """The mixing plan of the pass ``_begin_rows_pass`` has just begun -> ``(visit, partner, lam)``, partner and lam None without
        mixup.  The plan's generator is ``default_rng([seed, n_iter_])``: epochs differ even with a fixed ``random_state``."""
        if float(self.mixup_alpha) == 0.0:
            return visit, None, None
        from .sampling import mixup_plan
        if visit is None:
            visit = np.arange(n_samples, dtype=np.int64)
        rng = np.random.default_rng([self._regularizer_seed_value(), int(self.n_iter_)])
        partner, lam = mixup_plan(visit, batch_size, float(self.mixup_alpha), rng)
        return visit, partner, lam

    def _fitted(self) -> bool:
        return getattr(self, "_h", None) is not None and bool(self._h.value)

    # ---- training ------------------------------------------------------------------------------------------------
    def partial_fit(self, X, y, classes: Sequence[Any] | None = None) -> "TorchMLPClassifier":
        if float(getattr(self, "mixup_alpha", 0.0)) != 0.0:
            raise ValueError("mixup_alpha > 0 mixes rows of a resident FeatureSet: train with partial_fit_rows, not partial_fit.")
        X_arr = np.asarray(X, dtype=np.float32)
        if X_arr.ndim != 2:
            raise ValueError(f"X must be 2D, got shape {X_arr.shape}")
        if not self._fitted():
            self.classes_ = np.unique(np.asarray(y)) if classes is None else np.unique(np.asarray(classes))
            self.n_features_in_ = int(X_arr.shape[1])
            self.n_iter_ = 0
            self.loss_curve_ = []
            self._class_weight_vector = self._build_class_weight_vector()
            self._logit_prior_vector = self._build_logit_prior_vector()
            self._hierarchy_arrays = self._build_hierarchy_arrays()
            self._create_trainer(*self._initial_parameters())
        elif X_arr.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {X_arr.shape[1]} features, expected {self.n_features_in_}")
        y_indices = self._labels_to_indices(np.asarray(y))
        n_samples = X_arr.shape[0]
        batch_size = self._resolve_batch_size(n_samples)
        rng = self._seed_rng()
        order = np.arange(n_samples)
        if self.shuffle:
            rng.shuffle(order)
        avg = C.c_double(0.0)
        di = _device_index(self.device)
        if X_arr.shape[1] % 4 == 0:
            # the visiting order is applied on the device (a gather kernel): no host-side copy of the shuffled matrix
            Xn = np.ascontiguousarray(X_arr)
            yn = np.ascontiguousarray(y_indices.astype(np.int32))
            od = np.ascontiguousarray(order.astype(np.int64))
            _lib.check(_lib.lib().mmc_trainer_partial_fit_ordered(self._h, Xn.ctypes.data, yn.ctypes.data, od.ctypes.data, n_samples,
                                                                  int(batch_size), C.byref(avg), _current_stream_ptr(di)))
        else:
            Xo = np.ascontiguousarray(X_arr[order])
            yo = np.ascontiguousarray(y_indices[order].astype(np.int32))
            _lib.check(_lib.lib().mmc_trainer_partial_fit(self._h, Xo.ctypes.data, yo.ctypes.data, n_samples, int(batch_size),
                                                          C.byref(avg), _current_stream_ptr(di)))
        self._end_pass(avg.value)
        return self

    def partial_fit_rows(self, fs, rows=None, classes: Sequence[Any] | None = None, *, row_weight=None,
                         row_group=None, targets=None) -> "TorchMLPClassifier":
        """``partial_fit(X[rows], y[rows], classes)`` for rows that are resident in the ``FeatureSet`` ``fs`` (``rows=None``: every
        row, in stored order): same first-call initialisation, mini-batch size, shuffle, ``loss_curve_`` / ``n_iter_`` -- and the
        same bits.  The shuffle is composed with ``rows`` on the host; only the indices are uploaded
        (``mmc_trainer_partial_fit_set``).  The set's label indices are the classifier's, so ``fs.classes`` must equal
        ``classes_`` and ``fs.dim`` ``n_features_in_`` (``ValueError``); on a first call without ``classes`` the set's class list
        is taken (``partial_fit`` would take the labels present in the rows).

        ``row_weight`` (real, >= 0) and ``row_group`` (integers in ``[0, n_groups)``; needs ``n_groups``) are indexed by row of the
        SET, one entry per stored row, and gathered by the visiting order here (``mmc_trainer_partial_fit_set_weighted``): a weight per
        row, and group DRO over the rows' groups (include/mmc.h, "group-robust training").  Both None is the pass above, bit for bit.

        ``targets`` (a ``TargetSet`` aligned with ``fs``; needs ``distill_alpha > 0``) adds the distillation term: every visited row
        reads its own target row in place (``mmc_trainer_partial_fit_set_distill``; include/mmc.h, "distillation")."""
        rw, rg = check_row_arrays(self, len(fs), row_weight, row_group)
        targets = check_targets(self, fs, targets)
        visit, n_samples, batch_size = self._begin_rows_pass(fs, rows, classes)
        visit, partner, lam = self._mix_plan(visit, n_samples, batch_size)
        avg = C.c_double(0.0)
        if targets is not None:
            rw, rg = by_position(rw, visit, n_samples), by_position(rg, visit, n_samples)
            _lib.check(_lib.lib().mmc_trainer_partial_fit_set_distill(
                self._h, fs._handle(), targets._handle(), None if visit is None else visit.ctypes.data,
                None if rw is None else rw.ctypes.data, None if rg is None else rg.ctypes.data, n_samples, int(batch_size), C.byref(avg),
                _current_stream_ptr(_device_index(self.device))))
        elif rw is not None or rg is not None:
            rw, rg = by_position(rw, visit, n_samples), by_position(rg, visit, n_samples)
            _lib.check(_lib.lib().mmc_trainer_partial_fit_set_weighted(
                self._h, fs._handle(), None if visit is None else visit.ctypes.data, None if rw is None else rw.ctypes.data,
                None if rg is None else rg.ctypes.data, n_samples, int(batch_size), C.byref(avg),
                _current_stream_ptr(_device_index(self.device))))
        elif partner is None:
            _lib.check(_lib.lib().mmc_trainer_partial_fit_set(self._h, fs._handle(), None if visit is None else visit.ctypes.data, n_samples,
                                                              int(batch_size), C.byref(avg), _current_stream_ptr(_device_index(self.device))))
        else:
            _lib.check(_lib.lib().mmc_trainer_partial_fit_set_mixed(self._h, fs._handle(), visit.ctypes.data, partner.ctypes.data,
                                                                    lam.ctypes.data, n_samples, int(batch_size), C.byref(avg),
                                                                    _current_stream_ptr(_device_index(self.device))))
        self._end_pass(avg.value)
        return self

    def _begin_rows_pass(self, fs, rows, classes):
        """The host half of a pass over rows of ``fs``, before any device work on the pass: argument checks, first-call
        initialisation, mini-batch size and shuffle.  -> ``(visit, n, batch_size)``: the visiting order as contiguous int64 row
        indices of the set, or None for every row in stored order.  (``sweep.partial_fit_rows_group`` runs this per classifier
        and hands the results to one grouped call.)"""
        if rows is None:
            n_samples = len(fs)
            rows_arr = None
        else:
            rows_arr = np.asarray(rows)
            if rows_arr.ndim != 1 or not (np.issubdtype(rows_arr.dtype, np.integer) or rows_arr.size == 0):
                raise ValueError(f"rows must be a 1D array of row indices, got {rows_arr.dtype} {rows_arr.shape}")
            rows_arr = rows_arr.astype(np.int64)
            n_samples = int(rows_arr.shape[0])
        if not self._fitted():
            classes_ = fs.classes if classes is None else np.unique(np.asarray(classes))
            if not np.array_equal(fs.classes, classes_):
                raise ValueError(f"the feature set's classes {fs.classes.tolist()} differ from classes_ {classes_.tolist()}")
            self.classes_ = classes_
            self.n_features_in_ = int(fs.dim)
            self.n_iter_ = 0
            self.loss_curve_ = []
            self._class_weight_vector = self._build_class_weight_vector()
            self._logit_prior_vector = self._build_logit_prior_vector()
            self._hierarchy_arrays = self._build_hierarchy_arrays()
            self._create_trainer(*self._initial_parameters())
        else:
            fs._check_against(self)
        if n_samples < 1:
            raise ValueError("partial_fit_rows: no rows")
        batch_size = self._resolve_batch_size(n_samples)
        rng = self._seed_rng()
        order = np.arange(n_samples)
        if self.shuffle:
            rng.shuffle(order)
        if rows_arr is None and not self.shuffle:
            visit = None
        else:
            visit = np.ascontiguousarray((order if rows_arr is None else rows_arr[order]).astype(np.int64))
        return visit, n_samples, batch_size

    def _end_pass(self, avg: float) -> None:
        self.loss_curve_.append(float(avg))
        self.n_iter_ += 1
        self._read_grad_norms()
        self._read_group_weights()

    def fit(self, X, y) -> "TorchMLPClassifier":
        y_arr = np.asarray(y)
        classes = np.unique(y_arr).tolist()
        self._release()
        for attr in ("classes_", "n_features_in_", "n_iter_", "loss_curve_"):
            if hasattr(self, attr):
                delattr(self, attr)
        prev_loss = np.inf
        for _ in range(self.max_iter):
            self.partial_fit(X, y_arr, classes=classes)
            cur = self.loss_curve_[-1]
            if abs(prev_loss - cur) < self.tol:
                break
            prev_loss = cur
        return self

    # ---- inference (pre-calibration semantics the head was fit on) -----------------------------------------------
    def _forward_probs(self, X) -> np.ndarray:
        if not self._fitted():
            raise RuntimeError("TorchMLPClassifier is not fitted. Call partial_fit or fit before predict/predict_proba.")
        X_arr = np.ascontiguousarray(np.asarray(X, dtype=np.float32))
        if X_arr.ndim != 2:
            raise ValueError(f"X must be 2D, got shape {X_arr.shape}")
        if X_arr.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {X_arr.shape[1]} features, expected {self.n_features_in_}")
        n, k = X_arr.shape[0], len(self.classes_)
        logits = np.empty((n, k), dtype=np.float32)
        if n:
            di = _device_index(self.device)
            _lib.check(_lib.lib().mmc_trainer_logits(self._h, X_arr.ctypes.data, n, logits.ctypes.data, _current_stream_ptr(di)))
        z = logits - logits.max(axis=1, keepdims=True)                   # fp32 softmax, then float64 + renormalise
        e = np.exp(z, dtype=np.float32)
        probs_np = (e / e.sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float64)
        row_sums = probs_np.sum(axis=1)
        max_drift = float(np.max(np.abs(row_sums - 1.0))) if n else 0.0
        if max_drift > _EXPECTED_FP_DRIFT_TOL:
            warnings.warn(f"predict_proba row sums deviate from 1.0 by up to {max_drift:.2e}, exceeding the expected float32 "
                          f"softmax drift bound ({_EXPECTED_FP_DRIFT_TOL:.0e}). Renormalizing anyway, but this likely indicates "
                          f"a numerical issue (extreme logits, NaN/Inf, or a bypassed softmax) rather than rounding.",
                          RuntimeWarning, stacklevel=2)
        probs_np /= row_sums[:, np.newaxis]
        return probs_np

    def predict_proba(self, X) -> np.ndarray:
        return self._forward_probs(X)

    def predict(self, X) -> np.ndarray:
        return self.classes_[np.argmax(self._forward_probs(X), axis=1)]

    # ---- parameters ----------------------------------------------------------------------------------------------
    def parameters(self):
        """-> (weights, biases): lists of float32 arrays in ``nn.Linear`` layout, read back from the device -- the weights that
        evaluation reads: the averaged ones of a classifier with ``ema_decay > 0`` (unless ``use_weights("raw")``), else the raw ones."""
        if self._averages() and getattr(self, "_eval_weights", "averaged") == "averaged":
            return self.averaged_parameters()
        if self._normalises():
            return self.folded_parameters()
        return self.raw_parameters()

    def folded_parameters(self):
        """-> (weights, biases) of the stack with batch normalisation folded in (``mmc_trainer_folded_params``): what evaluation reads.
        Of a classifier without ``batch_norm``: ``raw_parameters()``."""
        if not self._fitted():
            raise RuntimeError("TorchMLPClassifier is not fitted.")
        ws = [np.empty((o, i), np.float32) for i, o in zip(self._dims[:-1], self._dims[1:])]
        bs = [np.empty((o,), np.float32) for o in self._dims[1:]]
        _lib.check(_lib.lib().mmc_trainer_folded_params(self._h, _ptr_array(ws), _ptr_array(bs)))
        return ws, bs

    def _bn_arrays(self):
        return [[np.empty((o,), np.float32) for o in self._dims[1:-1]] for _ in range(8)]

    def batch_norm_state(self) -> dict:
        """-> ``{"gamma", "beta", "running_mean", "running_var"}``, each a list with one float32 array per hidden layer
        (``batch_norm=True`` only); ``optim.fold_batch_norm(*raw_parameters(), ...)`` of them is ``parameters()``."""
        if not self._fitted():
            raise RuntimeError("TorchMLPClassifier is not fitted.")
        if not self._normalises():
            raise ValueError("this classifier has no batch normalisation (batch_norm is False).")
        arrays = self._bn_arrays()
        _lib.check(_lib.lib().mmc_trainer_batch_norm_state(self._h, 0, *[_ptr_array(a) for a in arrays]))
        return dict(zip(("gamma", "beta", "running_mean", "running_var"), arrays[:4]))

    def raw_parameters(self):
        """-> (weights, biases) that the training steps read and write, whatever evaluation reads."""
        if not self._fitted():
            raise RuntimeError("TorchMLPClassifier is not fitted.")
        ws = [np.empty((o, i), np.float32) for i, o in zip(self._dims[:-1], self._dims[1:])]
        bs = [np.empty((o,), np.float32) for o in self._dims[1:]]
        _lib.check(_lib.lib().mmc_trainer_get_params(self._h, _ptr_array(ws), _ptr_array(bs)))
        return ws, bs

    def averaged_parameters(self):
        """-> (weights, biases) of the exponential average (``ema_decay > 0`` only)."""
        if not self._fitted():
            raise RuntimeError("TorchMLPClassifier is not fitted.")
        if not self._averages():
            raise ValueError("this classifier keeps no averaged weights (ema_decay is 0).")
        ws = [np.empty((o, i), np.float32) for i, o in zip(self._dims[:-1], self._dims[1:])]
        bs = [np.empty((o,), np.float32) for o in self._dims[1:]]
        _lib.check(_lib.lib().mmc_trainer_ema_state(self._h, 0, _ptr_array(ws), _ptr_array(bs)))
        return ws, bs

    @property
    def _module(self):
        """A torch module with the reference's ``_MLPModule`` layout (``.linears``), built from the current device
        parameters -- what ``build_calibrated_head`` (inference/head.py) and the export path read."""
        import torch
        import torch.nn as nn
        ws, bs = self.parameters()

        class _MLPModule(nn.Module):
            def __init__(self):
                super().__init__()
                self.linears = nn.ModuleList([nn.Linear(w.shape[1], w.shape[0]) for w in ws])
                with torch.no_grad():
                    for m, w, b in zip(self.linears, ws, bs):
                        m.weight.copy_(torch.from_numpy(w))
                        m.bias.copy_(torch.from_numpy(b))

            def forward(self, x):
                for i, m in enumerate(self.linears):
                    x = m(x)
                    if i < len(self.linears) - 1:
                        x = torch.relu(x)
                return x

        return _MLPModule().eval()

    def _adam_state(self):
        out = {}
        step = C.c_longlong(0)
        for which, name in ((0, "exp_avg"), (1, "exp_avg_sq")):
            ws = [np.empty((o, i), np.float32) for i, o in zip(self._dims[:-1], self._dims[1:])]
            bs = [np.empty((o,), np.float32) for o in self._dims[1:]]
            _lib.check(_lib.lib().mmc_trainer_adam_state(self._h, which, 0, _ptr_array(ws), _ptr_array(bs), C.byref(step)))
            out[name] = (ws, bs)
        out["step"] = int(step.value)
        if self._averages():
            out["ema"] = self.averaged_parameters()
        if self._normalises():   # gamma, beta, running mean / variance, then the Adam moments of gamma and beta
            arrays = self._bn_arrays()
            _lib.check(_lib.lib().mmc_trainer_batch_norm_state(self._h, 0, *[_ptr_array(a) for a in arrays]))
            out["batch_norm"] = arrays
        return out

    def get_params(self, deep: bool = True) -> dict:
        return {"hidden_layer_sizes": self.hidden_layer_sizes, "activation": self.activation, "solver": self.solver,
                "alpha": self.alpha, "batch_size": self.batch_size, "learning_rate_init": self.learning_rate_init,
                "max_iter": self.max_iter, "shuffle": self.shuffle, "random_state": self.random_state, "tol": self.tol,
                "beta_1": self.beta_1, "beta_2": self.beta_2, "epsilon": self.epsilon,
                "class_weight": getattr(self, "class_weight", None), "label_smoothing": self.label_smoothing,
                "focal_gamma": self.focal_gamma, "logit_prior": self.logit_prior, "dropout": self.dropout,
                "input_dropout": self.input_dropout, "mixup_alpha": self.mixup_alpha, "regularizer_seed": self.regularizer_seed,
                "lr_schedule": self.lr_schedule, "warmup_steps": self.warmup_steps, "schedule_steps": self.schedule_steps,
                "final_lr_ratio": self.final_lr_ratio, "max_grad_norm": self.max_grad_norm, "ema_decay": self.ema_decay,
                "group_dro_eta": self.group_dro_eta, "n_groups": self.n_groups, "class_levels": self.class_levels,
                "level_weights": self.level_weights, "soft_targets": self.soft_targets, "batch_norm": self.batch_norm,
                "batch_norm_eps": self.batch_norm_eps, "batch_norm_momentum": self.batch_norm_momentum,
                "distill_alpha": self.distill_alpha, "distill_temperature": self.distill_temperature}

    def set_params(self, **params: Any) -> "TorchMLPClassifier":
        for key, value in params.items():
            if not hasattr(self, key):
                raise ValueError(f"Invalid parameter {key!r} for TorchMLPClassifier")
            setattr(self, key, value)
        return self

    # ---- pickling: parameters + optimizer state as arrays, rebuilt on load (torch_classifier.py:404-437) ------------
    def __getstate__(self) -> dict:
        state = {k: v for k, v in self.__dict__.items() if k != "_h"}
        if self._fitted():
            state["_module_state"] = self.raw_parameters()
            state["_optimizer_state"] = self._adam_state()
        return state

    def __setstate__(self, state: dict) -> None:
        params = state.pop("_module_state", None)
        opt = state.pop("_optimizer_state", None)
        self.__dict__.update(state)
        # a pickle made before the loss options existed loads as the plain loss
        # ... and one made before the regularisers existed as a classifier without them
        for key, default in (("label_smoothing", 0.0), ("focal_gamma", 0.0), ("logit_prior", None), ("_logit_prior_vector", None),
                             ("dropout", 0.0), ("input_dropout", 0.0), ("mixup_alpha", 0.0), ("regularizer_seed", None),
                             # ... and one made before the optimiser options existed with the constant rate, unclipped, unaveraged
                             ("lr_schedule", "constant"), ("warmup_steps", 0), ("schedule_steps", None), ("final_lr_ratio", 0.0),
                             ("max_grad_norm", None), ("ema_decay", 0.0),
                             # ... and one made before group DRO existed without it
                             ("group_dro_eta", 0.0), ("n_groups", None),
                             # ... and one made before the taxonomy-aware loss existed with the flat loss
                             ("class_levels", None), ("level_weights", None), ("soft_targets", None), ("_hierarchy_arrays", None),
                             # ... and one made before batch normalisation existed as a plain head
                             ("batch_norm", False), ("batch_norm_eps", 1e-5), ("batch_norm_momentum", 0.1),
                             # ... and one made before distillation existed as a student of its labels alone
                             ("distill_alpha", 0.0), ("distill_temperature", 1.0)):
            self.__dict__.setdefault(key, default)
        self._h = None
        if params is not None:
            self._create_trainer(*params)
            if opt is not None:
                step = C.c_longlong(opt["step"])
                for which, name in ((0, "exp_avg"), (1, "exp_avg_sq")):
                    ws, bs = opt[name]
                    _lib.check(_lib.lib().mmc_trainer_adam_state(self._h, which, 1, _ptr_array(ws), _ptr_array(bs), C.byref(step)))
                if self._averages() and opt.get("ema") is not None:   # without one the shadow stays the parameters just loaded
                    ws, bs = opt["ema"]
                    _lib.check(_lib.lib().mmc_trainer_ema_state(self._h, 1, _ptr_array(ws), _ptr_array(bs)))
                if self._normalises() and opt.get("batch_norm") is not None:   # without one the statistics start afresh
                    arrays = [[np.ascontiguousarray(a, dtype=np.float32) for a in group] for group in opt["batch_norm"]]
                    _lib.check(_lib.lib().mmc_trainer_batch_norm_state(self._h, 1, *[_ptr_array(a) for a in arrays]))
            logq = self.__dict__.get("_group_logq")
            if self.n_groups is not None and logq is not None and len(logq) == int(self.n_groups):   # q continues where it was
                logq = np.ascontiguousarray(logq, dtype=np.float64)
                _lib.check(_lib.lib().mmc_trainer_group_dro_state(self._h, 1, logq.ctypes.data))

    def _release(self) -> None:
        if self._fitted():
            _lib.lib().mmc_trainer_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass
