"""A hyper-parameter sweep of MLP heads trained in lockstep on the MI355X.

The reference trains one head per run of ``MermaidTrainer.__call__`` (``mermaid_classifier/pyspacer/trainer.py:83-293``); the
sweeps that fixed its production recipe (``docs/research/hidden-layer-experiments.md``: architectures x learning rates;
``docs/research/balancing-experiments.md``: 15 configurations screened, 3 confirmed) were S such runs side by side.  On one
MI355X a single head's Adam step is some 30 small launches that leave most of the device idle, so S runs one after the other are
the worst way to spend it.  Here the S models advance together:

``partial_fit_rows_group``  one pass of ``TorchMLPClassifier.partial_fit_rows`` for each of several classifiers over one resident
                            ``FeatureSet``, in one ``mmc_trainer_group_partial_fit_set`` call per 16 of them -- every kind of
                            launch of a step once for the whole group.  Same bits as the passes made one by one.
``SweepConfig``             what a sweep varies: the classifier's constructor arguments and the row-subset hook.
``sweep_loop``              ``training.epoch_loop`` for several models at once, device steps passed in (testable without a device).
``train_sweep``             ``training.train_classifier`` for every configuration, in lockstep: entry i of the result is what
                            ``train_classifier`` returns for configuration i run alone.

``rank_sweep``              the study's promotion rule over ``train_sweep``'s result: every calibrated model scored on the validation
                            split (``validate`` / ``grouped_validate``), sorted by balanced accuracy, then macro f1.

What a balancing configuration is made of comes from ``sampling.py``: ``effective_number_weights`` -> ``SweepConfig.class_weight``,
``subsample_targets`` / ``subsample_rows`` / ``row_batches`` -> ``SweepConfig.batches``, ``logit_adjustment`` ->
``SweepConfig.logit_prior``.  With ``class_scores=True`` every epoch's
callback dict carries the validation balanced accuracy and macro f1 next to the accuracy (``calibration.evaluate_classes``).

Evaluation and calibration stay per model (``calibration.evaluate`` / ``evaluate_classes`` / ``calibrate``): they are forward-only
at 16 384 rows a chunk and fill the device on their own.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, feature_transform as _ft, logit_scaling as _ls
from .backbone import _current_stream_ptr, _device_index
from .calibration import CalibratedMLP, calibrate, evaluate, evaluate_classes
from .featureset import FeatureSet
from .metrics import grouped_validate
from .torch_classifier import TorchMLPClassifier, by_position, check_row_arrays, check_targets
from .training import EarlyStopping, _check_splits, _contiguous_batches, _fill_schedule_steps, _val_entries, resolve_targets
from .validation import validate

__all__ = ["SweepConfig", "partial_fit_rows_group", "sweep_loop", "train_sweep", "rank_sweep"]


def _rows_per_classifier(rows, count: int) -> List[Any]:
    """``rows`` as one entry per classifier: None and a single index array stand for every classifier; a list / tuple whose
    entries are all None or arrays is taken per classifier and must have ``count`` entries."""
    if rows is None:
        return [None] * count
    if isinstance(rows, (list, tuple)) and len(rows) > 0 and all(r is None or np.ndim(r) >= 1 for r in rows):
        if len(rows) != count:
            raise ValueError(f"rows has {len(rows)} entries for {count} classifiers")
        entries = list(rows)
    else:
        entries = [rows] * count
    for r in entries:
        if r is None:
            continue
        arr = np.asarray(r)
        if arr.ndim != 1 or not (np.issubdtype(arr.dtype, np.integer) or arr.size == 0):
            raise ValueError(f"rows must be a 1D array of row indices, got {arr.dtype} {arr.shape}")
    return entries


def _arrays_per_classifier(name: str, arr, count: int) -> List[Any]:
    """``row_weight`` / ``row_group`` as one entry per classifier: None and a single array stand for every classifier; a list / tuple
    whose entries are all None or arrays is taken per classifier and must have ``count`` entries."""
    if arr is None:
        return [None] * count
    if isinstance(arr, (list, tuple)) and len(arr) > 0 and all(a is None or np.ndim(a) >= 1 for a in arr):
        if len(arr) != count:
            raise ValueError(f"{name} has {len(arr)} entries for {count} classifiers")
        return list(arr)
    return [arr] * count


def _targets_per_classifier(targets, count: int) -> List[Any]:
    """``targets`` as one entry per classifier: None and a single ``TargetSet`` stand for every classifier; a list / tuple is taken
    per classifier (``TargetSet`` or None) and must have ``count`` entries."""
    if isinstance(targets, (list, tuple)):
        if len(targets) != count:
            raise ValueError(f"targets has {len(targets)} entries for {count} classifiers")
        return list(targets)
    return [targets] * count


def partial_fit_rows_group(clfs: Sequence[TorchMLPClassifier], fs: FeatureSet, rows=None,
                           classes: Optional[Sequence[Any]] = None, *, row_weight=None, row_group=None,
                           targets=None) -> List[TorchMLPClassifier]:
    """``clf.partial_fit_rows(fs, rows_m, classes)`` for every classifier of ``clfs``, with the device work of all of them in one
    ``mmc_trainer_group_partial_fit_set`` call per ``MMC_TRAINER_GROUP_MAX`` (16) classifiers.  Parameters, Adam state,
    ``loss_curve_`` and ``n_iter_`` of each end up exactly as after its own ``partial_fit_rows``.

    ``rows``: None (every row of the set, for everyone), one index array for all, or a list with one entry -- array or None --
    per classifier.  The classifiers may differ in everything a ``TorchMLPClassifier`` can be configured with (depth, widths,
    optimizer settings, class weights, mini-batch size, shuffle, seed) and in how many passes they have behind them.

    ``row_weight`` / ``row_group`` as in ``partial_fit_rows`` (indexed by row of the set): None, one array for all, or a list with one
    entry -- array or None -- per classifier.  A classifier whose two entries are None runs its plain kernels beside the others
    (``mmc_trainer_group_partial_fit_set_weighted``).  One call of at most 16 classifiers cannot hold both a weighted member and one
    with ``mixup_alpha > 0`` (``ValueError``): no entry point takes both.

    ``targets`` as in ``partial_fit_rows``: None, one ``TargetSet`` for all, or a list with one entry -- ``TargetSet`` or None -- per
    classifier; the members may share one set or use different ones, and a member without one runs its own kernels beside the others
    (``mmc_trainer_group_partial_fit_set_distill``).  Members with targets count as weighted ones in the rule above.

    ``ValueError`` before any device work: ``rows`` that do not fit ``clfs``, the same classifier twice, a classifier on another
    device than the set.  A pass the library rejects (an index outside the set, a mini-batch of zero class weight, ...) raises
    as ``partial_fit_rows`` does and changes none of the classifiers of that call."""
    clfs = list(clfs)
    entries = _rows_per_classifier(rows, len(clfs))
    weights = _arrays_per_classifier("row_weight", row_weight, len(clfs))
    groups = _arrays_per_classifier("row_group", row_group, len(clfs))
    soft = _targets_per_classifier(targets, len(clfs))
    if len({id(c) for c in clfs}) != len(clfs):
        raise ValueError("the same classifier appears twice in clfs")
    arrays = [check_row_arrays(clf, len(fs), w, g) for clf, w, g in zip(clfs, weights, groups)]
    soft = [check_targets(clf, fs, t) for clf, t in zip(clfs, soft)]
    for i, clf in enumerate(clfs):
        if _device_index(clf.device) != fs.device_index:
            raise ValueError(f"classifier {i} is on device {_device_index(clf.device)}, the feature set on device {fs.device_index}")
    lib = _lib.lib()
    for first in range(0, len(clfs), _lib.MMC_TRAINER_GROUP_MAX):
        group = clfs[first:first + _lib.MMC_TRAINER_GROUP_MAX]
        members = arrays[first:first + _lib.MMC_TRAINER_GROUP_MAX]
        teachers = soft[first:first + _lib.MMC_TRAINER_GROUP_MAX]
        distilled = any(t is not None for t in teachers)
        weighted = distilled or any(w is not None or g is not None for w, g in members)
        if weighted and any(float(clf.mixup_alpha) != 0.0 for clf in group):
            raise ValueError(f"one grouped call cannot hold members with {'targets' if distilled else 'row_weight / row_group'} and members "
                             "with mixup_alpha > 0")
        passes = [clf._begin_rows_pass(fs, r, classes) for clf, r in zip(group, entries[first:])]
        plans = [clf._mix_plan(v, n_m, b_m) for clf, (v, n_m, b_m) in zip(group, passes)]     # (visit, partner, lam) per member
        count = len(group)
        handles = (C.c_void_p * count)(*[clf._h.value for clf in group])
        visit = (C.c_void_p * count)(*[None if v is None else v.ctypes.data for v, _, _ in plans])
        n = (C.c_int64 * count)(*[int(p[1]) for p in passes])
        batch = (C.c_int * count)(*[int(p[2]) for p in passes])
        avg = (C.c_double * count)()
        if weighted:                                          # a member without either keeps a NULL pair: its plain kernels
            pos = [(by_position(w, v, n_m), by_position(g, v, n_m)) for (w, g), (v, _, _), (_, n_m, _) in zip(members, plans, passes)]
            rw = (C.c_void_p * count)(*[None if w is None else w.ctypes.data for w, _ in pos])
            rg = (C.c_void_p * count)(*[None if g is None else g.ctypes.data for _, g in pos])
            if distilled:                                     # a member without targets keeps a NULL entry: its own kernels
                ts = (C.c_void_p * count)(*[None if t is None else t._handle().value for t in teachers])
                _lib.check(lib.mmc_trainer_group_partial_fit_set_distill(handles, count, fs._handle(), ts, visit, rw, rg, n, batch, avg,
                                                                         _current_stream_ptr(fs.device_index)))
            else:
                _lib.check(lib.mmc_trainer_group_partial_fit_set_weighted(handles, count, fs._handle(), visit, rw, rg, n, batch, avg,
                                                                          _current_stream_ptr(fs.device_index)))
        elif all(partner is None for _, partner, _ in plans):
            _lib.check(lib.mmc_trainer_group_partial_fit_set(handles, count, fs._handle(), visit, n, batch, avg,
                                                             _current_stream_ptr(fs.device_index)))
        else:                                                 # a member without mixup keeps a NULL pair: it is not mixed
            partner = (C.c_void_p * count)(*[None if q is None else q.ctypes.data for _, q, _ in plans])
            lam = (C.c_void_p * count)(*[None if w is None else w.ctypes.data for _, _, w in plans])
            _lib.check(lib.mmc_trainer_group_partial_fit_set_mixed(handles, count, fs._handle(), visit, partner, lam, n, batch, avg,
                                                                   _current_stream_ptr(fs.device_index)))
        for clf, a in zip(group, avg):
            clf._end_pass(a)
    return clfs


@dataclass
class SweepConfig:
    """One configuration of a sweep: the ``TorchMLPClassifier`` constructor arguments a sweep varies (the defaults are the
    production head's, trainer.py:118-123) and ``batches``, ``train_classifier``'s row-subset hook -- a callable
    ``epoch -> iterable of row-index arrays`` into the train set, e.g. a class-balancing subsample; None takes contiguous
    slices of ``train_sweep``'s ``batch_size`` rows.  ``label_smoothing`` / ``focal_gamma`` / ``logit_prior`` are the classifier's loss
    formulation (``mmc_trainer_set_loss``): the members of one grouped pass may each have their own.  ``logit_scaling`` (keyword only)
    is ``train_classifier``'s argument of that name for this configuration.  ``dropout`` / ``input_dropout`` / ``mixup_alpha`` /
    ``regularizer_seed`` are the classifier's regularisers, again per member, and so are its optimiser options ``lr_schedule`` /
    ``warmup_steps`` / ``schedule_steps`` / ``final_lr_ratio`` / ``max_grad_norm`` / ``ema_decay`` (keyword only; a decaying schedule
    with ``schedule_steps=None`` ends after ``nbr_epochs`` epochs of this member's own steps).  ``row_weight`` / ``row_group`` (keyword
    only; arrays indexed by row of the train set) go to every pass of this member, ``group_dro_eta`` / ``n_groups`` to its classifier:
    one sweep can hold an ERM member, a group-balanced one (``group_dro_eta=0``) and DRO members side by side.  ``class_levels`` /
    ``level_weights`` / ``soft_targets`` (keyword only) are the classifier's taxonomy-aware loss: flat, level-weighted and soft-label
    heads can train side by side.  ``batch_norm`` / ``batch_norm_eps`` / ``batch_norm_momentum`` (keyword only) are the classifier's batch
    normalisation (``mmc_trainer_set_batch_norm``): plain and normalised heads, say at ``1e-4`` and ``1e-3``, can train side by side.
    ``distill_alpha`` / ``distill_temperature`` (keyword only) are the classifier's distillation options: with ``train_sweep(targets=)``
    or ``(teacher=)`` the members with ``distill_alpha > 0`` read the shared target set, the others train on their labels alone."""
    hidden_layer_sizes: Tuple[int, ...] = (500, 300, 100)
    learning_rate_init: float = 1e-4
    alpha: float = 1e-4
    class_weight: Optional[dict] = None
    random_state: Optional[int] = 0
    batch_size: Any = "auto"
    beta_1: float = 0.9
    beta_2: float = 0.999
    epsilon: float = 1e-8
    # keyword-only, so it takes no positional slot: a kind string or a fitted LogitScaling, fitted on ref after training and folded
    # before calibrate (train_sweep's logit_scaling= for one configuration); not a classifier argument
    logit_scaling: Any = field(default=None, kw_only=True)
    # the classifier's regularisers (mmc_trainer_set_dropout, sampling.mixup_plan): keyword only, as in its constructor
    dropout: float = field(default=0.0, kw_only=True)
    input_dropout: float = field(default=0.0, kw_only=True)
    mixup_alpha: float = field(default=0.0, kw_only=True)
    regularizer_seed: Optional[int] = field(default=None, kw_only=True)
    # the classifier's optimiser options (mmc_trainer_set_lr_schedule / _set_grad_clip / _set_ema): keyword only, as in its constructor
    lr_schedule: str = field(default="constant", kw_only=True)
    warmup_steps: int = field(default=0, kw_only=True)
    schedule_steps: Optional[int] = field(default=None, kw_only=True)
    final_lr_ratio: float = field(default=0.0, kw_only=True)
    max_grad_norm: Optional[float] = field(default=None, kw_only=True)
    ema_decay: float = field(default=0.0, kw_only=True)
    # group-robust training (include/mmc.h): the member's per-row arrays over the train set and its classifier's group DRO
    row_weight: Any = field(default=None, kw_only=True)
    row_group: Any = field(default=None, kw_only=True)
    group_dro_eta: float = field(default=0.0, kw_only=True)
    n_groups: Optional[int] = field(default=None, kw_only=True)
    # the classifier's taxonomy-aware loss (mmc_trainer_set_hierarchy): keyword only, as in its constructor
    class_levels: Optional[dict] = field(default=None, kw_only=True)
    level_weights: Optional[Sequence[float]] = field(default=None, kw_only=True)
    soft_targets: Optional[dict] = field(default=None, kw_only=True)
    # the classifier's batch normalisation (mmc_trainer_set_batch_norm): keyword only, as in its constructor
    batch_norm: bool = field(default=False, kw_only=True)
    batch_norm_eps: float = field(default=1e-5, kw_only=True)
    batch_norm_momentum: float = field(default=0.1, kw_only=True)
    # the classifier's distillation options (mmc_trainer_set_distillation): keyword only, as in its constructor
    distill_alpha: float = field(default=0.0, kw_only=True)
    distill_temperature: float = field(default=1.0, kw_only=True)
    batches: Optional[Callable[[int], Iterable[np.ndarray]]] = None
    label_smoothing: float = 0.0
    focal_gamma: float = 0.0
    logit_prior: Optional[dict] = None

    def classifier(self, device=0) -> TorchMLPClassifier:
        """The untrained classifier of this configuration."""
        return TorchMLPClassifier(hidden_layer_sizes=tuple(self.hidden_layer_sizes), learning_rate_init=self.learning_rate_init,
                                  alpha=self.alpha, class_weight=self.class_weight, random_state=self.random_state,
                                  batch_size=self.batch_size, beta_1=self.beta_1, beta_2=self.beta_2, epsilon=self.epsilon,
                                  device=device, label_smoothing=self.label_smoothing, focal_gamma=self.focal_gamma,
                                  logit_prior=self.logit_prior, dropout=self.dropout, input_dropout=self.input_dropout,
                                  mixup_alpha=self.mixup_alpha, regularizer_seed=self.regularizer_seed,
                                  lr_schedule=self.lr_schedule, warmup_steps=self.warmup_steps, schedule_steps=self.schedule_steps,
                                  final_lr_ratio=self.final_lr_ratio, max_grad_norm=self.max_grad_norm, ema_decay=self.ema_decay,
                                  group_dro_eta=self.group_dro_eta, n_groups=self.n_groups, class_levels=self.class_levels,
                                  level_weights=self.level_weights, soft_targets=self.soft_targets, batch_norm=self.batch_norm,
                                  batch_norm_eps=self.batch_norm_eps, batch_norm_momentum=self.batch_norm_momentum,
                                  distill_alpha=self.distill_alpha, distill_temperature=self.distill_temperature)


def sweep_loop(clfs: Sequence[Any], batches: Sequence[Callable[[int], Iterable[Any]]],
               fit_group: Callable[[List[Any], List[Any]], None], eval_ref: Callable[[Any], float],
               eval_val: Callable[[Any], Tuple[float, float]], nbr_epochs: int, early_stopping_patience: Optional[int] = None,
               on_epoch_end: Optional[Callable[[Dict[str, Any]], None]] = None, class_scores: bool = False
               ) -> List[Tuple[Any, Dict[str, Any]]]:
    """``training.epoch_loop`` for the models ``clfs`` in lockstep.  -> one ``(clf, info)`` per model, each what ``epoch_loop``
    returns for that model alone.

    An epoch walks the outer batch positions: at position p, ``fit_group(models, rows)`` is called once with the models whose
    ``batches[i](epoch)`` has a p-th entry and those entries (a model with fewer batches sits the later positions out).  Then every
    model still running is scored -- ``eval_ref(clf) -> accuracy``, ``eval_val(clf) -> (accuracy, log_loss)`` -- and its own
    ``EarlyStopping`` decides: best snapshot, patience, stop.  A model that has stopped takes no further part.
    ``on_epoch_end`` gets ``epoch_loop``'s dict plus ``"config"``, the model's index, once per model and epoch.  With
    ``class_scores=True``, ``eval_val(clf)`` returns ``(accuracy, log_loss, ClassScores)`` and the dict gains
    ``val_balanced_accuracy`` and ``val_f1_macro``, as in ``epoch_loop``; the decisions still read ``val_loss`` alone."""
    clfs = list(clfs)
    if len(batches) != len(clfs):
        raise ValueError(f"{len(batches)} batch callables for {len(clfs)} models")
    states = [EarlyStopping(nbr_epochs, early_stopping_patience) for _ in clfs]
    live = list(range(len(clfs)))
    done = object()
    for epoch in range(int(nbr_epochs)):
        its = {i: iter(batches[i](epoch)) for i in live}
        while its:
            rows = {i: next(it, done) for i, it in its.items()}
            its = {i: it for i, it in its.items() if rows[i] is not done}
            if its:
                fit_group([clfs[i] for i in its], [rows[i] for i in its])
        for i in live:
            ref_acc = eval_ref(clfs[i])
            val_acc, val_loss, extra = _val_entries(eval_val(clfs[i]), class_scores)
            metrics = states[i].epoch_done(clfs[i], epoch, ref_acc, val_acc, val_loss, extra=extra)
            if on_epoch_end is not None:
                metrics["config"] = i
                on_epoch_end(metrics)
        live = [i for i in live if not states[i].stopped]
        if not live:
            break
    return [state.result(clf) for state, clf in zip(states, clfs)]


def train_sweep(train: FeatureSet, ref: FeatureSet, val: FeatureSet, configs: Sequence[SweepConfig], nbr_epochs: int, *,
                batch_size: int, early_stopping_patience: Optional[int] = None,
                on_epoch_end: Optional[Callable[[Dict[str, Any]], None]] = None, class_scores: bool = False, transform=None,
                logit_scaling=None, targets=None, teacher=None) -> List[Tuple[CalibratedMLP, Dict[str, Any], List[float]]]:
    """Train, early-stop and calibrate one head per configuration on three resident splits, all heads advancing in the same
    launches.  -> one ``(calibrated, info, ref_accs)`` per configuration, equal to
    ``train_classifier(train, ref, val, nbr_epochs, batch_size=batch_size, early_stopping_patience=..., batches=cfg.batches,
    clf=cfg.classifier(ref.device))`` run alone: parameters, Platt a / b, ``info`` and ``ref_accs``.

    Per epoch: one ``partial_fit_rows_group`` per outer batch position over the models that have a batch there, then
    ``evaluate`` on ``ref`` and ``val`` per model, then each model's early-stopping decision; a stopped model drops out.  At the
    end ``calibrate`` per returned classifier.  ``on_epoch_end`` gets ``epoch_loop``'s dict plus ``"config"``.
    ``class_scores=True`` scores ``val`` through ``calibration.evaluate_classes``: the dict gains ``val_balanced_accuracy`` and
    ``val_f1_macro`` per model and epoch, and nothing returned changes.

    ``transform`` as in ``train_classifier``: one transform (given, or fitted on ``train``) for the whole sweep; the splits are
    transformed once, every head trains on the transformed sets, and every model returned is folded.

    ``logit_scaling`` as in ``train_classifier``, for every configuration; a configuration's own ``SweepConfig.logit_scaling`` wins over
    it.  A configuration with neither is calibrated exactly as before.

    A configuration's ``row_weight`` / ``row_group`` go to each of its passes (``partial_fit_rows_group``); with ``transform=`` they
    index the transformed train set, which has the train set's rows.

    ``targets`` / ``teacher`` as in ``train_classifier``, one or the other: one target set for the whole sweep (a teacher's is made
    for the raw ``train`` and freed at the end).  The configurations with ``distill_alpha > 0`` read it in every pass; the others are
    trained exactly as without it, so label-only and distilled students at several alpha, tau advance side by side."""
    configs = list(configs)
    if not configs:
        raise ValueError("configs is empty")
    _check_splits(train, ref, val, batch_size)
    if teacher is not None:
        targets = resolve_targets(targets, teacher, train)
        try:
            return train_sweep(train, ref, val, configs, nbr_epochs, batch_size=batch_size, early_stopping_patience=early_stopping_patience,
                               on_epoch_end=on_epoch_end, class_scores=class_scores, transform=transform, logit_scaling=logit_scaling,
                               targets=targets)
        finally:
            targets.close()
    scalings = [cfg.logit_scaling if cfg.logit_scaling is not None else logit_scaling for cfg in configs]
    for sc in scalings:
        if sc is not None:
            _ls.check_argument(sc)
    if transform is not None:
        ft = _ft.resolve(transform, train)
        sets = []
        try:
            for fs in (train, ref, val):
                sets.append(ft.apply(fs))
            results = train_sweep(*sets, configs, nbr_epochs, batch_size=batch_size, early_stopping_patience=early_stopping_patience,
                                  on_epoch_end=on_epoch_end, class_scores=class_scores, logit_scaling=logit_scaling, targets=targets)
        finally:
            for fs in sets:
                fs.close()
        return [(cal.folded(ft), info, accs) for cal, info, accs in results]
    classes = ref.classes.tolist()
    clfs = [cfg.classifier(ref.device) for cfg in configs]
    batches = [cfg.batches if cfg.batches is not None else _contiguous_batches(len(train), int(batch_size)) for cfg in configs]
    for c, b in zip(clfs, batches):
        _fill_schedule_steps(c, b, nbr_epochs)
    ref_accs: Dict[int, List[float]] = {id(c): [] for c in clfs}

    def eval_ref(c):
        acc = evaluate(c, ref)[0]
        ref_accs[id(c)].append(acc)
        return acc

    eval_val = evaluate_classes if class_scores else evaluate
    member = {id(c): cfg for c, cfg in zip(clfs, configs)}

    def member_targets(c):   # the shared set for the members that distil, nothing for the others
        return targets if targets is not None and float(member[id(c)].distill_alpha) != 0.0 else None

    def fit_group(group, rows):
        if any(member_targets(c) is not None for c in group):
            return partial_fit_rows_group(group, train, rows, classes=classes, row_weight=[member[id(c)].row_weight for c in group],
                                          row_group=[member[id(c)].row_group for c in group], targets=[member_targets(c) for c in group])
        if all(member[id(c)].row_weight is None and member[id(c)].row_group is None for c in group):
            return partial_fit_rows_group(group, train, rows, classes=classes)
        return partial_fit_rows_group(group, train, rows, classes=classes, row_weight=[member[id(c)].row_weight for c in group],
                                      row_group=[member[id(c)].row_group for c in group])

    results = sweep_loop(clfs, batches, fit_group,
                         eval_ref, lambda c: eval_val(c, val), nbr_epochs, early_stopping_patience=early_stopping_patience,
                         on_epoch_end=on_epoch_end, class_scores=class_scores)
    return [(calibrate(clf, ref) if sc is None else calibrate(clf, ref, logit_scaling=sc), info, ref_accs[id(live)])
            for (clf, info), live, sc in zip(results, clfs, scalings)]


def rank_sweep(results: Sequence[Tuple[CalibratedMLP, Dict[str, Any], Any]], val, *, image_sizes=None,
               n_bins: int = 20) -> List[Dict[str, Any]]:
    """Rank the configurations of a sweep the way the balancing study promotes them (docs/research/balancing-experiments.md:43):
    by ``balanced_accuracy`` descending, ties by ``f1_macro`` descending, then by configuration index.

    ``results`` is what ``train_sweep`` returned (or any sequence of ``(calibrated, info, ...)``); every calibrated model is scored
    on ``val`` on the device, totals only -- ``validate(model, val, rows=False)``, or ``grouped_validate(model, val, image_sizes,
    n_bins=n_bins)`` when ``image_sizes`` is given.  -> one dict per configuration, best first: ``config`` (its index in
    ``results``), ``balanced_accuracy``, ``f1_macro``, ``mcc`` (``Validation.class_scores()``), ``accuracy``, ``log_loss`` (the
    ``Validation``'s), ``best_val_epoch`` and ``final_epoch`` (from ``info``; the screen-versus-confirmation caveat of :67, 82 is
    about how early these are); with ``image_sizes`` also ``cover_median_r_squared`` (``CoverStats.scalars()``) and ``ece``
    (``Reliability.ece``), the columns the study reports beside the ranking (:17-19)."""
    rows = []
    for i, entry in enumerate(results):
        model, info = entry[0], entry[1]
        if image_sizes is None:
            grouped, scored = None, validate(model, val, rows=False)
        else:
            grouped = grouped_validate(model, val, image_sizes, n_bins=n_bins)
            scored = grouped.validation
        cs = scored.class_scores()
        row = {"config": i, "balanced_accuracy": cs.balanced_accuracy, "f1_macro": cs.f1_macro, "accuracy": scored.accuracy,
               "mcc": cs.mcc, "log_loss": scored.log_loss, "best_val_epoch": info.get("best_val_epoch"),
               "final_epoch": info.get("final_epoch")}
        if grouped is not None:
            row["cover_median_r_squared"] = grouped.cover.scalars()["cover_median_r_squared"]
            row["ece"] = grouped.reliability.ece
        rows.append(row)
    rows.sort(key=lambda r: (-r["balanced_accuracy"], -r["f1_macro"], r["config"]))
    return rows
