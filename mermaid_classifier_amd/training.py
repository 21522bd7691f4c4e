"""The epoch loop of the reference's ``MermaidTrainer.__call__`` (``mermaid_classifier/pyspacer/trainer.py:83-293``) over splits
that are resident on the MI355X.

``epoch_loop`` is the host bookkeeping of :128-259 in this project's words -- epochs, early stopping on the validation loss,
best-snapshot restore, the per-epoch callback and the stop summary -- with the three device steps passed in as callables, so it
runs (and is tested) without a device.  ``train_classifier`` binds those callables to ``FeatureSet`` splits
(``TorchMLPClassifier.partial_fit_rows``, ``calibration.evaluate``) and ends, as :261-265 does, with the Platt calibration on the
ref split.  ``train_and_validate`` adds what follows there (:267-293) -- ``evaluate_classifier`` on val, ``ValResults``, the
previous models' accuracies -- through ``validation.validate``, and returns the reference's triple.
"""

from __future__ import annotations

import copy
import time
from typing import Any, Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import feature_transform as _ft, logit_scaling as _ls
from .calibration import CalibratedMLP, calibrate, evaluate, evaluate_classes
from .featureset import FeatureSet
from .torch_classifier import TorchMLPClassifier
from .validation import previous_accuracies, validate

__all__ = ["EarlyStopping", "epoch_loop", "train_classifier", "train_and_validate"]


def resolve_targets(targets, teacher, train):
    """``targets=`` / ``teacher=`` of a training call -> the target set, or None.  One or the other (``ValueError`` for both); a
    teacher's targets are made for ``train`` as it is given (``distill.teacher_targets``) and are the caller's to close.
    (``sweep.train_sweep`` resolves its arguments the same way.)"""
    if targets is not None and teacher is not None:
        raise ValueError("pass targets or teacher, not both")
    if teacher is None:
        return targets
    from .distill import teacher_targets
    return teacher_targets(teacher, train)


class EarlyStopping:
    """``epoch_loop``'s bookkeeping for one model: best validation loss so far with its epoch and ``copy.deepcopy`` snapshot,
    epochs since the last improvement, and what the callback dict and the stop summary are made of.  ``epoch_loop`` keeps one,
    ``sweep.sweep_loop`` one per model of the sweep."""

    def __init__(self, nbr_epochs: int, patience: Optional[int] = None):
        if int(nbr_epochs) < 1:
            raise ValueError(f"nbr_epochs must be >= 1, got {nbr_epochs!r}")
        if patience is not None and patience < 1:
            raise ValueError(f"early_stopping_patience must be >= 1 or None, got {patience!r}")
        self.nbr_epochs, self.patience = nbr_epochs, patience
        self.best_loss, self.best_epoch, self.best_clf = float("inf"), None, None
        self.since_best = 0
        self.epoch = 0            # the last epoch run (0-based)
        self.stopped = False      # out of patience
        self.t0 = time.time()

    def epoch_done(self, clf, epoch: int, ref_acc: float, val_acc: float, val_loss: float, *,
                   extra: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
        """Record epoch ``epoch`` of ``clf`` (snapshot it when it is the best so far).  -> the epoch's callback dict; ``stopped``
        says whether the patience has run out.  ``extra`` entries are added to the dict and decide nothing."""
        self.epoch = epoch
        if self.patience is not None:
            if val_loss < self.best_loss:
                self.best_loss, self.best_epoch, self.best_clf = val_loss, epoch, copy.deepcopy(clf)
                self.since_best = 0
            else:
                self.since_best += 1
        self.stopped = self.patience is not None and self.since_best >= self.patience
        curve = getattr(clf, "loss_curve_", [None])
        metrics: Dict[str, Any] = {"epoch": epoch, "ref_accuracy": ref_acc, "val_accuracy": val_acc, "val_loss": val_loss,
                                   "training_loss": curve[-1] if curve else None, "cumulative_seconds": time.time() - self.t0}
        if extra:
            metrics.update(extra)
        if self.stopped or epoch == self.nbr_epochs - 1:
            metrics["final_epoch"] = epoch + 1
            metrics["early_stopped"] = self.stopped
            if self.best_epoch is not None:
                metrics["best_val_epoch"] = self.best_epoch + 1
                metrics["best_val_loss"] = self.best_loss
        return metrics

    def result(self, clf) -> Tuple[Any, Dict[str, Any]]:
        """-> ``(clf, info)`` after the last epoch run: the best snapshot when the best epoch is not the last one."""
        if self.best_clf is not None and self.best_epoch != self.epoch:
            clf = self.best_clf
        info = {"enabled": self.patience is not None, "patience": self.patience,
                "stop_reason": "early_stopping" if self.stopped else "budget_exhausted", "final_epoch": self.epoch + 1,
                "best_val_epoch": None if self.best_epoch is None else self.best_epoch + 1,
                "best_val_loss": None if self.best_epoch is None else self.best_loss}
        return clf, info


def epoch_loop(clf, train_epoch: Callable[[Any, int], None], eval_ref: Callable[[Any], float],
               eval_val: Callable[[Any], Tuple[float, float]], nbr_epochs: int, early_stopping_patience: Optional[int] = None,
               on_epoch_end: Optional[Callable[[Dict[str, Any]], None]] = None, class_scores: bool = False
               ) -> Tuple[Any, Dict[str, Any]]:
    """Run up to ``nbr_epochs`` epochs of ``train_epoch(clf, epoch)``, each followed by ``eval_ref(clf) -> accuracy`` and
    ``eval_val(clf) -> (accuracy, log_loss)``.  -> ``(clf, info)``.

    With ``early_stopping_patience`` set, an epoch whose validation loss is strictly below every earlier one becomes the best
    epoch and ``copy.deepcopy(clf)`` is kept (a tie or a NaN is no improvement); the loop stops once ``patience`` epochs in a row
    brought none; and whenever the best epoch is not the last one run -- after an early stop or a used-up budget alike -- the
    snapshot is what is returned.  With ``None`` no snapshot is ever taken and the classifier of the last epoch is returned.

    ``on_epoch_end`` gets a dict per epoch: ``epoch`` (0-based), ``ref_accuracy``, ``val_accuracy``, ``val_loss``,
    ``training_loss`` (``clf.loss_curve_[-1]``, or None), ``cumulative_seconds``; on the last epoch run also ``final_epoch``
    (1-based), ``early_stopped`` and, when a best epoch exists, ``best_val_epoch`` (1-based) / ``best_val_loss``.

    With ``class_scores=True``, ``eval_val(clf)`` returns ``(accuracy, log_loss, ClassScores)`` (``calibration.evaluate_classes``)
    and the dict gains ``val_balanced_accuracy`` and ``val_f1_macro`` -- the metrics the balancing study ranks by, which move
    differently from accuracy over the epochs (docs/research/balancing-experiments.md:67, 82).  Early stopping still reads
    ``val_loss`` alone: everything else in the dict and everything returned is what ``class_scores=False`` gives.

    ``info``: ``enabled``, ``patience``, ``stop_reason`` ("early_stopping" or "budget_exhausted"), ``final_epoch``,
    ``best_val_epoch``, ``best_val_loss`` (None without a best epoch) -- the reference's ``_early_stop_info``."""
    state = EarlyStopping(nbr_epochs, early_stopping_patience)
    for epoch in range(int(nbr_epochs)):
        train_epoch(clf, epoch)
        ref_acc = eval_ref(clf)
        val_acc, val_loss, extra = _val_entries(eval_val(clf), class_scores)
        metrics = state.epoch_done(clf, epoch, ref_acc, val_acc, val_loss, extra=extra)
        if on_epoch_end is not None:
            on_epoch_end(metrics)
        if state.stopped:
            break
    return state.result(clf)


def _val_entries(result, class_scores: bool) -> Tuple[float, float, Optional[Dict[str, float]]]:
    """``eval_val``'s return value -> (accuracy, log_loss, the extra callback entries or None)."""
    if not class_scores:
        val_acc, val_loss = result
        return val_acc, val_loss, None
    val_acc, val_loss, scores = result
    return val_acc, val_loss, {"val_balanced_accuracy": scores.balanced_accuracy, "val_f1_macro": scores.f1_macro}


def _contiguous_batches(n_rows: int, batch_size: int) -> Callable[[int], Iterable[np.ndarray]]:
    def batches(epoch: int):
        for start in range(0, n_rows, batch_size):
            yield np.arange(start, min(start + batch_size, n_rows), dtype=np.int64)
    return batches


def _fill_schedule_steps(clf, batches, nbr_epochs: int) -> None:
    """A decaying ``lr_schedule`` whose ``schedule_steps`` is None ends with the budget: ``nbr_epochs`` x the Adam steps of the
    classifier's own epoch, counted on ``batches(0)`` (``optim.steps_per_epoch``).  Anything else is left alone."""
    if getattr(clf, "lr_schedule", "constant") == "constant" or getattr(clf, "schedule_steps", None) is not None:
        return
    from .optim import steps_per_epoch
    clf.schedule_steps = int(nbr_epochs) * steps_per_epoch(batches(0), clf.batch_size)


def _check_splits(train, ref, val, batch_size) -> None:
    if int(batch_size) < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size!r}")
    for name, fs in (("train", train), ("ref", ref), ("val", val)):
        if not isinstance(fs, FeatureSet):
            raise ValueError(f"{name} must be a FeatureSet, got {type(fs).__name__}")
        if not np.array_equal(fs.classes, ref.classes) or fs.dim != ref.dim:
            raise ValueError(f"the {name} set's classes / width differ from the ref set's")
        if len(fs) < 1:
            raise ValueError(f"the {name} set is empty")


def train_classifier(train: FeatureSet, ref: FeatureSet, val: FeatureSet, nbr_epochs: int, *, batch_size: int,
                     class_weight: Optional[dict] = None, early_stopping_patience: Optional[int] = None,
                     on_epoch_end: Optional[Callable[[Dict[str, Any]], None]] = None,
                     batches: Optional[Callable[[int], Iterable[np.ndarray]]] = None,
                     clf: Optional[TorchMLPClassifier] = None, class_scores: bool = False, transform=None, logit_scaling=None,
                     row_weight=None, row_group=None, targets=None, teacher=None) -> Tuple[CalibratedMLP, Dict[str, Any], List[float]]:
    """Train, early-stop and calibrate the MLP head on three resident splits.  -> ``(calibrated, info, ref_accs)``:
    the ``CalibratedMLP`` of the returned classifier on ``ref``, ``epoch_loop``'s ``info``, and the ref accuracy after every
    epoch run (the reference's ``TrainClassifierReturnMsg.ref_accs``).

    ``clf`` defaults to the production head (trainer.py:118-123): hidden layers (500, 300, 100), ``learning_rate_init=1e-4``,
    ``random_state=0``, with ``class_weight``; a classifier passed in keeps its own ``class_weight``.  The three sets must share
    one class list, which is what the first ``partial_fit_rows`` is given.

    Each epoch makes one ``partial_fit_rows(train, rows)`` call per array that ``batches(epoch)`` yields -- one array stands for
    one batch of ``labels.train.load_data_in_batches(batch_size, random_seed=epoch)`` (:141-145).  The default is contiguous
    slices of ``batch_size`` rows in stored order, the same every epoch.  pyspacer's shuffle of the images behind that loader is
    not reproduced here; ``batches`` is the hook for it (any callable ``epoch -> iterable of row-index arrays``).  Within a batch
    the classifier shuffles as ``partial_fit`` does.

    ``class_scores=True`` scores ``val`` through ``calibration.evaluate_classes`` instead of ``evaluate``: the ``on_epoch_end``
    dict gains ``val_balanced_accuracy`` and ``val_f1_macro`` (see ``epoch_loop``); nothing returned changes.

    ``transform``: a fitted ``FeatureTransform`` or a dict of ``FeatureTransform.fit`` keyword arguments (fitted on ``train``).  The
    three splits are transformed on the device into resident sets of their own, the head is trained and calibrated on those, they
    are freed, and the model returned is ``CalibratedMLP.folded(transform)``: it takes RAW features (``n_features_in_ ==
    train.dim``) and carries the transform as ``transform_``.  ``None`` is the path described above, call for call.

    ``logit_scaling``: a kind string (``"temperature"`` / ``"bias"`` / ``"vector"``) or a fitted ``LogitScaling``.  After the epoch loop
    and the best-snapshot restore the scaling is fitted on ``ref`` (``logit_scaling.fit_logit_scaling``) and folded into the last
    layer, and ``calibrate`` runs on the folded classifier; the model carries it as ``logit_scaling_``.  Early stopping and the
    per-epoch evaluation keep reading raw logits.

    A ``clf`` with a decaying ``lr_schedule`` and ``schedule_steps=None`` gets ``nbr_epochs`` x its steps per epoch (counted on
    ``batches(0)``); one with ``ema_decay > 0`` is evaluated, early-stopped, scaled and calibrated on its averaged weights.  With ``transform=`` the scaling goes into the last layer and the transform into the
    first -- on a head with no hidden layer the scaling first, then the transform.  ``None`` changes no call.

    ``row_weight`` / ``row_group``: arrays indexed by row of ``train``, handed to every epoch's ``partial_fit_rows`` (a weight per row;
    group DRO over the rows' groups, on a ``clf`` with ``n_groups``).  ``None`` changes no call.

    ``targets`` (a ``TargetSet`` aligned with ``train``) or ``teacher`` (a ``HeadEnsemble``, ``CalibratedMLP`` or ``Predictor``, whose
    targets are made for ``train`` and freed at the end), one or the other: every epoch's ``partial_fit_rows`` gets the targets, on a
    ``clf`` with ``distill_alpha > 0`` (``distill.distill`` builds one).  With ``transform=`` a teacher scores the RAW train split,
    before it is transformed; ``FeatureTransform.apply`` keeps the row order, so the rows still align.  ``None`` changes no call."""
    _check_splits(train, ref, val, batch_size)
    if logit_scaling is not None:
        _ls.check_argument(logit_scaling)
    if teacher is not None:   # made for the train split as given (raw, when there is a transform), freed when the training ends
        targets = resolve_targets(targets, teacher, train)
        try:
            return train_classifier(train, ref, val, nbr_epochs, batch_size=batch_size, class_weight=class_weight,
                                    early_stopping_patience=early_stopping_patience, on_epoch_end=on_epoch_end, batches=batches,
                                    clf=clf, class_scores=class_scores, transform=transform, logit_scaling=logit_scaling,
                                    row_weight=row_weight, row_group=row_group, targets=targets)
        finally:
            targets.close()
    if transform is not None:
        ft = _ft.resolve(transform, train)
        sets = []
        try:
            for fs in (train, ref, val):
                sets.append(ft.apply(fs))
            cal, info, accs = train_classifier(*sets, nbr_epochs, batch_size=batch_size, class_weight=class_weight,
                                               early_stopping_patience=early_stopping_patience, on_epoch_end=on_epoch_end,
                                               batches=batches, clf=clf, class_scores=class_scores, logit_scaling=logit_scaling,
                                               row_weight=row_weight, row_group=row_group, targets=targets)
        finally:
            for fs in sets:
                fs.close()
        return cal.folded(ft), info, accs
    if clf is None:
        clf = TorchMLPClassifier(hidden_layer_sizes=(500, 300, 100), learning_rate_init=1e-4, class_weight=class_weight,
                                 random_state=0, device=ref.device)
    elif class_weight is not None:
        raise ValueError("pass class_weight either here or on clf, not both")
    classes = ref.classes.tolist()
    if batches is None:
        batches = _contiguous_batches(len(train), int(batch_size))
    _fill_schedule_steps(clf, batches, nbr_epochs)
    ref_accs: List[float] = []

    def train_epoch(c, epoch):
        for rows in batches(epoch):
            if targets is not None:
                c.partial_fit_rows(train, rows, classes=classes, row_weight=row_weight, row_group=row_group, targets=targets)
            elif row_weight is None and row_group is None:
                c.partial_fit_rows(train, rows, classes=classes)
            else:
                c.partial_fit_rows(train, rows, classes=classes, row_weight=row_weight, row_group=row_group)

    def eval_ref(c):
        ref_accs.append(evaluate(c, ref)[0])
        return ref_accs[-1]

    eval_val = evaluate_classes if class_scores else evaluate
    clf, info = epoch_loop(clf, train_epoch, eval_ref, lambda c: eval_val(c, val), nbr_epochs,
                           early_stopping_patience=early_stopping_patience, on_epoch_end=on_epoch_end, class_scores=class_scores)
    if logit_scaling is None:
        return calibrate(clf, ref), info, ref_accs
    return calibrate(clf, ref, logit_scaling=logit_scaling), info, ref_accs


def train_and_validate(train: FeatureSet, ref: FeatureSet, val: FeatureSet, nbr_epochs: int, *, batch_size: int,
                       pc_models: Sequence[Any] = (), **kwargs):
    """``MermaidTrainer.__call__`` to its end (trainer.py:83-293) on three resident splits.  -> ``(calibrated, val_results,
    return_msg)``: ``train_classifier``'s ``CalibratedMLP`` (which takes ``kwargs``), the ``ValResults`` of that model on ``val``
    (``Validation.val_results``) and a ``TrainClassifierReturnMsg`` with ``acc`` (the validation accuracy), ``pc_accs`` (the
    accuracy of every model in ``pc_models`` -- ``Predictor`` or ``CalibratedMLP`` -- on ``val``), ``ref_accs`` (one entry per
    epoch run) and ``runtime`` in seconds.  pyspacer's message classes are used when importable, ``spacer_shim``'s otherwise.
    The validation rows are scored where they lie (``validation.validate``) -- with ``transform=`` in ``kwargs`` too: the folded
    model takes the raw ``val`` rows."""
    t0 = time.time()
    calibrated, _info, ref_accs = train_classifier(train, ref, val, nbr_epochs, batch_size=batch_size, **kwargs)
    scored = validate(calibrated, val)
    pc_accs = previous_accuracies(pc_models, val)
    try:
        from spacer.messages import TrainClassifierReturnMsg  # type: ignore
    except ImportError:
        from .spacer_shim import TrainClassifierReturnMsg
    msg = TrainClassifierReturnMsg(acc=scored.accuracy, pc_accs=pc_accs, ref_accs=ref_accs, runtime=time.time() - t0)
    return calibrated, scored.val_results(), msg
