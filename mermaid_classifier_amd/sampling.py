"""The balancing strategies of the reference's training package, as the inputs of a ``SweepConfig``.

=============================================================  ==========================================================
reference                                                      here
=============================================================  ==========================================================
``compute_class_weights`` (``mermaid_classifier/training/      ``effective_number_weights(counts, beta, weight_ratio_cap)``
sample_weighting/effective_number.py:38-75``)                  -> ``SweepConfig.class_weight``
(none: Menon et al. 2021, logit adjustment)                    ``logit_adjustment(counts, tau)`` -> ``SweepConfig.logit_prior``
``compute_per_class_targets`` (``training/subsample/           ``subsample_targets(counts, strategy, total_annotations,
registry.py:53-181``): ``stratified``, ``balanced``            min_per_class)``
``TrainingDataset._apply_subsample`` (``training/              ``subsample_rows(labels, targets, order)``: the first
dataset.py:222-347``; ``_rn <= target_n``, :292-310)           ``target`` rows of each class in primary-key order
one epoch's batches over the kept rows                         ``row_batches(rows, batch_size)`` -> ``SweepConfig.batches``
(none: Zhang et al. 2018, mixup)                               ``mixup_plan(visit, batch_size, alpha, rng)`` -> the plan of
                                                               ``mmc_trainer_partial_fit_set_mixed``
(none: "per-source rebalancing",                               ``group_balance_weights(groups, labels)`` ->
docs/research/balancing-experiments.md:141)                    ``partial_fit_rows(row_weight=)`` / ``SweepConfig.row_weight``
=============================================================  ==========================================================

A balancing configuration of ``docs/research/balancing-experiments.md`` is a class-weight dict, a subsample, or both, over one
train split.  These functions run once per configuration on the host, on the labels alone (``class_counts`` reads a
``FeatureSet``'s labels back, never its rows): there is no hot path here and no kernel.  The rows of a subsample are then visited
where they lie on the device (``TorchMLPClassifier.partial_fit_rows``)."""

from __future__ import annotations

from typing import Any, Callable, Dict, Iterable, Mapping, Optional

import numpy as np

from .featureset import FeatureSet

__all__ = ["class_counts", "effective_number_weights", "logit_adjustment", "subsample_targets", "subsample_rows", "row_batches", "mixup_plan", "group_balance_weights", "STRATEGIES"]

STRATEGIES = ("stratified", "balanced")


def _label_indices(labels_or_featureset) -> np.ndarray:
    if isinstance(labels_or_featureset, FeatureSet):
        from .backbone import _current_stream_ptr
        from .validation import _set_labels
        fs = labels_or_featureset
        n = len(fs)
        return _set_labels(fs, 0, n, None, _current_stream_ptr(fs.device_index)) if n else np.zeros(0, np.int32)
    y = np.asarray(labels_or_featureset)
    if y.ndim != 1 or not (y.dtype.kind in "iu" or y.size == 0):
        raise ValueError(f"labels must be a 1-D array of class indices, got {y.dtype} {y.shape}")
    return y


def class_counts(labels_or_featureset, n_classes: Optional[int] = None) -> np.ndarray:
    """-> int64 ``counts[k]`` = rows of class index ``k``.  ``labels_or_featureset`` is a 1-D array of class indices in
    ``[0, n_classes)`` or a ``FeatureSet`` (whose labels alone are read back; ``n_classes`` defaults to its class count)."""
    if n_classes is None:
        if not isinstance(labels_or_featureset, FeatureSet):
            raise ValueError("n_classes is required for a label array")
        n_classes = len(labels_or_featureset.classes)
    if int(n_classes) != n_classes or n_classes < 1:
        raise ValueError(f"n_classes must be a positive integer, got {n_classes!r}")
    y = _label_indices(labels_or_featureset)
    if y.size and (int(y.min()) < 0 or int(y.max()) >= n_classes):
        raise ValueError(f"labels outside [0, {n_classes})")
    return np.bincount(y.astype(np.int64), minlength=int(n_classes)).astype(np.int64)


def effective_number_weights(counts: Mapping[Any, int], beta: float = 0.9999, weight_ratio_cap: Optional[float] = None) -> Dict[Any, float]:
    """Effective-number-of-samples class weights (Cui et al. 2019), ``compute_class_weights`` with the switch on
    (effective_number.py:38-75): ``w = 1 / max((1 - beta**n) / (1 - beta), 1e-12)`` with ``n = max(count, 1)``; with
    ``weight_ratio_cap`` (>= 1) and at least two classes, weights above ``min(w) * cap`` are lowered to it.  An empty input gives
    ``{}``.  The reference fixes ``beta`` at 0.9999 (``BETA``)."""
    if not 0.0 <= beta < 1.0:
        raise ValueError(f"beta must lie in [0, 1), got {beta!r}")
    if weight_ratio_cap is not None and weight_ratio_cap < 1.0:
        raise ValueError(f"weight_ratio_cap must be None or >= 1.0, got {weight_ratio_cap!r}")
    if not counts:
        return {}
    weights: Dict[Any, float] = {}
    for label, count in counts.items():
        n = max(int(count), 1)
        effective_n = (1.0 - beta**n) / (1.0 - beta)
        weights[label] = 1.0 / max(effective_n, 1e-12)
    if weight_ratio_cap is not None and len(weights) >= 2:
        ceiling = min(weights.values()) * weight_ratio_cap
        for label, weight in weights.items():
            if weight > ceiling:
                weights[label] = ceiling
    return weights


def logit_adjustment(counts: Mapping[Any, int], tau: float = 1.0) -> Dict[Any, float]:
    """The per-class offsets of the logit-adjusted loss (Menon et al. 2021): ``tau * log(n_c / N)`` with ``N`` the sum of the
    counts -- ``SweepConfig.logit_prior`` / ``TorchMLPClassifier(logit_prior=)``, added to the logits inside the training loss only.
    Takes the ``counts`` mapping of ``effective_number_weights``; no counterpart in the reference.  ``ValueError``: an empty mapping,
    a count below 1 (its logarithm is not finite), a ``tau`` that is not finite."""
    if not counts:
        raise ValueError("counts is empty")
    if not np.isfinite(tau):
        raise ValueError(f"tau must be finite, got {tau!r}")
    for label, count in counts.items():
        if int(count) != count or count < 1:
            raise ValueError(f"count for {label!r} must be an integer >= 1, got {count!r}")
    total = sum(int(c) for c in counts.values())
    return {label: float(tau) * float(np.log(int(count) / total)) for label, count in counts.items()}


def subsample_targets(counts: Mapping[Any, int], strategy: str, total_annotations: int, min_per_class: int = 0) -> Dict[Any, int]:
    """Per-class row targets, ``compute_per_class_targets`` (registry.py:53-181).

    ``"stratified"``: ``round(total_annotations * n_c / N)`` (Python's ``round``: half to even), capped at ``n_c`` and floored at
    ``min_per_class``; a sum above ``total_annotations`` is trimmed from the classes in the order ``(-count, key)``, never below
    the floor, and an undershoot is left as it is.  ``"balanced"``: ``total_annotations // number of classes``, capped and floored
    the same way.  (The floor is not capped at ``n_c``, as in the reference: ``subsample_rows`` rejects a target a class cannot
    fill.)  Empty ``counts`` give ``{}``.  ``ValueError``: another strategy, ``total_annotations`` not a positive integer,
    a negative ``min_per_class`` (the reference's ``SubsampleOptions``)."""
    if strategy not in STRATEGIES:
        raise ValueError(f"strategy must be one of {STRATEGIES}, got {strategy!r}")
    if isinstance(total_annotations, bool) or total_annotations is None or int(total_annotations) != total_annotations or total_annotations <= 0:
        raise ValueError(f"total_annotations must be an integer > 0, got {total_annotations!r}")
    if int(min_per_class) != min_per_class or min_per_class < 0:
        raise ValueError(f"min_per_class must be an integer >= 0, got {min_per_class!r}")
    total, floor = int(total_annotations), int(min_per_class)
    counts = {k: int(v) for k, v in counts.items()}
    if not counts:
        return {}
    if strategy == "balanced":
        per = total // len(counts)
        return {k: max(floor, min(n, per)) for k, n in counts.items()}
    grand_total = sum(counts.values())
    if grand_total == 0:
        return dict.fromkeys(counts, 0)
    targets = {k: max(floor, min(n, round(total * n / grand_total))) for k, n in counts.items()}
    overshoot = sum(targets.values()) - total
    if overshoot <= 0:
        return targets
    for k in sorted(targets, key=lambda k: (-counts[k], k)):
        if overshoot == 0:
            break
        delta = min(max(0, targets[k] - floor), overshoot)
        targets[k] -= delta
        overshoot -= delta
    return targets


def subsample_rows(labels, targets_by_class_index: Mapping[int, int], order=None) -> np.ndarray:
    """-> the sorted int64 indices of the rows a subsample keeps: for every class index in ``targets_by_class_index`` the first
    ``target`` rows of that class in ``order`` -- the ``_rn <= target_n`` of dataset.py:292-310, whose ``ROW_NUMBER()`` runs over
    the primary-key order within a class.  ``labels`` are class indices (array or ``FeatureSet``); ``order`` is a permutation of
    the row indices standing for the primary-key order (``order[0]`` is the first row), ``None`` the stored order.  A class
    without a target is dropped (the inner join of :300-310); a target above the class's row count is a ``ValueError``.
    Rows are rows: in a set built from ``extract_images(..., views=...)`` every annotation has G of them (its views), and a
    subsample counts and keeps views, not annotations.  The views of one annotation must stay in one split."""
    y = _label_indices(labels).astype(np.int64)
    n = len(y)
    if order is None:
        seq = np.arange(n, dtype=np.int64)
    else:
        seq = np.asarray(order)
        if seq.shape != (n,) or not (seq.dtype.kind in "iu" or n == 0) or not np.array_equal(np.sort(seq), np.arange(n)):
            raise ValueError(f"order must be a permutation of the {n} row indices")
        seq = seq.astype(np.int64)
    K = int(y.max()) + 1 if n else 0
    target = np.zeros(K, np.int64)
    counts = np.bincount(y, minlength=K) if n else np.zeros(0, np.int64)
    for k, t in targets_by_class_index.items():
        if int(k) != k or int(t) != t or t < 0 or k < 0:
            raise ValueError(f"targets must map class indices to counts >= 0; got {k!r}: {t!r}")
        have = int(counts[k]) if k < K else 0
        if t > have:
            raise ValueError(f"class {k}: target {t} above its {have} rows (no oversampling)")
        if k < K:
            target[k] = t
    if n == 0:
        return np.zeros(0, np.int64)
    lab = y[seq]
    by_class = np.argsort(lab, kind="stable")                       # positions of seq, class by class, each in `order`
    start = np.concatenate([[0], np.cumsum(counts)])[:-1]
    rank = np.arange(n) - start[lab[by_class]]                      # 0-based ROW_NUMBER() within the class
    return np.sort(seq[by_class[rank < target[lab[by_class]]]])


def row_batches(rows, batch_size: int) -> Callable[[int], Iterable[np.ndarray]]:
    """-> the ``batches`` hook of ``train_classifier`` / ``SweepConfig`` over a fixed row subset: a callable ``epoch -> iterable``
    of contiguous slices of ``rows``, ``batch_size`` rows each (the last one shorter), the same every epoch -- what the default
    hook does over a whole set."""
    rows = np.ascontiguousarray(np.asarray(rows), dtype=np.int64) if np.size(rows) else np.zeros(0, np.int64)
    if rows.ndim != 1:
        raise ValueError(f"rows must be 1-D, got shape {rows.shape}")
    if int(batch_size) != batch_size or batch_size < 1:
        raise ValueError(f"batch_size must be an integer >= 1, got {batch_size!r}")
    size = int(batch_size)

    def batches(epoch: int):
        for first in range(0, len(rows), size):
            yield rows[first:first + size]
    return batches


def mixup_plan(visit, batch_size: int, alpha: float, rng: np.random.Generator):
    """The mixing plan of one pass over the rows ``visit`` (row indices of a ``FeatureSet`` in visiting order) in mini-batches of
    ``batch_size``: -> ``(partner, lam)``.  ``partner`` (int64, one per position) is, within each mini-batch, a permutation of that
    mini-batch's visited rows, so a row is mixed with a row of its own mini-batch (Zhang et al. 2018 mix a batch with a shuffle of
    itself); ``lam`` (float32, one per mini-batch) is drawn from Beta(alpha, alpha).  Both come from ``rng`` alone."""
    visit = np.ascontiguousarray(np.asarray(visit, dtype=np.int64))
    if visit.ndim != 1 or visit.size < 1:
        raise ValueError(f"visit must be a non-empty 1D array of row indices, got shape {visit.shape}")
    if int(batch_size) < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size!r}")
    if not (float(alpha) > 0.0 and np.isfinite(float(alpha))):
        raise ValueError(f"alpha must be a finite number > 0, got {alpha!r}")
    n = int(visit.size)
    mb = min(int(batch_size), n)
    steps = -(-n // mb)
    partner = np.empty(n, dtype=np.int64)
    lam = np.empty(steps, dtype=np.float32)
    for s in range(steps):
        rows = visit[s * mb:(s + 1) * mb]
        partner[s * mb:s * mb + rows.size] = rows[rng.permutation(rows.size)]
        lam[s] = np.float32(rng.beta(float(alpha), float(alpha)))
    return partner, lam


def group_balance_weights(groups, labels=None) -> np.ndarray:
    """Static per-source rebalancing as row weights: ``r_i`` proportional to ``1 / n_group(i)``, the number of the given rows in row
    i's group -- or, with ``labels``, to ``1 / n_(group, class)(i)`` -- scaled so that the mean over the rows given is 1.  Every
    group (every group x class cell that occurs) then carries the same total weight.  -> float32, one weight per row: the
    ``row_weight`` of ``TorchMLPClassifier.partial_fit_rows`` when ``groups`` covers the rows of the set.

    ``groups`` (and ``labels``) are 1D and of one length; the values are only compared for equality."""
    g = np.asarray(groups)
    if g.ndim != 1 or g.size == 0:
        raise ValueError(f"groups must be a non-empty 1D array, got shape {g.shape}")
    _, cell = np.unique(g, return_inverse=True)
    if labels is not None:
        y = np.asarray(labels)
        if y.shape != g.shape:
            raise ValueError(f"labels has shape {y.shape}, groups {g.shape}")
        _, yi = np.unique(y, return_inverse=True)
        _, cell = np.unique(cell.astype(np.int64) * (int(yi.max()) + 1) + yi, return_inverse=True)
    counts = np.bincount(cell)
    w = 1.0 / counts[cell].astype(np.float64)
    return (w * (g.size / w.sum())).astype(np.float32)
