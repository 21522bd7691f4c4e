"""Score a validation split with a calibrated head on the MI355X: what ``MermaidTrainer.__call__`` computes after the calibration
(``mermaid_classifier/pyspacer/trainer.py:267-293``) and the per-row reductions of the reference's metrics.

=====================================================  ===================================================================
reference                                              here
=====================================================  ===================================================================
``evaluate_classifier(clf_calibrated, labels.val)``    ``validate(model, data)`` -> ``Validation`` (``est``, ``scores``, ``gt``)
``ValResults(scores, gt, est, classes)`` (:279-284)    ``Validation.val_results()``
``accuracy_score(val_gts, val_ests)`` (:287)           ``Validation.accuracy``
the previous models' accuracies (:273-277)             ``previous_accuracies(pc_models, val)``
``_compute_topk_mrr`` (metrics/ranking.py:42-65)       ``Validation.topk_accuracy(k)``, ``Validation.mrr`` (from ``rank_hist``)
per-sample log-loss (metrics/probability.py:43-49)     ``Validation.log_loss`` (from ``nll_q32``), ``Validation.p_true``
``compute_precision_recall_f1`` and                    ``Validation.class_scores()`` (``class_scores.ClassScores`` of
``compute_balanced_accuracy_mcc``                      ``confusion``)
(metrics/classification.py:171-302)
=====================================================  ===================================================================

The reference builds the N x K probability matrix on the host (``metrics/coordinator.py:59-76``) and reduces it to one rank and
one probability per row.  Here ``calibrate_eval_kernel`` (``mmc_head_evaluate`` / ``mmc_head_evaluate_set``) ends every row in its
label, its score, the rank and the probability of its true class and adds the totals as integers: the matrix is never written, and
16 bytes per row plus the integer tables come back.  A ``FeatureSet`` is read where it lies on the device.

Equal probabilities rank in class order (the rule of ``Predictor.predict_topk``); the reference's ``np.argsort(-proba)`` leaves
that order undefined.  No CPU fallback."""

from __future__ import annotations

import ctypes as C
from typing import Any, List, Optional, Sequence

import numpy as np

from . import _lib
from .backbone import _current_stream_ptr
from .calibration import CalibratedMLP, _batches
from .class_scores import ClassScores
from .featureset import FeatureSet
from .inference import Predictor

__all__ = ["Validation", "validate", "previous_accuracies", "label_map"]

MAX_ROWS_PER_CALL = 59000000   # include/mmc.h MMC_EVALUATE_SET_MAX_ROWS


def label_map(model_classes: Sequence[Any], data_classes: Sequence[Any]) -> np.ndarray:
    """-> int32 ``m`` with ``m[j]`` the position of ``data_classes[j]`` in ``model_classes``, or -1 for a class the model lacks."""
    where = {c: i for i, c in enumerate(np.asarray(model_classes).tolist())}
    if len(where) != len(model_classes):
        raise ValueError("the model's class list holds duplicates")
    return np.asarray([where.get(c, -1) for c in np.asarray(data_classes).tolist()], dtype=np.int32)


class Validation:
    """The outcome of ``validate``.  Per row (``None`` when ``validate(..., rows=False)``): ``gt`` / ``est`` (indices into
    ``classes``; ``gt`` is -1 for a class the model lacks), ``scores`` (float64, the probability of ``est``), ``ranks`` (1-based
    rank of the true class, 0 for an unknown one), ``p_true`` (float32, its probability).  Totals, exact integers: ``n``,
    ``n_correct``, ``n_unknown``, ``n_nonfinite`` (rows whose probabilities hold a NaN: kept out of everything below),
    ``confusion[gt, est]``, ``rank_hist[rank - 1]`` and ``nll_q32`` = sum of round(-log(clip(p_true, 1e-15, 1)) * 2^32)."""

    def __init__(self, classes, gt, est, scores, ranks, p_true, confusion, rank_hist, n, n_correct, n_unknown, n_nonfinite, nll_q32):
        self.classes = np.asarray(classes).tolist()
        K = len(self.classes)
        rows = (gt, est, scores, ranks, p_true)
        if any(v is None for v in rows) and not all(v is None for v in rows):
            raise ValueError("per-row values must be given all or none")
        self.gt = None if gt is None else np.asarray(gt, dtype=np.int32)
        self.est = None if est is None else np.asarray(est, dtype=np.int32)
        self.scores = None if scores is None else np.asarray(scores, dtype=np.float64)
        self.ranks = None if ranks is None else np.asarray(ranks, dtype=np.int32)
        self.p_true = None if p_true is None else np.asarray(p_true, dtype=np.float32)
        self.confusion = np.asarray(confusion, dtype=np.int64)
        self.rank_hist = np.asarray(rank_hist, dtype=np.int64)
        self.n, self.n_correct, self.n_unknown = int(n), int(n_correct), int(n_unknown)
        self.n_nonfinite, self.nll_q32 = int(n_nonfinite), int(nll_q32)
        if self.confusion.shape != (K, K) or self.rank_hist.shape != (K,):
            raise ValueError(f"confusion {self.confusion.shape} / rank_hist {self.rank_hist.shape} do not fit {K} classes")
        if self.gt is not None and any(v.shape != (self.n,) for v in (self.gt, self.est, self.scores, self.ranks, self.p_true)):
            raise ValueError(f"per-row values must have shape ({self.n},)")

    @property
    def has_rows(self) -> bool:
        return self.gt is not None

    @property
    def n_scored(self) -> int:
        """Rows that entered ``confusion``, ``rank_hist`` and the loss sum."""
        return self.n - self.n_unknown - self.n_nonfinite

    @property
    def accuracy(self) -> float:
        """``n_correct / n``: a row of a class the model lacks counts as wrong, as the reference's comparison of label strings
        counts it."""
        return self.n_correct / self.n if self.n else float("nan")

    @property
    def log_loss(self) -> float:
        """Mean of -log(clip(p_true, 1e-15, 1)) over the scored rows (probability.py:49): one int / int division."""
        return self.nll_q32 / (self.n_scored << 32) if self.n_scored else float("nan")

    def topk_accuracy(self, k: int) -> float:
        """``np.mean(ranks <= k)`` (ranking.py:63) from the histogram; rows outside it (unknown, non-finite) count as misses."""
        if int(k) != k or k < 1:
            raise ValueError(f"k must be an integer >= 1; got {k!r}")
        return int(self.rank_hist[: int(k)].sum()) / self.n if self.n else float("nan")

    @property
    def mrr(self) -> float:
        """``np.mean(1 / ranks)`` (ranking.py:64) from the histogram."""
        if not self.n:
            return float("nan")
        return float((self.rank_hist / np.arange(1, len(self.rank_hist) + 1, dtype=np.float64)).sum() / self.n)

    def class_scores(self) -> ClassScores:
        """-> ``ClassScores(self.confusion, self.classes)``: per-class precision / recall / f1, the macro averages, balanced accuracy
        and MCC of the scored rows (``compute_precision_recall_f1`` and ``compute_balanced_accuracy_mcc``,
        metrics/classification.py:171-302)."""
        return ClassScores(self.confusion, self.classes)

    def merge(self, other: "Validation") -> "Validation":
        """The validation of this one's rows followed by ``other``'s: integer adds and row concatenation."""
        if self.classes != other.classes:
            raise ValueError("merge: the class lists differ")
        if self.has_rows != other.has_rows:
            raise ValueError("merge: one side has per-row values, the other has none")
        cat = (lambda a, b: np.concatenate([a, b])) if self.has_rows else (lambda a, b: None)
        return Validation(self.classes, cat(self.gt, other.gt), cat(self.est, other.est), cat(self.scores, other.scores),
                          cat(self.ranks, other.ranks), cat(self.p_true, other.p_true), self.confusion + other.confusion,
                          self.rank_hist + other.rank_hist, self.n + other.n, self.n_correct + other.n_correct,
                          self.n_unknown + other.n_unknown, self.n_nonfinite + other.n_nonfinite, self.nll_q32 + other.nll_q32)

    def val_results(self):
        """-> ``ValResults(scores, gt, est, classes)`` of plain Python lists (trainer.py:279-284): pyspacer's class when it is
        importable, ``spacer_shim.ValResults`` otherwise."""
        if not self.has_rows:
            raise ValueError("val_results needs the per-row values: validate(..., rows=True)")
        if self.n_unknown:
            raise ValueError(f"{self.n_unknown} rows carry a class the model lacks: ValResults indexes gt into the model's classes "
                             "(the reference's classes.index raises there too)")
        try:
            from spacer.data_classes import ValResults  # type: ignore
        except ImportError:
            from .spacer_shim import ValResults
        return ValResults(scores=self.scores.tolist(), gt=self.gt.tolist(), est=self.est.tolist(), classes=list(self.classes))


def _model_parts(model):
    """-> (DeviceHead or None until needed, class list, input width)."""
    if isinstance(model, CalibratedMLP):
        return model._device_head, model.classes_.tolist(), model.n_features_in_
    if isinstance(model, Predictor):
        return (lambda: model._head), list(model.classes), int(model.input_dim)
    raise ValueError(f"model must be a CalibratedMLP or a Predictor, got {type(model).__name__}")


def _host_labels(classes: List[Any], y, n: int, strict: bool):
    """Host labels -> (y int32, map or None): indices into the model's classes; when some label is unknown to the model (and that is
    allowed) indices into the K + 1 entry map [0 .. K-1, -1]."""
    y = np.asarray(y)
    if y.shape != (n,):
        raise ValueError(f"y has shape {y.shape}, expected ({n},)")
    uniq, inv = np.unique(y, return_inverse=True)
    idx = label_map(classes, uniq)[inv.reshape(-1)] if n else np.zeros(0, np.int32)
    if np.all(idx >= 0):
        return np.ascontiguousarray(idx, dtype=np.int32), None
    if strict:
        bad = sorted(set(uniq[label_map(classes, uniq) < 0].tolist()))
        raise ValueError(f"Labels {bad} are not in the model's classes {classes}.")
    K = len(classes)
    return (np.ascontiguousarray(np.where(idx < 0, K, idx), dtype=np.int32),
            np.ascontiguousarray(np.append(np.arange(K, dtype=np.int32), np.int32(-1))))


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data


def _prepare(model, data, rows, strict: bool, who: str, one_pair: bool = False):
    """What ``validate`` and ``grouped_validate`` do before the device is touched -> (head getter, classes, sources).  ``sources`` is
    ``[(FeatureSet, None, map)]`` or the non-empty host batches ``[(X float32, y int32, map), ...]``, every one checked; ``map`` is the
    label map of that source, or None when its labels index the model's classes."""
    if not isinstance(rows, bool):
        raise ValueError(f"rows must be True or False, got {rows!r}")
    get_head, classes, dim = _model_parts(model)
    if isinstance(data, FeatureSet):
        if data.dim != dim:
            raise ValueError(f"the feature set has {data.dim} features, expected {dim}")
        if len(data) == 0:
            raise ValueError(f"{who}: no rows")
        same = data.classes.tolist() == classes
        return get_head, classes, [(data, None, None if same else np.ascontiguousarray(label_map(classes, data.classes)))]
    if one_pair and not (isinstance(data, (tuple, list)) and len(data) == 2):
        raise ValueError("data must be a FeatureSet or one (X, y) pair")
    sources = []
    for x, y in ([(data[0], data[1])] if one_pair else _batches(data)):
        X = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
        if X.ndim != 2:
            raise ValueError(f"X must be 2D, got shape {X.shape}")
        if X.shape[1] != dim:
            raise ValueError(f"X has {X.shape[1]} features, expected {dim}")
        yi, lmap = _host_labels(classes, y, X.shape[0], strict)
        if X.shape[0]:
            sources.append((X, yi, lmap))
    if not sources:
        raise ValueError(f"{who}: no rows")
    return get_head, classes, sources


class _Call:
    """One ``mmc_head_evaluate*`` call's host outputs: ``args`` are its (est, score, rank, p_true, totals, confusion, rank_hist)
    arguments; ``gt`` is set by the caller when rows are kept."""

    def __init__(self, K: int, n: int, rows: bool):
        self.gt = None
        self.per_row = (np.empty(n, np.int32), np.empty(n, np.float32), np.empty(n, np.int32), np.empty(n, np.float32)) if rows else (None,) * 4
        self.tables = (np.zeros(_lib.MMC_EVAL_TOTALS, np.int64), np.zeros((K, K), np.int64), np.zeros(K, np.int64))
        self.args = tuple(_ptr(a) for a in self.per_row + self.tables)


class _Outputs:
    """Allocates the evaluate outputs of the calls of one validation and turns them into a ``Validation``."""

    def __init__(self, K: int, rows: bool):
        self.K, self.rows, self.calls = K, rows, []

    def call(self, n: int) -> _Call:
        self.calls.append(_Call(self.K, n, self.rows))
        return self.calls[-1]

    def result(self, classes) -> Validation:
        tot, conf, hist = (sum(c.tables[i] for c in self.calls) for i in range(3))
        if self.rows:
            cat = (lambda v: v[0]) if len(self.calls) == 1 else np.concatenate
            gt = cat([c.gt for c in self.calls])
            est, score, rank, p_true = (cat([c.per_row[i] for c in self.calls]) for i in range(4))
            score = score.astype(np.float64)
        else:
            gt = est = score = rank = p_true = None
        return Validation(classes, gt, est, score, rank, p_true, conf, hist, *tot.tolist())


def _set_labels(data: FeatureSet, first: int, n: int, lmap, st) -> np.ndarray:
    """The ground truth of rows [first, first + n) of a feature set as model class indices: the labels alone come back (no feature
    row does)."""
    y = np.empty(n, np.int32)
    _lib.check(_lib.lib().mmc_featureset_read(data._handle(), first, n, None, y.ctypes.data, st))
    return y if lmap is None else lmap[y]


def _validate(model, data, rows: bool, strict: bool) -> Validation:
    get_head, classes, sources = _prepare(model, data, rows, strict, "validate")
    out = _Outputs(len(classes), rows)
    head = get_head()
    lib = _lib.lib()
    st = _current_stream_ptr(head.device_index)
    for src, yi, lmap in sources:
        map_args = (_ptr(lmap), 0 if lmap is None else len(lmap))
        for first in range(0, len(src), MAX_ROWS_PER_CALL):
            cur = min(MAX_ROWS_PER_CALL, len(src) - first)
            c = out.call(cur)
            if yi is None:
                _lib.check(lib.mmc_head_evaluate_set(head._h, src._handle(), first, cur, *map_args, *c.args, st))
                if rows:
                    c.gt = _set_labels(src, first, cur, lmap, st)
            else:
                ys = yi[first:first + cur]
                _lib.check(lib.mmc_head_evaluate(head._h, src[first:first + cur].ctypes.data, ys.ctypes.data, cur, *map_args, *c.args,
                                                 _lib.MMC_IN_HOST, st))
                c.gt = ys if lmap is None else lmap[ys]
    return out.result(classes)


def validate(model, data, *, rows: bool = True) -> Validation:
    """Score every row of ``data`` with ``model`` (a ``CalibratedMLP`` or a ``Predictor``) on the device.  ``data`` is a
    ``FeatureSet`` (read in place), an ``(X, y)`` pair or an iterable of such batches (the forms ``calibration.evaluate`` takes);
    ``y`` are class labels.  A ``FeatureSet`` whose class list differs from the model's goes through a label map built on the
    host, and a class the model lacks maps to -1 (``Validation.n_unknown``); a label of a host batch that is not among the model's
    classes is a ``ValueError``.  ``rows=False`` asks for the totals only: nothing per row is computed into host memory."""
    return _validate(model, data, rows, strict=True)


def previous_accuracies(pc_models, val) -> List[float]:
    """``[accuracy_score(gts, ests)]`` of every earlier model on the validation data (trainer.py:273-277).  Each model has its own
    class list: the labels go through a map built per model, and a row whose class a model lacks counts as wrong for it, as the
    reference's comparison of label strings does.  Totals only."""
    if not isinstance(val, (FeatureSet, tuple, list)):
        val = list(val)   # an iterator of batches is walked once per model
    return [_validate(m, val, False, strict=False).accuracy for m in pc_models]
