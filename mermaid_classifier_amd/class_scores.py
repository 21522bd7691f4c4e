"""``ClassScores``: the confusion-matrix groups of the reference's ``MetricsCoordinator`` --
``compute_precision_recall_f1`` and ``compute_balanced_accuracy_mcc`` (``mermaid_classifier/pyspacer/metrics/
classification.py:171-302``) -- from a K x K table of integer counts.

The reference hands label lists to sklearn; every score it reads there is a function of the confusion matrix alone, and the device
already returns that matrix as exact integers: ``Validation.confusion`` for a calibrated head (``calibrate_eval_kernel``) and
``calibration.evaluate_classes`` for the classifier during training (``eval_rows_kernel<CONF>``).  Everything below is float64
arithmetic on those integers, with sklearn's conventions.  No sklearn in the path."""

from __future__ import annotations

import math
from typing import Any, Dict

import numpy as np

__all__ = ["ClassScores"]


class ClassScores:
    """``ClassScores(confusion, classes)``: ``confusion[gt, est]`` (K x K integers, counts >= 0) over ``classes`` (K entries)."""

    def __init__(self, confusion, classes):
        c = np.asarray(confusion)
        self.classes = np.asarray(classes).tolist()
        K = len(self.classes)
        if c.shape != (K, K):
            raise ValueError(f"confusion has shape {c.shape}, expected ({K}, {K})")
        if c.dtype.kind not in "iu":
            raise ValueError(f"confusion must hold integers, got {c.dtype}")
        if K and int(c.min()) < 0:
            raise ValueError("confusion holds a negative count")
        self.confusion = c.astype(np.int64)
        self._tp = np.diag(self.confusion).astype(np.float64)
        self._support = self.confusion.sum(1)      # rows of each true class
        self._predicted = self.confusion.sum(0)    # rows of each predicted class

    @property
    def n(self) -> int:
        return int(self.confusion.sum())

    def per_class(self) -> Dict[str, np.ndarray]:
        """-> ``precision``, ``recall``, ``f1`` (float64) and ``support`` (int64), one entry per class in class order: the columns of
        ``metrics_per_label`` (classification.py:194-232).  ``zero_division = 0``; ``f1 = 0`` where ``precision + recall == 0``."""
        with np.errstate(divide="ignore", invalid="ignore"):
            p = np.where(self._predicted > 0, self._tp / self._predicted, 0.0)
            r = np.where(self._support > 0, self._tp / self._support, 0.0)
            f = np.where(p + r > 0, 2 * (p * r) / (p + r), 0.0)
        return {"precision": p, "recall": r, "f1": f, "support": self._support.copy()}

    def _macro(self, name: str) -> float:
        present = (self._support + self._predicted) > 0    # sklearn's default label set: the classes in gt or est
        if not present.any():
            return float("nan")
        return float(self.per_class()[name][present].mean())

    @property
    def precision_macro(self) -> float:
        """``precision_score(average="macro", zero_division=0)`` over the classes present in gt or est (classification.py:245-250)."""
        return self._macro("precision")

    @property
    def recall_macro(self) -> float:
        """``recall_score(average="macro", zero_division=0)`` over the same classes (classification.py:251-256)."""
        return self._macro("recall")

    @property
    def f1_macro(self) -> float:
        """The harmonic mean of the two macro averages (classification.py:257), 0 when both are 0 -- not the mean of the per-class
        f1 (which is what ``metrics.SourceStats`` reports per source, as per_source.py does)."""
        p, r = self.precision_macro, self.recall_macro
        return 2 * (p * r) / (p + r) if (p + r) > 0 else 0.0

    @property
    def balanced_accuracy(self) -> float:
        """``sklearn.metrics.balanced_accuracy_score`` (classification.py:294): the mean recall over the classes with support."""
        has = self._support > 0
        if not has.any():
            return float("nan")
        return float((self._tp[has] / self._support[has]).mean())

    @property
    def mcc(self) -> float:
        """``sklearn.metrics.matthews_corrcoef`` (classification.py:295) as it is computed from the confusion matrix; 0 when the
        denominator is 0.  The covariances are exact integers here (Python ints); one square root and one division round."""
        t = [int(v) for v in self._support]
        p = [int(v) for v in self._predicted]
        n, correct = sum(t), int(np.trace(self.confusion))
        cov_tp = correct * n - sum(a * b for a, b in zip(t, p))
        cov_pp = n * n - sum(b * b for b in p)
        cov_tt = n * n - sum(a * a for a in t)
        if cov_pp * cov_tt == 0:
            return 0.0
        return cov_tp / math.sqrt(cov_pp * cov_tt)

    @property
    def accuracy(self) -> float:
        n = self.n
        return int(np.trace(self.confusion)) / n if n else float("nan")

    def scalars(self) -> Dict[str, Any]:
        """The scalars the two reference groups log: ``precision_macro``, ``recall_macro``, ``f1_macro``, ``balanced_accuracy``,
        ``mcc``; and ``accuracy``."""
        return {k: getattr(self, k) for k in ("precision_macro", "recall_macro", "f1_macro", "balanced_accuracy", "mcc", "accuracy")}
