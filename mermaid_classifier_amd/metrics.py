"""Grouped validation on the MI355X: the whole-split metric groups of the reference's ``MetricsCoordinator.compute_and_log_all``
(``mermaid_classifier/pyspacer/metrics/coordinator.py``) that ``validate``'s totals cannot answer.

===========================================================  ==============================================================
reference                                                    here
===========================================================  ==============================================================
``compute_cover`` (metrics/cover.py:24-146)                  ``GroupedValidation.cover``: ``CoverStats.table()``, ``.scalars()``
``compute_per_source`` (metrics/per_source.py:43-183)        ``GroupedValidation.sources``: ``SourceStats.table()``, ``.scalars()``
``_adaptive_ece`` (metrics/calibration.py:32-79)             ``GroupedValidation.reliability``: ``Reliability.ece``, ``.bins``
per-category log-loss (metrics/probability.py:43-60) and     ``GroupedValidation.by_class(category_of_class)``
accuracy / mean confidence (metrics/calibration.py:139-140)
per-category ECE (metrics/calibration.py:120-161)            ``GroupedValidation.category_reliability``, ``.category_calibration()``
===========================================================  ==============================================================

The reference walks ``ValResults`` row by row on the host.  Here ``mmc_head_evaluate_grouped(_set)`` adds one pass on the device to
``validate``'s evaluation and returns tables: exact integers wherever the quantity is a count (per-class sums, one confusion table
per source, the reliability bins found by a radix select instead of a sort), and fp64 sums reduced in a fixed order for the cover
statistics (per-image class counts stay in device scratch).  The objects below turn the tables into the reference's scalars and
table columns; like ``Validation`` they can be built from arrays.  No pandas, sklearn or matplotlib; no CPU fallback for the pass."""

from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from .backbone import _current_stream_ptr
from .validation import MAX_ROWS_PER_CALL, Validation, _Outputs, _prepare, _ptr, _set_labels

__all__ = ["grouped_validate", "GroupedValidation", "CoverStats", "SourceStats", "Reliability", "category_bins"]

COVER_COLUMNS = ("sum_true", "sum_pred", "sum_err", "sum_sq_err", "sum_abs_err", "min_true", "max_true", "sum_sq_dev_true")


class CoverStats:
    """Per-class sums over the images of the split.  ``sums[c] = (sum t, sum p, sum (p - t), sum (p - t)^2, sum |p - t|, min t,
    max t, sum (t - mean t)^2)`` with ``t`` / ``p`` the true / predicted cover fraction of class ``c`` in an image, over the
    ``n_images_used`` images that hold a scored row."""

    def __init__(self, sums, n_images_used: int):
        self.sums = np.asarray(sums, dtype=np.float64)
        self.n_images_used = int(n_images_used)
        if self.sums.ndim != 2 or self.sums.shape[1] != len(COVER_COLUMNS):
            raise ValueError(f"sums has shape {self.sums.shape}, expected (K, {len(COVER_COLUMNS)})")
        if self.n_images_used < 0:
            raise ValueError(f"n_images_used = {n_images_used} is negative")

    @classmethod
    def from_fractions(cls, true_cover, pred_cover) -> "CoverStats":
        """The sums from per-image cover fractions themselves: ``true_cover`` / ``pred_cover`` (n_images, K) float64, one row per
        image that counts (``cover.CoverEstimate.compare`` drops the images without a usable point first).  Host arithmetic."""
        t, p = np.asarray(true_cover, np.float64), np.asarray(pred_cover, np.float64)
        if t.ndim != 2 or t.shape != p.shape:
            raise ValueError(f"true_cover {t.shape} / pred_cover {p.shape} must be equal (n_images, K) shapes")
        n, K = t.shape
        sums = np.zeros((K, len(COVER_COLUMNS)))
        if n:
            d = p - t
            sums[:, 0], sums[:, 1], sums[:, 2], sums[:, 3], sums[:, 4] = t.sum(0), p.sum(0), d.sum(0), (d * d).sum(0), np.abs(d).sum(0)
            sums[:, 5], sums[:, 6] = t.min(0), t.max(0)
            sums[:, 7] = ((t - t.sum(0) / n) ** 2).sum(0)
        return cls(sums, n)

    def table(self) -> Dict[str, np.ndarray]:
        """The columns of ``cover/per_class_cover_metrics`` (cover.py:62-86) but the names: ``class`` (index), ``mean_true_cover_pct``,
        ``bias_pct``, ``rmse_pct``, ``mae_pct``, ``r_squared`` (NaN where the true cover is the same in every image), for the classes
        that occur in gt or est, by mean true cover descending (equal covers in class order)."""
        s, n = self.sums, self.n_images_used
        if n == 0:
            keep = np.zeros(0, np.int64)
        else:
            keep = np.flatnonzero((s[:, 0] > 0) | (s[:, 1] > 0))
        s = s[keep]
        with np.errstate(divide="ignore", invalid="ignore"):
            mean_true = s[:, 0] / n * 100 if n else np.zeros(0)
            r2 = np.where(s[:, 6] > s[:, 5], 1.0 - s[:, 3] / s[:, 7], np.nan)
        order = np.argsort(-mean_true, kind="stable")
        cols = {"class": keep, "mean_true_cover_pct": mean_true}
        if n:
            cols.update(bias_pct=s[:, 2] / n * 100, rmse_pct=np.sqrt(s[:, 3] / n) * 100, mae_pct=s[:, 4] / n * 100, r_squared=r2)
        else:
            cols.update(bias_pct=np.zeros(0), rmse_pct=np.zeros(0), mae_pct=np.zeros(0), r_squared=np.zeros(0))
        return {k: np.asarray(v)[order] for k, v in cols.items()}

    def scalars(self) -> Dict[str, float]:
        """``cover_mean_abs_bias_pct``, ``cover_mean_rmse_pct``, ``cover_mean_mae_pct``, ``cover_median_r_squared`` over the classes
        with more than 0.5 % mean true cover; the median skips NaN (NaN when nothing is left); all 0.0 without such a class
        (cover.py:88-120)."""
        t = self.table()
        sig = t["mean_true_cover_pct"] > 0.5
        names = ("cover_mean_abs_bias_pct", "cover_mean_rmse_pct", "cover_mean_mae_pct", "cover_median_r_squared")
        if not sig.any():
            return dict.fromkeys(names, 0.0)
        r2 = t["r_squared"][sig]
        r2 = r2[~np.isnan(r2)]
        return {names[0]: float(np.abs(t["bias_pct"][sig]).mean()), names[1]: float(t["rmse_pct"][sig].mean()),
                names[2]: float(t["mae_pct"][sig].mean()), names[3]: float(np.median(r2)) if len(r2) else float("nan")}


class SourceStats:
    """One confusion table per data source: ``confusion[s, gt, est]`` (int64)."""

    def __init__(self, confusion):
        self.confusion = np.asarray(confusion, dtype=np.int64)
        if self.confusion.ndim != 3 or self.confusion.shape[1] != self.confusion.shape[2]:
            raise ValueError(f"confusion has shape {self.confusion.shape}, expected (sources, K, K)")

    def _source(self, s: int, top):
        c = self.confusion[s]
        n = int(c.sum())
        tp = np.diag(c).astype(np.float64)
        support, predicted = c.sum(1).astype(np.float64), c.sum(0).astype(np.float64)
        present = (support + predicted) > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            recall_supported = tp[support > 0] / support[support > 0]
            precision = np.where(predicted > 0, tp / predicted, 0.0)[present]
            recall = np.where(support > 0, tp / support, 0.0)[present]
            f1 = np.where(support + predicted > 0, 2 * tp / (support + predicted), 0.0)[present]
        wrong = n - int(np.trace(c))
        out = dict(n=n, accuracy=int(np.trace(c)) / n, balanced_accuracy=float(recall_supported.mean()), f1_macro=float(f1.mean()),
                   precision_macro=float(precision.mean()), recall_macro=float(recall.mean()))
        if top is not None:
            cross = int(c[top[:, None] != top[None, :]].sum())   # (different top level implies off the diagonal)
            out["cross_branch_error_rate"] = cross / wrong if wrong else 0.0
        return out

    def _rows(self, top_of_class):
        top = None
        if top_of_class is not None:
            top = np.asarray(top_of_class)
            if top.shape != (self.confusion.shape[1],) or top.dtype.kind not in "iu":
                raise ValueError(f"top_of_class must be {self.confusion.shape[1]} integers")
        return [(s, self._source(s, top)) for s in range(len(self.confusion)) if self.confusion[s].any()]

    def table(self, source_keys: Sequence[Any], images_per_source: Sequence[int], top_of_class=None) -> Dict[str, list]:
        """The rows of ``per_source/metrics`` (per_source.py:88-165) as a dict of columns: accuracy, sklearn's balanced accuracy
        (mean recall over the classes with support), macro precision / recall / F1 over the labels present in gt or est of the
        source (``zero_division=0``), and -- with ``top_of_class[c]`` the integer id of class c's top-level ancestor -- the share
        of the errors that cross top-level branches.  Rounded to 4 decimals and sorted by annotations descending (equal counts in
        source order), as the reference does; sources without a scored row are left out."""
        S = len(self.confusion)
        if len(source_keys) != S or len(images_per_source) != S:
            raise ValueError(f"source_keys / images_per_source must have {S} entries")
        rows = self._rows(top_of_class)
        rows.sort(key=lambda r: -r[1]["n"])
        cols: Dict[str, list] = {"source_key": [source_keys[s] for s, _ in rows],
                                 "num_val_images": [int(images_per_source[s]) for s, _ in rows],
                                 "num_val_annotations": [r["n"] for _, r in rows]}
        for name in ("accuracy", "balanced_accuracy", "f1_macro", "precision_macro", "recall_macro", "cross_branch_error_rate"):
            if rows and name not in rows[0][1]:
                continue
            cols[name] = [round(r[name], 4) for _, r in rows]
        return cols

    def scalars(self) -> Dict[str, float]:
        """``per_source/n_sources``, ``per_source/min_accuracy``, ``per_source/max_accuracy`` (per_source.py:169-175); empty without
        a source that holds a scored row."""
        acc = [r["accuracy"] for _, r in self._rows(None)]
        if not acc:
            return {}
        return {"per_source/n_sources": float(len(acc)), "per_source/min_accuracy": float(min(acc)), "per_source/max_accuracy": float(max(acc))}


class Reliability:
    """The equal-mass reliability bins of ``_adaptive_ece`` (calibration.py:32-79) from per-bin integers: ``count``, ``n_correct``,
    ``conf_q32`` = sum of llrint(score * 2^32), and ``conf_min`` / ``conf_max``, the scores of the bin's first and last row in
    (score, correct) order."""

    def __init__(self, count, n_correct, conf_q32, conf_min, conf_max):
        self.count = np.asarray(count, dtype=np.int64)
        self.n_correct = np.asarray(n_correct, dtype=np.int64)
        self.conf_q32 = np.asarray(conf_q32, dtype=np.int64)
        self.conf_min = np.asarray(conf_min, dtype=np.float32)
        self.conf_max = np.asarray(conf_max, dtype=np.float32)
        if self.count.ndim != 1 or any(v.shape != self.count.shape for v in (self.n_correct, self.conf_q32, self.conf_min, self.conf_max)):
            raise ValueError("the per-bin columns must be 1-D and equally long")

    @property
    def bins(self) -> List[Dict[str, Any]]:
        """The dicts of ``_adaptive_ece`` plus ``gap`` (calibration.py:95), empty bins skipped."""
        out = []
        for c, k, q, lo, hi in zip(self.count.tolist(), self.n_correct.tolist(), self.conf_q32.tolist(), self.conf_min.tolist(),
                                   self.conf_max.tolist()):
            if c == 0:
                continue
            conf, acc = q / (c << 32), k / c
            out.append({"avg_confidence": conf, "avg_accuracy": acc, "count": c, "conf_min": lo, "conf_max": hi, "gap": conf - acc})
        return out

    @property
    def ece(self) -> float:
        n = int(self.count.sum())
        ece = 0.0
        for b in self.bins:
            ece += abs(b["avg_accuracy"] - b["avg_confidence"]) * b["count"] / n
        return ece


class GroupedValidation:
    """The outcome of ``grouped_validate``: ``validation`` (an ordinary ``Validation``), ``cover`` (``CoverStats``), ``sources``
    (``SourceStats``, or None without ``source_of_image``), ``reliability`` (``Reliability``) and the per-true-class integer sums
    ``support``, ``nll_q32``, ``score_q32``.  With ``category_of_class`` given to ``grouped_validate``: ``category_of_class`` (K
    integers, -1 = no category) and ``category_reliability``, one ``Reliability`` per category that holds a scored row, with the
    category's own bin count ``min(20, max(2, n // 10))`` (calibration.py:137); both None otherwise."""

    def __init__(self, validation: Validation, cover: CoverStats, sources: Optional[SourceStats], reliability: Reliability, support, nll_q32,
                 score_q32, category_of_class=None, category_reliability: Optional[Dict[int, Reliability]] = None):
        self.validation, self.cover, self.sources, self.reliability = validation, cover, sources, reliability
        if (category_of_class is None) != (category_reliability is None):
            raise ValueError("category_of_class and category_reliability go together")
        self.category_of_class = None if category_of_class is None else _check_categories(category_of_class, len(validation.classes))[0]
        self.category_reliability = None if category_reliability is None else dict(category_reliability)
        K = len(validation.classes)
        self.support = np.asarray(support, dtype=np.int64)
        self.nll_q32 = np.asarray(nll_q32, dtype=np.int64)
        self.score_q32 = np.asarray(score_q32, dtype=np.int64)
        if any(v.shape != (K,) for v in (self.support, self.nll_q32, self.score_q32)):
            raise ValueError(f"support / nll_q32 / score_q32 must have shape ({K},)")

    def by_class(self, category_of_class, min_samples: int = 30) -> Dict[int, Dict[str, float]]:
        """Per category (``category_of_class[c]``: an integer id, negative = leave the class out): ``log_loss``
        (probability.py:43-60), ``accuracy`` and ``avg_confidence`` (calibration.py:139-140) and ``n_samples`` over the scored rows
        whose true class lies in it, from integer adds; categories with fewer than ``min_samples`` rows are left out."""
        cat = np.asarray(category_of_class)
        if cat.shape != self.support.shape or cat.dtype.kind not in "iu":
            raise ValueError(f"category_of_class must be {len(self.support)} integers")
        correct = np.diag(self.validation.confusion)
        out = {}
        for c in sorted(set(cat[cat >= 0].tolist())):
            m = cat == c
            n = int(self.support[m].sum())
            if n < max(1, int(min_samples)):
                continue
            out[c] = {"log_loss": int(self.nll_q32[m].sum()) / (n << 32), "accuracy": int(correct[m].sum()) / n,
                      "avg_confidence": int(self.score_q32[m].sum()) / (n << 32), "n_samples": n}
        return out


    def category_calibration(self, min_samples: int = 30) -> List[Dict[str, Any]]:
        """The rows of ``calibration/per_category_ece`` (calibration.py:133-151): ``category`` (the integer id), ``ece``, ``accuracy``,
        ``avg_confidence``, ``n_samples``, by ``ece`` descending (equal ``ece`` by category id ascending: the reference's stable sort
        leaves insertion order there); categories with fewer than ``min_samples`` scored rows are left out.  ``accuracy`` and
        ``avg_confidence`` come from the integers ``by_class`` uses.  Needs ``grouped_validate(..., category_of_class=...)``."""
        if self.category_reliability is None:
            raise ValueError("no category tables: call grouped_validate(..., category_of_class=...)")
        sums = self.by_class(self.category_of_class, min_samples=min_samples)
        rows = []
        for c in sorted(self.category_reliability):
            if c not in sums:
                continue
            rel = self.category_reliability[c]
            if int(rel.count.sum()) != sums[c]["n_samples"]:
                raise ValueError(f"category {c}: the bins hold {int(rel.count.sum())} rows, the per-class sums {sums[c]['n_samples']}")
            rows.append({"category": c, "ece": rel.ece, "accuracy": sums[c]["accuracy"], "avg_confidence": sums[c]["avg_confidence"],
                         "n_samples": sums[c]["n_samples"]})
        rows.sort(key=lambda r: -r["ece"])
        return rows


def category_bins(n: int) -> int:
    """``n_bins_cat`` of a category of ``n`` rows (calibration.py:137); 0 without a row."""
    return min(_lib.MMC_CATEGORY_MAX_BINS, max(_lib.MMC_CATEGORY_MIN_BINS, n // _lib.MMC_CATEGORY_ROWS_PER_BIN)) if n > 0 else 0


def _check_categories(category_of_class, K: int):
    """-> (int32 array with every negative entry -1, number of categories); every complaint is a ValueError."""
    cat = np.asarray(category_of_class)
    if cat.shape != (K,) or cat.dtype.kind not in "iu":
        raise ValueError(f"category_of_class must be {K} integers")
    cat = np.where(cat < 0, -1, cat)
    if int(cat.max()) < 0:
        raise ValueError("category_of_class names no category")
    if int(cat.max()) >= _lib.MMC_CATEGORY_MAX:
        raise ValueError(f"category_of_class: category ids must lie below {_lib.MMC_CATEGORY_MAX}; got {int(cat.max())}")
    return np.ascontiguousarray(cat, dtype=np.int32), int(cat.max()) + 1


def _check_groups(n: int, image_sizes, source_of_image, n_bins):
    """-> (offsets int64, sources int32 or None, number of sources); every complaint is a ValueError."""
    sizes = np.asarray(image_sizes)
    if sizes.ndim != 1 or len(sizes) == 0 or sizes.dtype.kind not in "iu":
        raise ValueError("image_sizes must be a non-empty 1-D sequence of integers")
    if int(sizes.min()) < 1:
        raise ValueError(f"image_sizes[{int(sizes.argmin())}] = {int(sizes.min())}: every image holds at least one point")
    if int(sizes.sum(dtype=np.int64)) != n:
        raise ValueError(f"image_sizes add up to {int(sizes.sum(dtype=np.int64))}, the data has {n} rows")
    if isinstance(n_bins, bool) or int(n_bins) != n_bins or not 1 <= n_bins <= _lib.MMC_GROUPED_MAX_BINS:
        raise ValueError(f"n_bins must be an integer in [1, {_lib.MMC_GROUPED_MAX_BINS}]; got {n_bins!r}")
    offsets = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(sizes, out=offsets[1:])
    if source_of_image is None:
        return offsets, None, 0
    src = np.asarray(source_of_image)
    if src.shape != sizes.shape:
        raise ValueError(f"source_of_image has shape {src.shape}, expected {sizes.shape}")
    if src.dtype.kind not in "iu" or int(src.min()) < 0:
        raise ValueError("source_of_image must hold integers >= 0")
    return offsets, np.ascontiguousarray(src, dtype=np.int32), int(src.max()) + 1


def grouped_validate(model, data, image_sizes, *, source_of_image=None, n_bins: int = 20, rows: bool = False,
                     category_of_class=None) -> GroupedValidation:
    """``validate(model, data, rows=rows)`` plus the grouped tables, in one call on the device.  ``data`` is a ``FeatureSet``
    (read in place) or one ``(X, y)`` pair; ``image_sizes[i]`` is the number of points of image ``i``, in row order (each image's
    points are contiguous, cover.py:34-36); ``source_of_image[i]`` an integer source id.  Everything is checked on the host before
    the device is touched.  One call covers a whole split: more than ``MAX_ROWS_PER_CALL`` rows is a ``ValueError``.
    ``category_of_class`` (K integers below 64, negative = the class has no category) adds one reliability table per category
    (``mmc_head_evaluate_categories``): ``category_reliability`` and ``category_calibration()`` of the result."""
    get_head, classes, ((rows_src, yi, lmap),) = _prepare(model, data, rows, True, "grouped_validate", one_pair=True)
    K, n = len(classes), len(rows_src)
    if n > MAX_ROWS_PER_CALL:
        raise ValueError(f"{n} rows: one grouped call covers a whole split of at most {MAX_ROWS_PER_CALL} rows")
    offsets, src, S = _check_groups(n, image_sizes, source_of_image, n_bins)
    if len(offsets) - 1 > _lib.MMC_GROUPED_MAX_COVER_CELLS // K:
        raise ValueError(f"{len(offsets) - 1} images x {K} classes: at most {_lib.MMC_GROUPED_MAX_COVER_CELLS} per-image counts")
    if S * K * K > _lib.MMC_GROUPED_MAX_SOURCE_CELLS:
        raise ValueError(f"{S} sources x {K} x {K} classes: at most {_lib.MMC_GROUPED_MAX_SOURCE_CELLS} per-source cells")
    n_bins = int(n_bins)
    cat, C_ = (None, 0) if category_of_class is None else _check_categories(category_of_class, K)
    out = _Outputs(K, rows)
    c = out.call(n)
    support, nll, sq = np.zeros(K, np.int64), np.zeros(K, np.int64), np.zeros(K, np.int64)
    sconf = np.zeros((S, K, K), np.int64) if S else None
    cover = np.zeros((K, _lib.MMC_COVER_SUMS), np.float64)
    used = np.zeros(1, np.int64)
    bc, bk, bq = np.zeros(n_bins, np.int64), np.zeros(n_bins, np.int64), np.zeros(n_bins, np.int64)
    bmin, bmax = np.zeros(n_bins, np.float32), np.zeros(n_bins, np.float32)
    head = get_head()
    lib = _lib.lib()
    st = _current_stream_ptr(head.device_index)
    common = (_ptr(lmap), 0 if lmap is None else len(lmap), *c.args, offsets.ctypes.data, len(offsets) - 1, _ptr(src), S, n_bins,
              support.ctypes.data, nll.ctypes.data, sq.ctypes.data, _ptr(sconf), cover.ctypes.data, used.ctypes.data, bc.ctypes.data,
              bk.ctypes.data, bq.ctypes.data, bmin.ctypes.data, bmax.ctypes.data)
    evaluate_set, evaluate_rows = lib.mmc_head_evaluate_grouped_set, lib.mmc_head_evaluate_grouped
    if cat is not None:
        B = _lib.MMC_CATEGORY_MAX_BINS
        crows, cnb = np.zeros(C_, np.int64), np.zeros(C_, np.int32)
        cc, ck, cq = np.zeros((C_, B), np.int64), np.zeros((C_, B), np.int64), np.zeros((C_, B), np.int64)
        cmin, cmax = np.zeros((C_, B), np.float32), np.zeros((C_, B), np.float32)
        common += (cat.ctypes.data, C_, crows.ctypes.data, cnb.ctypes.data, cc.ctypes.data, ck.ctypes.data, cq.ctypes.data, cmin.ctypes.data,
                   cmax.ctypes.data)
        evaluate_set, evaluate_rows = lib.mmc_head_evaluate_categories_set, lib.mmc_head_evaluate_categories
    if yi is None:
        _lib.check(evaluate_set(head._h, rows_src._handle(), 0, n, *common, st))
        if rows:
            c.gt = _set_labels(rows_src, 0, n, lmap, st)
    else:
        _lib.check(evaluate_rows(head._h, rows_src.ctypes.data, yi.ctypes.data, n, *common, _lib.MMC_IN_HOST, st))
        c.gt = yi if lmap is None else lmap[yi]
    cat_rel = None
    if cat is not None:
        cat_rel = {c: Reliability(cc[c, :nb], ck[c, :nb], cq[c, :nb], cmin[c, :nb], cmax[c, :nb])
                   for c, nb in enumerate(cnb.tolist()) if crows[c] > 0}
    return GroupedValidation(out.result(classes), CoverStats(cover, int(used[0])), SourceStats(sconf) if S else None,
                             Reliability(bc, bk, bq, bmin, bmax), support, nll, sq, cat, cat_rel)
