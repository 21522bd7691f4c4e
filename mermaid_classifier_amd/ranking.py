"""Ranking validation on the MI355X: the metric group of the reference's ``compute_ranking``
(``mermaid_classifier/pyspacer/metrics/ranking.py``) that ``validate``'s overall rank histogram cannot answer.

===========================================================  ==============================================================
reference                                                    here
===========================================================  ==============================================================
``top_k_accuracy`` / ``mrr`` scalars (ranking.py:80-86)      ``RankedValidation.scalars()`` (from ``Validation.rank_hist``)
``ranking/per_category_topk`` (ranking.py:88-128)            ``RankedValidation.by_category(category_of_class)``
``ranking/hierarchical_topk`` (ranking.py:163-209)           ``RankedValidation.hierarchical()``
``taxonomic_similarity`` per (gt, candidate) pair            a K x K matrix from the caller -> ``similarity_levels``
===========================================================  ==============================================================

The reference sorts the N x K probability matrix on the host and walks it row by row.  Here ``mmc_head_evaluate_ranked(_set)`` adds
``rank_rows_kernel`` to ``validate``'s evaluation: per chunk it selects each scored row's best classes in the order of
``Predictor.predict_topk`` (score descending, equal scores in class order; the reference's ``np.argsort(-proba)`` leaves ties open),
looks their similarity to the true class up as a level code and counts.  Two integer tables come back, no row does:
``class_rank_hist[g, rank - 1]`` and ``hier_hist[j, level]`` (rows whose largest level among their ``j + 1`` best classes is
``level``).  The derivations below are integer adds and a few fp64 divisions.  Taxonomy libraries stay with the caller: it passes
integer category ids and the similarity matrix.  No pandas; no CPU fallback for the pass."""

from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .backbone import _current_stream_ptr
from .validation import MAX_ROWS_PER_CALL, Validation, _Outputs, _prepare, _ptr, _set_labels

__all__ = ["ranking_validate", "RankedValidation", "similarity_levels"]

MAX_K = 16        # include/mmc.h MMC_RANKED_MAX_K
MAX_LEVELS = 256  # level codes are uint8
DEFAULT_THRESHOLDS = ((1.0, "hit_exact"), (0.75, "hit_sibling_0.75"), (0.5, "hit_family_0.5"))


def similarity_levels(similarity) -> Tuple[np.ndarray, np.ndarray]:
    """K x K similarities (row = true class) -> ``(levels uint8 K x K, values float64 [n_levels])`` with
    ``values[levels] == similarity`` exactly.  ``values`` ascends, so the codes are monotone in the similarity and the largest
    code among some classes is the code of their largest similarity.  More than 256 distinct values, a NaN or a shape that is not
    square raises ``ValueError``."""
    S = np.asarray(similarity, dtype=np.float64)
    if S.ndim != 2 or S.shape[0] != S.shape[1] or S.shape[0] == 0:
        raise ValueError(f"similarity must be a K x K matrix, got shape {S.shape}")
    if np.isnan(S).any():
        raise ValueError("similarity holds a NaN")
    values = np.unique(S)
    if len(values) > MAX_LEVELS:
        raise ValueError(f"similarity takes {len(values)} distinct values: at most {MAX_LEVELS} levels")
    levels = np.searchsorted(values, S).astype(np.uint8)
    return np.ascontiguousarray(levels), values


def _ks(ks) -> List[int]:
    out = []
    for k in ks:
        if isinstance(k, bool) or int(k) != k or k < 1:
            raise ValueError(f"every k must be an integer >= 1; got {k!r}")
        out.append(int(k))
    return out


class RankedValidation:
    """The outcome of ``ranking_validate``: ``validation`` (an ordinary ``Validation``), ``class_rank_hist`` (K x K int64: scored
    rows of true class ``g`` whose true class ranks ``r + 1``-th, at ``[g, r]``) and -- with a similarity matrix, else None --
    ``hier_hist`` (kmax x n_levels int64: at ``[j, l]`` the scored rows whose largest similarity level to the true class among their
    ``j + 1`` best classes is ``l``) and ``level_values`` (the similarity of each level, ascending)."""

    def __init__(self, validation: Validation, class_rank_hist, hier_hist=None, level_values=None):
        self.validation = validation
        K = len(validation.classes)
        self.class_rank_hist = np.asarray(class_rank_hist, dtype=np.int64)
        if self.class_rank_hist.shape != (K, K):
            raise ValueError(f"class_rank_hist has shape {self.class_rank_hist.shape}, expected ({K}, {K})")
        if (hier_hist is None) != (level_values is None):
            raise ValueError("hier_hist and level_values must be given both or neither")
        self.hier_hist = None if hier_hist is None else np.asarray(hier_hist, dtype=np.int64)
        self.level_values = None if level_values is None else np.asarray(level_values, dtype=np.float64)
        if self.hier_hist is not None:
            if self.level_values.ndim != 1 or self.hier_hist.ndim != 2 or self.hier_hist.shape[1] != len(self.level_values) or \
                    not 1 <= self.hier_hist.shape[0] <= K:
                raise ValueError(f"hier_hist {self.hier_hist.shape} does not fit {len(self.level_values)} levels and {K} classes")

    @property
    def kmax(self) -> int:
        """The number of best classes the pass walked per row (0 without a similarity matrix)."""
        return 0 if self.hier_hist is None else int(self.hier_hist.shape[0])

    def by_category(self, category_of_class, ks: Sequence[int] = (1, 3, 5, 10), min_samples: int = 30) -> List[Dict[str, Any]]:
        """The rows of ``ranking/per_category_topk`` (ranking.py:103-117): per category (``category_of_class[c]``: an integer id,
        negative = leave the class out) over the scored rows whose true class lies in it ``category``, ``n_samples``, ``mrr`` and
        ``top_<k>``.  Categories with fewer than ``min_samples`` rows are left out; sorted by ``top_1`` descending (equal values in
        category order).  Integer adds over the classes of a category, then ``sum(hist[r] / (r + 1)) / n`` in fp64."""
        K = len(self.class_rank_hist)
        cat = np.asarray(category_of_class)
        if cat.shape != (K,) or cat.dtype.kind not in "iu":
            raise ValueError(f"category_of_class must be {K} integers")
        ks = _ks(ks)
        inv_rank = 1.0 / np.arange(1, K + 1, dtype=np.float64)
        rows = []
        for c in sorted(set(cat[cat >= 0].tolist())):
            hist = self.class_rank_hist[cat == c].sum(0)
            n = int(hist.sum())
            if n < max(1, int(min_samples)):
                continue
            row = {"category": c, "n_samples": n, "mrr": float((hist * inv_rank).sum() / n)}
            for k in ks:
                row[f"top_{k}"] = int(hist[:k].sum()) / n
            rows.append((int(hist[0]) / n, row))
        rows.sort(key=lambda r: r[0], reverse=True)   # (stable: equal top-1 shares stay in category order)
        return [row for _, row in rows]

    def _need_hier(self):
        if self.hier_hist is None:
            raise ValueError("no hierarchical table: ranking_validate(..., similarity=...) makes one")

    def hierarchical(self, ks: Sequence[int] = (1, 3, 5, 10), thresholds=DEFAULT_THRESHOLDS) -> List[Dict[str, Any]]:
        """The rows of ``ranking/hierarchical_topk`` (ranking.py:193-202): per ``k`` the mean over the scored rows of the largest
        similarity between the true class and the row's ``k`` best classes, and per ``(threshold, name)`` the share of rows where it
        reaches the threshold.  A ``k`` above ``kmax`` uses ``kmax`` (the reference's ``sims[:k]`` does the same when K < k).
        NaN without a scored row."""
        self._need_hier()
        rows = []
        for k in _ks(ks):
            hist = self.hier_hist[min(k, self.kmax) - 1]
            n = int(hist.sum())
            row = {"k": k, "mean_max_similarity": float((hist * self.level_values).sum() / n) if n else float("nan")}
            for t, name in thresholds:
                row[name] = int(hist[self.level_values >= t].sum()) / n if n else float("nan")
            rows.append(row)
        return rows

    def scalars(self) -> Dict[str, float]:
        """``top_{1,3,5,10}_accuracy`` and ``mrr`` (ranking.py:84-86, over every row: an unscored row is a miss) and, with a
        similarity matrix, ``hierarchical_top_5_mean_similarity`` (ranking.py:186-190)."""
        v = self.validation
        out = {f"top_{k}_accuracy": v.topk_accuracy(k) for k in (1, 3, 5, 10)}
        out["mrr"] = v.mrr
        if self.hier_hist is not None:
            out["hierarchical_top_5_mean_similarity"] = self.hierarchical(ks=(5,), thresholds=())[0]["mean_max_similarity"]
        return out


def ranking_validate(model, data, *, similarity=None, max_k: int = 10, rows: bool = False) -> RankedValidation:
    """``validate(model, data, rows=rows)`` plus the ranking tables, in the same pass on the device.  ``model`` and ``data`` are
    as for ``validate``.  ``similarity`` is the K x K matrix of similarities between the model's classes (row = true class,
    ``taxonomic_similarity`` in the reference), at most 256 distinct values; without it only ``class_rank_hist`` is made.
    ``max_k`` (at most 16; clamped to K) is the number of best classes walked per row: the largest ``k`` ``hierarchical`` can
    answer.  Everything is checked on the host before the device is touched."""
    if isinstance(max_k, bool) or not isinstance(max_k, (int, np.integer)) or not 1 <= max_k <= MAX_K:
        raise ValueError(f"max_k must be an integer in [1, {MAX_K}]; got {max_k!r}")
    get_head, classes, sources = _prepare(model, data, rows, True, "ranking_validate")
    K = len(classes)
    kmax = min(int(max_k), K)
    levels = values = None
    if similarity is not None:
        levels, values = similarity_levels(similarity)
        if levels.shape != (K, K):
            raise ValueError(f"similarity has shape {levels.shape}, the model has {K} classes")
    n_levels = 1 if values is None else len(values)
    out = _Outputs(K, rows)
    class_hist = np.zeros((K, K), np.int64)
    hier = None if levels is None else np.zeros((kmax, n_levels), np.int64)
    head = get_head()
    lib = _lib.lib()
    st = _current_stream_ptr(head.device_index)
    for src, yi, lmap in sources:
        map_args = (_ptr(lmap), 0 if lmap is None else len(lmap))
        for first in range(0, len(src), MAX_ROWS_PER_CALL):
            cur = min(MAX_ROWS_PER_CALL, len(src) - first)
            c = out.call(cur)
            ch = np.zeros((K, K), np.int64)
            hh = None if levels is None else np.zeros((kmax, n_levels), np.int64)
            ranked = (_ptr(levels), n_levels, kmax, ch.ctypes.data, _ptr(hh))
            if yi is None:
                _lib.check(lib.mmc_head_evaluate_ranked_set(head._h, src._handle(), first, cur, *map_args, *c.args, *ranked, st))
                if rows:
                    c.gt = _set_labels(src, first, cur, lmap, st)
            else:
                ys = yi[first:first + cur]
                _lib.check(lib.mmc_head_evaluate_ranked(head._h, src[first:first + cur].ctypes.data, ys.ctypes.data, cur, *map_args, *c.args,
                                                        *ranked, _lib.MMC_IN_HOST, st))
                c.gt = ys if lmap is None else lmap[ys]
            class_hist += ch   # integer tables: the calls add up exactly
            if hh is not None:
                hier += hh
    return RankedValidation(out.result(classes), class_hist, hier, values)
