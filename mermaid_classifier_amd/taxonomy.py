"""The taxonomic metric group of the reference's ``MetricsCoordinator.compute_and_log_all``
(``mermaid_classifier/pyspacer/metrics/taxonomic.py``), derived on the host from a K x K confusion table.

===========================================================  ==============================================================
reference                                                    here
===========================================================  ==============================================================
``_compute_error_attribution`` (taxonomic.py:55-177)         ``TaxonomicScores.error_attribution()``
``_compute_top_level_confusion`` (taxonomic.py:313-397)      ``TaxonomicScores.top_level_confusion()``
``_compute_gf_differentiation`` (taxonomic.py:400-547)       ``TaxonomicScores.growth_forms()``
the four scalars the three log                               ``TaxonomicScores.scalars()``
===========================================================  ==============================================================

The reference walks ``ValResults`` row by row; every number it makes is a function of the ``(gt, est)`` pairs alone, that is of the
confusion table ``Validation.confusion`` already holds (or of the sum of several).  Nothing here touches the device, and no per-row
data is needed.  Taxonomy libraries and names stay with the caller, as in ``ranking.py``: a class is described by the root-first path
of its benthic attribute (what ``build_ba_paths`` returns for it, the attribute itself included) and by its growth form, both as
hashable ids.  No pandas, sklearn or matplotlib.

Order where the reference's depends on row order.  ``Counter.most_common`` keeps equal counts in insertion order, the order in which
the rows of the split first produced each key; a table does not carry that.  The rules here, all over the table in row-major order
(true class, then prediction): error-attribution rows of equal count stand in the order of the first ``(g, est)`` cell that produced
their node; top-level categories of equal true frequency and growth forms of equal support stand in the order of their first class.

Two helpers have no counterpart in the reference: ``hierarchy_levels`` and ``soft_labels`` turn the same class paths, and the K x K
similarity matrix ``ranking_validate`` takes, into the arrays of the taxonomy-aware training loss (include/mmc.h, "taxonomy-aware
loss"; ``TorchMLPClassifier(class_levels=, soft_targets=)``)."""

from __future__ import annotations

from typing import Any, Dict, Hashable, List, Optional, Sequence

import numpy as np

__all__ = ["TaxonomicScores", "SCALAR_NAMES", "hierarchy_levels", "soft_labels"]

SCALAR_NAMES = ("cross_branch_error_rate", "within_branch_error_rate", "gf_accuracy_gf_relevant", "within_ba_gf_accuracy")


def _floor_pct(cm: np.ndarray) -> np.ndarray:
    """``np.floor(cm / row_sums * 100)`` in float64, the reference's own expression (taxonomic.py:343-345, 515-517): 29 of 100 is 28
    there, because 29 / 100 * 100 is 28.999999999999996.  Integer division would say 29."""
    row_sums = cm.sum(axis=1, keepdims=True)
    row_sums[row_sums == 0] = 1
    return np.floor(cm / row_sums * 100).astype(np.int64)


def _by_count(keys: Sequence[Hashable], counts: Dict[Hashable, int]) -> List[Hashable]:
    """``keys`` (in first-seen order) by count descending, equal counts in that order: ``Counter.most_common``."""
    return sorted(keys, key=lambda k: -counts[k])


class TaxonomicScores:
    """``confusion[g, est]``: K x K int64 counts, rows = true class.  ``class_paths[c]``: the root-first path of class c's benthic
    attribute, itself included (length >= 1, hashable nodes).  ``class_growth_form[c]``: a hashable id, or None for a class without
    a growth form."""

    def __init__(self, confusion, class_paths: Sequence[Sequence[Hashable]], class_growth_form: Sequence[Optional[Hashable]]):
        c = np.asarray(confusion)
        if c.ndim != 2 or c.shape[0] != c.shape[1] or c.dtype.kind not in "iu":
            raise ValueError(f"confusion must be a square table of integers; got shape {c.shape}, dtype {c.dtype}")
        if c.size and int(c.min()) < 0:
            raise ValueError("confusion holds a negative count")
        self.confusion = c.astype(np.int64)
        K = len(self.confusion)
        if len(class_paths) != K or len(class_growth_form) != K:
            raise ValueError(f"class_paths / class_growth_form must have {K} entries")
        self.paths = [tuple(p) for p in class_paths]
        if any(len(p) < 1 for p in self.paths):
            raise ValueError("every class path holds at least the class's own benthic attribute")
        self.growth_form = list(class_growth_form)
        self._cells = [(g, e, int(self.confusion[g, e])) for g in range(K) for e in range(K) if self.confusion[g, e] > 0]

    # ---- error attribution by lowest common ancestor ----

    def _lca(self, g: int, e: int):
        """``find_lca`` (_taxonomy_helpers.py:50-67): the last node the two paths share from the root; None when the roots differ.
        Two classes of one benthic attribute (different growth forms) share the whole path: the attribute itself."""
        lca = None
        for a, b in zip(self.paths[g], self.paths[e]):
            if a != b:
                break
            lca = a
        return lca

    def error_attribution(self) -> Dict[str, Any]:
        """``rows``: one dict per LCA node with ``lca_node`` (None = the errors that cross top-level branches), ``branch`` (the first
        node of the paths through the LCA; None for cross-branch), ``error_count``, ``pct_of_errors``, ``classes_in_subtree`` (the
        distinct class benthic attributes whose path contains the node; 0 for cross-branch), by count descending, equal counts in the
        order of the first ``(g, est)`` cell, row-major, that produced the node.  Plus ``cross_branch_error_rate`` and
        ``within_branch_error_rate``, both 0.0 without an error."""
        counts: Dict[Hashable, int] = {}
        branch: Dict[Hashable, Hashable] = {}
        total = 0
        for g, e, m in self._cells:
            if g == e:
                continue
            total += m
            node = self._lca(g, e)
            counts[node] = counts.get(node, 0) + m
            if node is not None:
                branch.setdefault(node, self.paths[g][0])
        if total == 0:
            return {"rows": [], "cross_branch_error_rate": 0.0, "within_branch_error_rate": 0.0}
        leaf_paths = {p[-1]: p for p in self.paths}
        rows = []
        for node in _by_count(list(counts), counts):
            rows.append({"lca_node": node, "branch": branch.get(node), "error_count": counts[node],
                         "pct_of_errors": counts[node] / total * 100,
                         "classes_in_subtree": 0 if node is None else sum(node in p for p in leaf_paths.values())})
        cross = counts.get(None, 0)
        return {"rows": rows, "cross_branch_error_rate": cross / total, "within_branch_error_rate": (total - cross) / total}

    # ---- top-level confusion ----

    def top_level_confusion(self) -> Dict[str, Any]:
        """``categories``: the top-level ids (first node of a class's path) by true frequency descending, then those seen only as a
        prediction, sorted ascending; ``matrix`` (int64 counts) and ``percent`` (row-normalised, ``np.floor(cm / row_sums * 100)``
        in float64 like the reference) over them; ``rows``: the off-diagonal cells with a count as dicts ``true``, ``predicted``,
        ``row_normalized_pct``, ``sample_count``, by percent descending, equal percents in row-major order."""
        top = [p[0] for p in self.paths]
        true_n: Dict[Hashable, int] = {}
        pred_n: Dict[Hashable, int] = {}
        for g, e, m in self._cells:
            true_n[top[g]] = true_n.get(top[g], 0) + m
            pred_n[top[e]] = pred_n.get(top[e], 0) + m
        first_class = {}
        for c, t in enumerate(top):
            first_class.setdefault(t, c)
        cats = _by_count(sorted(true_n, key=first_class.get), true_n)
        cats += sorted(set(pred_n) - set(true_n))
        at = {t: i for i, t in enumerate(cats)}
        cm = np.zeros((len(cats), len(cats)), np.int64)
        for g, e, m in self._cells:
            cm[at[top[g]], at[top[e]]] += m
        pct = _floor_pct(cm)
        rows = [{"true": cats[i], "predicted": cats[j], "row_normalized_pct": int(pct[i, j]), "sample_count": int(cm[i, j])}
                for i in range(len(cats)) for j in range(len(cats)) if i != j and cm[i, j] > 0]
        rows.sort(key=lambda r: -r["row_normalized_pct"])
        return {"categories": cats, "matrix": cm, "percent": pct, "rows": rows}

    # ---- growth forms ----

    def growth_forms(self) -> Dict[str, Any]:
        """Over the rows whose true class has a growth form: ``gf_accuracy_gf_relevant`` (the predicted class has the same growth
        form), ``within_ba_gf_accuracy`` (the same among the rows whose benthic attribute is predicted right; NaN when there is no
        such row); ``table``: per growth form ``growth_form``, ``precision``, ``recall``, ``f1`` (rounded to 3 places, a zero
        denominator gives 0: ``precision_recall_fscore_support(..., zero_division=0)``) and ``support``, by support descending;
        ``labels`` (those growth forms in that order), ``matrix`` (rows = labels, columns = labels + "no growth form" last;
        predictions of a growth form that is no label are dropped) and ``percent`` (the float floor of ``top_level_confusion``).
        Both scalars are 0.0, and the rest empty, without a row whose true class has a growth form."""
        gf = self.growth_form
        ba = [p[-1] for p in self.paths]
        cells = [(g, e, m) for g, e, m in self._cells if gf[g] is not None]
        n_rel = sum(m for _, _, m in cells)
        if n_rel == 0:
            return {"gf_accuracy_gf_relevant": 0.0, "within_ba_gf_accuracy": 0.0, "table": [], "labels": [],
                    "matrix": np.zeros((0, 1), np.int64), "percent": np.zeros((0, 1), np.int64)}
        right = sum(m for g, e, m in cells if gf[e] == gf[g])
        ba_n = sum(m for g, e, m in cells if ba[g] == ba[e])
        ba_right = sum(m for g, e, m in cells if ba[g] == ba[e] and gf[e] == gf[g])
        support: Dict[Hashable, int] = {}
        for g, _, m in cells:
            support[gf[g]] = support.get(gf[g], 0) + m
        first_class = {}
        for c, f in enumerate(gf):
            if f is not None:
                first_class.setdefault(f, c)
        labels = _by_count(sorted(support, key=first_class.get), support)
        at = {f: i for i, f in enumerate(labels)}
        cm = np.zeros((len(labels), len(labels) + 1), np.int64)
        for g, e, m in cells:
            col = len(labels) if gf[e] is None else at.get(gf[e])
            if col is not None:
                cm[at[gf[g]], col] += m
        table = []
        for i, f in enumerate(labels):
            tp, n_pred, n_true = int(cm[i, i]), int(cm[:, i].sum()), support[f]
            precision = tp / n_pred if n_pred else 0.0
            recall = tp / n_true
            f1 = 2 * tp / (n_pred + n_true)
            table.append({"growth_form": f, "precision": float(np.round(precision, 3)), "recall": float(np.round(recall, 3)),
                          "f1": float(np.round(f1, 3)), "support": n_true})
        return {"gf_accuracy_gf_relevant": right / n_rel, "within_ba_gf_accuracy": ba_right / ba_n if ba_n else float("nan"),
                "table": table, "labels": labels, "matrix": cm, "percent": _floor_pct(cm)}

    def scalars(self) -> Dict[str, float]:
        """The four scalars the reference logs for the group (``SCALAR_NAMES``)."""
        ea, g = self.error_attribution(), self.growth_forms()
        return {"cross_branch_error_rate": float(ea["cross_branch_error_rate"]), "within_branch_error_rate": float(ea["within_branch_error_rate"]),
                "gf_accuracy_gf_relevant": float(g["gf_accuracy_gf_relevant"]), "within_ba_gf_accuracy": float(g["within_ba_gf_accuracy"])}


def hierarchy_levels(class_paths: Sequence[Sequence[Hashable]], depths: Sequence[int] = (1, 2), attribute: bool = True) -> np.ndarray:
    """The level ids of the taxonomy-aware loss from the root-first paths ``TaxonomicScores`` takes -> K x L int32, row c the node of
    class c at every level.  One level per depth d of ``depths``: the node of a class is its path prefix of length d, and a class
    whose path is shorter than d gets its whole path.  With ``attribute=True`` one more level, the whole path: classes that share a
    benthic attribute and differ only in growth form share its node.  A node's id is the index of the first class in it."""
    paths = [tuple(p) for p in class_paths]
    if any(len(p) < 1 for p in paths):
        raise ValueError("every class path holds at least the class's own benthic attribute")
    depths = [int(d) for d in depths]
    if any(d < 1 for d in depths):
        raise ValueError(f"depths must be positive, got {depths!r}")
    keys = [[p[:d] for p in paths] for d in depths] + ([paths] if attribute else [])
    out = np.empty((len(paths), len(keys)), np.int32)
    for l, level in enumerate(keys):
        first: Dict[Any, int] = {}
        for c, key in enumerate(level):
            out[c, l] = first.setdefault(key, c)
    return out


def soft_labels(similarity, beta: float) -> np.ndarray:
    """Soft targets from a K x K similarity matrix S (the one ``ranking_validate`` takes): ``T[t, c] = exp(beta S[t, c]) /
    sum_c' exp(beta S[t, c'])``, in float64 with a row-max shift -> K x K float32.  ``ValueError`` for a matrix that is not square or
    holds a NaN, or a ``beta`` that is not finite."""
    S = np.asarray(similarity, dtype=np.float64)
    if S.ndim != 2 or S.shape[0] != S.shape[1]:
        raise ValueError(f"similarity must be a square matrix, got shape {S.shape}")
    if np.isnan(S).any():
        raise ValueError("similarity holds a NaN")
    if not np.isfinite(float(beta)):
        raise ValueError(f"beta must be finite, got {beta!r}")
    a = float(beta) * S
    e = np.exp(a - a.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
