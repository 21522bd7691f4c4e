"""Nearest neighbours between resident ``FeatureSet``s: label audit, a kNN probe of the features, near-duplicate search.

The reference has no counterpart.  Its point labels are noisy, its balancing report closes on a per-source accuracy floor that "may
motivate a per-source feature-extraction review" (``docs/research/balancing-experiments.md``, Caveats), and every validation number
assumes that the splits share no near-duplicate rows; all three questions are "which rows are close to which".  The device stage is
``mmc_featureset_knn`` (``include/mmc.h`` "nearest neighbours", ``csrc/neighbors.hip``): a fused exact-f32 product + top-k that never
stores the score matrix.  Everything here is host algebra on its nq x k lists:

``nearest``          -> ``Neighbors`` (``index`` relative to the base range, ``score``, ``label`` as class indices, ``classes``)
``Neighbors``        ``votes``, ``predict`` (ties by class order), ``agreement``
``knn_validate``     a kNN classifier on the features, scored with ``ClassScores`` and, with ``sources=``, ``SourceStats``
``audit_labels``     a self-search with the row's own group (image) excluded; rows sorted by agreement ascending
``near_duplicates``  pairs (a row, b row) whose best cosine reaches a threshold

Whether any of this improves labels, features or splits on reef data has NOT been measured.  No CPU fallback for ``nearest``; a
``Neighbors`` made from arrays needs no device.
"""

from __future__ import annotations

from typing import Any, Dict, NamedTuple, Optional, Tuple

import numpy as np

from . import _lib
from .class_scores import ClassScores

__all__ = ["METRICS", "Neighbors", "KnnValidation", "knn_splits", "nearest", "knn_validate", "audit_labels", "near_duplicates"]

METRICS = {"dot": _lib.MMC_KNN_DOT, "cosine": _lib.MMC_KNN_COSINE, "l2": _lib.MMC_KNN_L2}


def knn_splits(nq: int, nb: int) -> int:
    """The number of contiguous base-tile ranges ``mmc_featureset_knn`` cuts ``nb`` base rows into for ``nq`` queries: the rule of
    ``include/mmc.h``, ``min(MMC_KNN_MAX_SPLITS, base tiles, max(1, 1024 / query tiles of one chunk))``."""
    t = _lib.MMC_KNN_TILE_ROWS
    query_tiles = (min(int(nq), _lib.MMC_KNN_CHUNK_ROWS) + t - 1) // t
    base_tiles = (int(nb) + t - 1) // t
    return max(1, min(_lib.MMC_KNN_MAX_SPLITS, base_tiles, max(1, 1024 // query_tiles if query_tiles else 1)))


class Neighbors:
    """``Neighbors(index, score, label, classes)``: per query row its neighbours, best first.  ``index`` (nq, k) int32 relative to the
    base range, ``score`` (nq, k) float32, ``label`` (nq, k) int32 indices into ``classes``; where fewer than k rows were eligible the
    tail holds ``index = -1``, ``score = -inf``, ``label = -1``."""

    def __init__(self, index, score, label, classes):
        self.index = np.asarray(index, dtype=np.int32)
        self.score = np.asarray(score, dtype=np.float32)
        self.label = np.asarray(label, dtype=np.int32)
        self.classes = np.asarray(classes)
        if self.index.ndim != 2 or self.score.shape != self.index.shape or self.label.shape != self.index.shape:
            raise ValueError(f"index {self.index.shape}, score {self.score.shape} and label {self.label.shape} must be one (nq, k) shape")
        if self.label.size and int(self.label.max()) >= len(self.classes):
            raise ValueError(f"a label index reaches {int(self.label.max())}, classes has {len(self.classes)} entries")

    def __len__(self) -> int:
        return int(self.index.shape[0])

    @property
    def k(self) -> int:
        return int(self.index.shape[1])

    @property
    def valid(self) -> np.ndarray:
        """(nq, k) bool: the entries that hold a neighbour."""
        return self.index >= 0

    def votes(self, weights: str = "uniform") -> np.ndarray:
        """-> (nq, K) float64: per class the number of valid neighbours (``"uniform"``) or the sum of their scores as returned
        (``"score"``: meant for cosine / dot, where a larger score is a closer row and scores of interest are positive)."""
        if weights not in ("uniform", "score"):
            raise ValueError(f"weights must be 'uniform' or 'score', got {weights!r}")
        nq, K = len(self), len(self.classes)
        out = np.zeros((nq, K), np.float64)
        ok = self.valid
        rows = np.broadcast_to(np.arange(nq)[:, None], ok.shape)[ok]
        w = np.ones(int(ok.sum()), np.float64) if weights == "uniform" else self.score[ok].astype(np.float64)
        np.add.at(out, (rows, self.label[ok]), w)
        return out

    def predict(self, weights: str = "uniform") -> np.ndarray:
        """-> (nq,) labels out of ``classes``: the class with the largest vote, equal votes by class order (a row without a valid
        neighbour therefore gets ``classes[0]``)."""
        return self.classes[np.argmax(self.votes(weights), axis=1)]

    def agreement(self, y) -> np.ndarray:
        """``y``: (nq,) labels out of ``classes`` -> (nq,) float64, the share of each row's valid neighbours that carry its label;
        NaN for a row without a valid neighbour."""
        yi = _label_indices(self.classes, y, len(self))
        ok = self.valid
        n_ok = ok.sum(axis=1)
        same = (ok & (self.label == yi[:, None])).sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(n_ok > 0, same / n_ok, np.nan)


def _label_indices(classes, y, n: int) -> np.ndarray:
    y = np.asarray(y)
    if y.shape != (n,):
        raise ValueError(f"y has shape {y.shape}, expected ({n},)")
    idx = np.searchsorted(classes, y)
    if n and not np.array_equal(classes[np.minimum(idx, len(classes) - 1)], y):
        raise ValueError(f"labels {sorted(set(y.tolist()) - set(classes.tolist()))} are not in classes")
    return idx.astype(np.int64)


def _range(fs, rows, what: str) -> Tuple[int, int]:
    total = len(fs)
    first, n = (0, total) if rows is None else (int(rows[0]), int(rows[1]))
    if first < 0 or n < 0 or first + n > total:
        raise ValueError(f"{what} rows [{first}, {first + n}) outside the set's {total} rows")
    return first, n


def _groups(g, n: int, what: str) -> np.ndarray:
    a = np.asarray(g)
    if a.shape != (n,) or a.dtype.kind not in "iu":
        raise ValueError(f"{what} must be {n} integers, got {a.dtype} {a.shape}")
    if n and (int(a.min()) < -2 ** 31 or int(a.max()) >= 2 ** 31):
        raise ValueError(f"{what} must fit int32")
    return np.ascontiguousarray(a.astype(np.int32))


def nearest(query, base, k: int, metric: str = "cosine", *, query_groups=None, base_groups=None, exclude_self: bool = False,
            query_rows: Optional[Tuple[int, int]] = None, base_rows: Optional[Tuple[int, int]] = None) -> Neighbors:
    """The ``k`` best rows of ``base`` (rows ``base_rows = (first, n)``, None: all) for every row of ``query`` (``query_rows``), by
    ``metric`` in ``"cosine"``, ``"dot"``, ``"l2"`` (scores: larger is better; l2 is minus the squared distance).  A base row is
    skipped for a query whose group id (``query_groups`` / ``base_groups``: integers, one per row of the ranges, both or neither)
    equals its own, and with ``exclude_self`` (``query is base`` only) when it is the query row itself.  Argument errors are raised
    before a device is touched."""
    from .backbone import _current_stream_ptr
    from .featureset import FeatureSet
    if not isinstance(query, FeatureSet) or not isinstance(base, FeatureSet):
        raise ValueError("query and base must be FeatureSets")
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {tuple(METRICS)}, got {metric!r}")
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= _lib.MMC_KNN_MAX_K:
        raise ValueError(f"k must be an integer in [1, {_lib.MMC_KNN_MAX_K}], got {k!r}")
    if query.dim != base.dim:
        raise ValueError(f"query has {query.dim} features, base {base.dim}")
    if query.device_index != base.device_index:
        raise ValueError(f"query is on device {query.device_index}, base on device {base.device_index}")
    if exclude_self and query is not base:
        raise ValueError("exclude_self needs query and base to be the same set")
    if (query_groups is None) != (base_groups is None):
        raise ValueError("query_groups and base_groups: both, or neither")
    q_first, nq = _range(query, query_rows, "query")
    b_first, nb = _range(base, base_rows, "base")
    k = int(k)
    qg = bg = None
    if query_groups is not None:
        qg, bg = _groups(query_groups, nq, "query_groups"), _groups(base_groups, nb, "base_groups")
    index = np.full((nq, k), -1, np.int32)
    score = np.full((nq, k), -np.inf, np.float32)
    label = np.full((nq, k), -1, np.int32)
    if nq:
        flags = _lib.MMC_IN_HOST | _lib.MMC_OUT_HOST | (_lib.MMC_KNN_EXCLUDE_SELF if exclude_self else 0)
        _lib.check(_lib.lib().mmc_featureset_knn(query._handle(), q_first, nq, base._handle(), b_first, nb, k, METRICS[metric],
                                                 None if qg is None else qg.ctypes.data, None if bg is None else bg.ctypes.data,
                                                 index.ctypes.data, score.ctypes.data, label.ctypes.data, flags,
                                                 _current_stream_ptr(query.device_index)))
    return Neighbors(index, score, label, base.classes)


def _stored_labels(fs) -> np.ndarray:
    """The set's labels as class indices, without moving its rows."""
    from .backbone import _current_stream_ptr
    n = len(fs)
    yi = np.empty(n, np.int32)
    if n:
        _lib.check(_lib.lib().mmc_featureset_read(fs._handle(), 0, n, None, yi.ctypes.data, _current_stream_ptr(fs.device_index)))
    return yi


class KnnValidation(NamedTuple):
    confusion: np.ndarray          # (K, K) int64, [gt, est]
    scores: ClassScores
    sources: Any                   # metrics.SourceStats with ``sources=``, else None
    neighbors: Neighbors


def confusion_table(gt_idx, est_idx, K: int, sources=None, n_sources: Optional[int] = None) -> np.ndarray:
    """(K, K) int64 counts ``[gt, est]``, or (S, K, K) per source with ``sources`` (one integer in [0, S) per row)."""
    gt, est = np.asarray(gt_idx, np.int64), np.asarray(est_idx, np.int64)
    if sources is None:
        return np.bincount(gt * K + est, minlength=K * K).reshape(K, K).astype(np.int64)
    src = np.asarray(sources)
    if src.shape != gt.shape or src.dtype.kind not in "iu":
        raise ValueError(f"sources must be {len(gt)} integers")
    S = int(n_sources) if n_sources is not None else (int(src.max()) + 1 if len(src) else 0)
    if len(src) and (int(src.min()) < 0 or int(src.max()) >= S):
        raise ValueError(f"a source id lies outside [0, {S})")
    return np.bincount((src.astype(np.int64) * K + gt) * K + est, minlength=S * K * K).reshape(S, K, K).astype(np.int64)


def knn_validate(train, val, k: int, metric: str = "cosine", *, weights: str = "uniform", sources=None, n_sources: Optional[int] = None,
                 train_groups=None, val_groups=None) -> KnnValidation:
    """A kNN classifier on the features: every row of ``val`` is given the majority label of its ``k`` nearest rows of ``train``
    (``Neighbors.predict``) and scored against its stored label.  -> ``KnnValidation(confusion, scores, sources, neighbors)``:
    the K x K table ``[gt, est]``, its ``ClassScores`` and, with ``sources`` (one source index per val row), the per-source tables as
    the ``SourceStats`` that ``grouped_validate`` reports (``.scalars()``: ``per_source/min_accuracy`` ...).  Both sets must carry
    the same classes."""
    from .metrics import SourceStats
    if not np.array_equal(train.classes, val.classes):
        raise ValueError("train and val must carry the same classes")
    nb = nearest(val, train, k, metric, query_groups=val_groups, base_groups=train_groups)
    K = len(val.classes)
    est = np.argmax(nb.votes(weights), axis=1)
    gt = _stored_labels(val)
    confusion = confusion_table(gt, est, K)
    per_source = None if sources is None else SourceStats(confusion_table(gt, est, K, sources, n_sources))
    return KnnValidation(confusion, ClassScores(confusion, val.classes), per_source, nb)


def audit_table(nb: Neighbors, y) -> Dict[str, np.ndarray]:
    """The host half of ``audit_labels``: ``y`` (nq,) the rows' own labels -> columns sorted by agreement ascending (equal
    agreement in row order; rows without a valid neighbour last): ``row``, ``label``, ``agreement``, ``majority`` (the neighbours'
    majority label, ties by class order) and ``majority_share`` (its share of the valid neighbours)."""
    agree = nb.agreement(y)
    votes = nb.votes("uniform")
    n_ok = votes.sum(axis=1)
    top = np.argmax(votes, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(n_ok > 0, votes[np.arange(len(nb)), top] / n_ok, np.nan)
    order = np.argsort(np.where(np.isnan(agree), np.inf, agree), kind="stable")
    return {"row": order.astype(np.int64), "label": np.asarray(y)[order], "agreement": agree[order],
            "majority": nb.classes[top][order], "majority_share": share[order]}


def audit_labels(fs, k: int, groups=None, metric: str = "cosine") -> Dict[str, np.ndarray]:
    """Candidates for label review: every row of ``fs`` against all the others -- those of its own group left out when ``groups``
    (one integer per row, e.g. the image id: points of one image overlap) is given, else only the row itself -- sorted by the share
    of the ``k`` neighbours that carry the row's label, ascending.  Columns: see ``audit_table``."""
    if groups is None:
        nb = nearest(fs, fs, k, metric, exclude_self=True)
    else:
        nb = nearest(fs, fs, k, metric, query_groups=groups, base_groups=groups, exclude_self=True)
    return audit_table(nb, fs.classes[_stored_labels(fs)])


def duplicate_pairs(nb: Neighbors, threshold: float) -> Dict[str, np.ndarray]:
    """The host half of ``near_duplicates``: the (query row, base row, score) of every listed neighbour whose score is >=
    ``threshold``, by query row, then best first."""
    hit = nb.valid & (nb.score >= np.float32(threshold))
    rows = np.broadcast_to(np.arange(len(nb))[:, None], hit.shape)[hit]
    return {"a": rows.astype(np.int64), "b": nb.index[hit].astype(np.int64), "score": nb.score[hit]}


def near_duplicates(a, b, threshold: float = 0.999, k: int = 1) -> Dict[str, np.ndarray]:
    """Rows of ``a`` with a near-duplicate in ``b``: -> columns ``a``, ``b`` (row numbers), ``score`` of the pairs among each ``a``
    row's ``k`` best cosine neighbours in ``b`` whose cosine is >= ``threshold``.  With ``a is b`` the row itself is left out (and
    every pair appears from both sides)."""
    if not np.isfinite(threshold):
        raise ValueError(f"threshold must be finite, got {threshold!r}")
    return duplicate_pairs(nearest(a, b, k, "cosine", exclude_self=a is b), threshold)
