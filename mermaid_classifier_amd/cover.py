"""Cover estimates on the MI355X: percent benthic cover per image, transect or source.

The reference has cover only as a validation metric (``compute_cover``, mermaid_classifier/pyspacer/metrics/cover.py: per-image
argmax counts against the annotated counts).  ``estimate_cover`` is the serving-side product: per contiguous group of points it
returns the argmax counts (``hard_cover``), the sum of the calibrated probabilities (``soft_cover``) and the class prior
re-estimated from those probabilities by EM (``adapted_cover``; Saerens, Latinne and Decaestecker 2002: the test-time remedy for
label shift, whose training-time half is the trainer's ``logit_prior``), and optionally the top-k labels under the adapted prior.
The definition is the text of include/mmc.h, section "cover estimation"; the arithmetic runs on the device (csrc/cover.hip) on the
probabilities where they lie -- ``mmc_head_cover`` / ``mmc_head_cover_set`` for a predictor, ``mmc_cover_proba`` for probabilities
made elsewhere.  No CPU fallback.
"""

from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from .backbone import _current_stream_ptr, check_views_per_point
from .classify import PointPredictions
from .featureset import FeatureSet
from .metrics import CoverStats

__all__ = ["estimate_cover", "CoverEstimate", "prior_from_labels", "check_cover_arguments"]

ESTIMATORS = ("hard", "soft", "adapted")


def prior_from_labels(y, K: int, pseudo_count: float = 0.0) -> np.ndarray:
    """The class frequencies of the training labels ``y`` (class indices in [0, K)) as a ``train_prior``: (K,) float64 summing to 1.
    Every class needs a positive entry; ``pseudo_count`` is added to every class count for label sets that miss a class."""
    K = int(K)
    if K < 1:
        raise ValueError(f"K must be positive; got {K}")
    if not (pseudo_count >= 0 and np.isfinite(pseudo_count)):
        raise ValueError(f"pseudo_count must be finite and >= 0; got {pseudo_count!r}")
    y = np.asarray(y)
    if y.ndim != 1 or (y.size and not np.issubdtype(y.dtype, np.integer)):
        raise ValueError(f"y must be a 1-D array of integer class indices; got {y.dtype} {y.shape}")
    if y.size and (y.min() < 0 or y.max() >= K):
        raise ValueError(f"labels outside [0, {K})")
    cnt = np.bincount(y.astype(np.int64), minlength=K).astype(np.float64) + float(pseudo_count)
    if not cnt.sum() > 0 or (cnt <= 0).any():
        raise ValueError(f"classes {np.flatnonzero(cnt <= 0).tolist()} have no label: every train_prior entry must be positive "
                         "(pass a pseudo_count)")
    return cnt / cnt.sum()


def check_cover_arguments(n_points: int, K: int, group_offsets, train_prior, strength, iters, k):
    """The host checks of every cover front-end, before the device is touched -> (offsets int64 (n_groups + 1,), train_prior
    float64 (K,) or None, strength, iters, k clamped to K).  ValueError names the offending argument."""
    off = np.asarray(group_offsets)
    if off.ndim != 1 or off.size < 1 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError(f"group_offsets must be a 1-D integer array of n_groups + 1 entries; got {off.dtype} {off.shape}")
    off = np.ascontiguousarray(off, dtype=np.int64)
    if off[0] != 0 or off[-1] != n_points or (np.diff(off) < 0).any():
        raise ValueError(f"group_offsets must start at 0, never decrease and end at the {n_points} points; got "
                         f"[{off[0]} .. {off[-1]}]")
    if n_points * K > _lib.MMC_COVER_MAX_CELLS:
        raise ValueError(f"{n_points} points x {K} classes exceed the {_lib.MMC_COVER_MAX_CELLS} resident cells of one call")
    tp = None
    if train_prior is not None:
        tp = np.ascontiguousarray(np.asarray(train_prior, dtype=np.float64))
        if tp.shape != (K,):
            raise ValueError(f"train_prior must have shape ({K},); got {tp.shape}")
        if not (np.isfinite(tp).all() and (tp > 0).all()):
            raise ValueError("every train_prior entry must be a positive finite number")
        if not abs(float(tp.sum()) - 1.0) <= 1e-6:
            raise ValueError(f"train_prior sums to {float(tp.sum())!r}: must be 1 within 1e-6")
    strength = float(strength)
    if not (strength >= 0 and np.isfinite(strength)):
        raise ValueError(f"strength must be finite and >= 0; got {strength!r}")
    if isinstance(iters, bool) or int(iters) != iters or not 0 <= iters <= _lib.MMC_COVER_MAX_ITERS:
        raise ValueError(f"iters must be an integer in [0, {_lib.MMC_COVER_MAX_ITERS}]; got {iters!r}")
    if isinstance(k, bool) or int(k) != k or k < 0:
        raise ValueError(f"k must be an integer >= 0 (0: no adapted top-k); got {k!r}")
    return off, tp, strength, int(iters), min(int(k), K)


class CoverEstimate:
    """What one cover call returns, per group: ``counts`` (n_groups, K) int64 argmax counts, ``soft_q32`` (n_groups, K) int64 sums
    of the probabilities in units of 2^-32, ``unusable`` (n_groups,) points with a non-finite probability, ``n`` (n_groups,) usable
    points, ``prior`` (n_groups, K) float64 the EM-adapted class prior; ``topk`` the ``PointPredictions`` under the adapted prior
    (None without ``k``); ``groups`` the group ids of ``cover_images`` (None elsewhere)."""

    def __init__(self, counts, soft_q32, unusable, sizes, prior, topk: Optional[PointPredictions] = None, groups=None):
        self.counts = np.asarray(counts, dtype=np.int64)
        self.soft_q32 = np.asarray(soft_q32, dtype=np.int64)
        self.unusable = np.asarray(unusable, dtype=np.int64)
        self.prior = np.asarray(prior, dtype=np.float64)
        if self.counts.ndim != 2 or self.soft_q32.shape != self.counts.shape or self.prior.shape != self.counts.shape:
            raise ValueError(f"counts {self.counts.shape}, soft_q32 {self.soft_q32.shape} and prior {self.prior.shape} must be equal "
                             "(n_groups, K) shapes")
        sizes = np.asarray(sizes, dtype=np.int64)
        if self.unusable.shape != (self.counts.shape[0],) or sizes.shape != self.unusable.shape:
            raise ValueError(f"unusable {self.unusable.shape} / sizes {sizes.shape} must have shape ({self.counts.shape[0]},)")
        self.n = sizes - self.unusable
        self.topk = topk
        self.groups = groups

    def _over_n(self, table) -> np.ndarray:
        out = np.full(self.counts.shape, np.nan)
        used = self.n > 0
        out[used] = np.asarray(table, np.float64)[used] / self.n[used, None]
        return out

    def hard_cover(self) -> np.ndarray:
        """(n_groups, K) float64: the fraction of a group's usable points whose best class is c (cover.py's predicted cover).  NaN
        rows for a group without a usable point, here and below."""
        return self._over_n(self.counts)

    def soft_cover(self) -> np.ndarray:
        """The mean calibrated probability of class c over the group's usable points."""
        return self._over_n(self.soft_q32.astype(np.float64) / 4294967296.0)

    def adapted_cover(self) -> np.ndarray:
        """The group's class prior after the EM iterations."""
        out = self.prior.copy()
        out[self.n <= 0] = np.nan
        return out

    def cover(self, estimator: str) -> np.ndarray:
        if estimator not in ESTIMATORS:
            raise ValueError(f"estimator must be one of {ESTIMATORS}; got {estimator!r}")
        return getattr(self, estimator + "_cover")()

    def compare(self, true_counts, estimator: str = "hard") -> CoverStats:
        """The per-class table and scalars of ``compute_cover`` (cover.py:44-120) for one estimator against annotated counts:
        ``true_counts`` (n_groups, K) non-negative integers, the true cover of a group being its row over its row sum.  Groups
        without a usable point or without a true label are left out.  -> ``CoverStats`` (``.table()``, ``.scalars()``)."""
        p = self.cover(estimator)
        t = np.asarray(true_counts)
        if t.shape != self.counts.shape or not np.issubdtype(t.dtype, np.integer) or (t < 0).any():
            raise ValueError(f"true_counts must be non-negative integers of shape {self.counts.shape}; got {t.dtype} {t.shape}")
        tot = t.sum(1)
        keep = (self.n > 0) & (tot > 0)
        return CoverStats.from_fractions(t[keep] / tot[keep, None].astype(np.float64), p[keep])


def _is_tensor(x) -> bool:
    try:
        import torch
        return isinstance(x, torch.Tensor)
    except ImportError:
        return False


def estimate_cover(model, data, group_offsets, train_prior=None, strength: float = 1.0, iters: int = 20, k: int = 0,
                   views_per_point: int = 1) -> CoverEstimate:
    """``estimate_cover(predictor, feats | FeatureSet, group_offsets, ...)`` or ``estimate_cover(proba, None, group_offsets, ...)``.

    ``predictor``: a ``Predictor`` (or its ``DeviceHead``); ``feats``: (n_points * G, input_dim) float32, numpy (host) or a cuda
    tensor on the head's device, or a ``FeatureSet`` whose rows are read in place; G = ``views_per_point`` rows per point (their
    mean probabilities are the point's).  ``proba``: (n, K) float32 calibrated probabilities made elsewhere, numpy or cuda tensor.
    ``group_offsets``: (n_groups + 1,) integers, group g owns points [offsets[g], offsets[g + 1]).  ``train_prior``: (K,) class
    frequencies the classifier was trained and calibrated on (``prior_from_labels``), None for uniform; ``strength``: the Dirichlet
    pseudo-count of the EM; ``iters``: its iterations (0 leaves ``train_prior``); ``k`` > 0 also ranks every point under its
    group's adapted prior.  Arguments are checked on the host before the device is touched."""
    lib = _lib.lib
    if isinstance(model, np.ndarray) or _is_tensor(model):
        if data is not None:
            raise ValueError("with probabilities as the first argument the second must be None")
        if views_per_point != 1:
            raise ValueError("views_per_point applies to features: probabilities are one row per point")
        on_device = not isinstance(model, np.ndarray)
        if on_device:
            import torch
            p = model.contiguous()
            if not p.is_cuda or p.dtype != torch.float32 or p.dim() != 2:
                raise ValueError(f"proba must be a float32 cuda tensor (n, K); got {p.dtype} {tuple(p.shape)}")
            device, ptr = p.device.index, p.data_ptr()
        else:
            p = np.ascontiguousarray(model, dtype=np.float32)
            if p.ndim != 2:
                raise ValueError(f"proba must be (n, K); got {p.shape}")
            device, ptr = 0, p.ctypes.data
        n, K = int(p.shape[0]), int(p.shape[1])
        if K < 1:
            raise ValueError("proba has no classes")
        classes: Sequence = list(range(K))
        off, tp, strength, iters, kk = check_cover_arguments(n, K, group_offsets, train_prior, strength, iters, k)

        def call(common):
            return lib().mmc_cover_proba(ptr, n, K, *common, device, (0 if on_device else _lib.MMC_IN_HOST) | _lib.MMC_OUT_HOST,
                                         _current_stream_ptr(device))
    else:
        head = getattr(model, "_head", model)
        if not hasattr(head, "_h") or not hasattr(head, "n_classes"):
            raise TypeError("the first argument must be a Predictor, a DeviceHead or an (n, K) array of probabilities")
        K = head.n_classes
        classes = list(getattr(model, "classes", range(K)))
        device = head.device_index
        if isinstance(data, FeatureSet):
            if data.dim != head.input_dim:
                raise ValueError(f"the feature set has {data.dim} features, the head expects {head.input_dim}")
            if data.device_index != device:
                raise ValueError(f"the feature set is on device {data.device_index}, the head on device {device}")
            rows = len(data)
            g = check_views_per_point(rows, views_per_point)
            n = rows // g
            off, tp, strength, iters, kk = check_cover_arguments(n, K, group_offsets, train_prior, strength, iters, k)

            def call(common):
                return lib().mmc_head_cover_set(head._h, data._handle(), 0, n, g, *common, _lib.MMC_OUT_HOST, _current_stream_ptr(device))
        else:
            x, ptr, rows, flags, _ = head._input(data)
            g = check_views_per_point(rows, views_per_point)
            n = rows // g
            off, tp, strength, iters, kk = check_cover_arguments(n, K, group_offsets, train_prior, strength, iters, k)

            def call(common):
                return lib().mmc_head_cover(head._h, ptr, n, g, *common, (flags & _lib.MMC_IN_HOST) | _lib.MMC_OUT_HOST,
                                            _current_stream_ptr(device))
    n_groups = off.size - 1
    counts = np.zeros((n_groups, K), np.int64)
    soft = np.zeros((n_groups, K), np.int64)
    unusable = np.zeros((n_groups,), np.int64)
    prior = np.zeros((n_groups, K), np.float64)
    idx = np.zeros((n, kk), np.int32) if kk else None
    scores = np.zeros((n, kk), np.float32) if kk else None
    common = (off.ctypes.data, n_groups, None if tp is None else tp.ctypes.data, strength, iters, counts.ctypes.data, soft.ctypes.data,
              unusable.ctypes.data, prior.ctypes.data, kk, None if idx is None else idx.ctypes.data,
              None if scores is None else scores.ctypes.data)
    _lib.check(call(common))
    topk = PointPredictions(None, idx, scores, classes) if kk else None
    return CoverEstimate(counts, soft, unusable, np.diff(off), prior, topk)


def image_groups(points_per_image: Sequence[int], group_of_image=None):
    """The groups of ``PointClassifier.cover_images`` -> (offsets int64 (n_groups + 1,), group ids): one group per image, or, with
    ``group_of_image`` (one id per image), one group per run of consecutive images that share an id (a transect, a source).  An id
    that comes back after another one is a ValueError: groups are contiguous."""
    sizes = [int(s) for s in points_per_image]
    if group_of_image is None:
        ids: List = list(range(len(sizes)))
        return np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]).astype(np.int64), ids
    gids = list(group_of_image)
    if len(gids) != len(sizes):
        raise ValueError(f"group_of_image has {len(gids)} entries for {len(sizes)} images")
    offsets, ids, seen, at = [0], [], set(), 0
    for i, (gid, s) in enumerate(zip(gids, sizes)):
        if ids and gid == ids[-1]:
            offsets[-1] = at + s
        else:
            if gid in seen:
                raise ValueError(f"group_of_image[{i}] = {gid!r} comes back after another id: the images of a group must be consecutive")
            seen.add(gid)
            ids.append(gid)
            offsets.append(at + s)
        at += s
    return np.asarray(offsets, np.int64), ids
