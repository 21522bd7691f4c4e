"""Head ensembles: M calibrated heads on one class list, scored together on the device (include/mmc.h, "head ensembles").

``train_sweep`` leaves up to 16 trained, early-stopped and Platt-calibrated heads, and ``rank_sweep`` orders them; a
``HeadEnsemble`` keeps the best M instead of the best one.  Per point the prediction is the fp32 mean of the members' calibrated
probabilities (left to right in member order; with ``views_per_point`` first the views definition per member), ranked as
``DeviceHead.topk`` ranks; beside it come the predictive entropy, the members' expected entropy, their mutual information (the
disagreement) and the number of members that vote for the ensemble's best class.  The members' Linear layers run as one launch
per layer, and no member's N x K probabilities are written.
"""

from __future__ import annotations

import ctypes as C
import json
from pathlib import Path
from typing import Any, Dict, List, NamedTuple, Optional, Sequence

import numpy as np

from . import _lib
from .backbone import _current_stream_ptr, check_views_per_point
from .calibration import CalibratedMLP, export_artifact
from .featureset import FeatureSet
from .inference import ManifestError, Predictor, load_predictor
from .validation import MAX_ROWS_PER_CALL, Validation, _Outputs, _prepare, _ptr, _set_labels, validate

__all__ = ["HeadEnsemble", "Uncertainty", "EnsembleValidation", "ensemble_validate", "export_ensemble", "load_ensemble",
           "risk_coverage", "select_from_ranking", "ENSEMBLE_FORMAT_VERSION"]

ENSEMBLE_FORMAT_VERSION = 1
ENSEMBLE_MANIFEST = "ensemble.json"


class Uncertainty(NamedTuple):
    """Per point: ``entropy`` H(e) and ``expected_entropy`` (1/M) sum_j H(m_j) in nats (float32), ``mutual_information`` = their
    difference clamped at 0 (the members' disagreement), ``votes`` = members whose own best class is the ensemble's (int32)."""
    entropy: np.ndarray
    expected_entropy: np.ndarray
    mutual_information: np.ndarray
    votes: np.ndarray


def _uncertainty(stats, votes) -> Uncertainty:
    if isinstance(stats, np.ndarray):
        return Uncertainty(stats[:, 0].copy(), stats[:, 1].copy(), np.maximum(stats[:, 2], np.float32(0)), votes)
    return Uncertainty(stats[:, 0], stats[:, 1], stats[:, 2].clamp_min(0), votes)


def _member_parts(i: int, member):
    if isinstance(member, CalibratedMLP):
        return member.classes_.tolist(), member.n_features_in_
    if isinstance(member, Predictor):
        return list(member.classes), int(member.input_dim)
    raise ValueError(f"member {i} must be a CalibratedMLP or a Predictor, got {type(member).__name__}")


def select_from_ranking(ranking: Sequence[Dict[str, Any]], top: int) -> List[int]:
    """The ``config`` indices of the ``top`` best rows of a ``rank_sweep`` table (it is sorted best first)."""
    if isinstance(top, bool) or int(top) != top or not 1 <= top <= _lib.MMC_ENSEMBLE_MAX:
        raise ValueError(f"top must be an integer in [1, {_lib.MMC_ENSEMBLE_MAX}]; got {top!r}")
    if top > len(ranking):
        raise ValueError(f"top = {top} members from a sweep of {len(ranking)} configurations")
    return [int(row["config"]) for row in ranking[: int(top)]]


class HeadEnsemble:
    """``members``: 1 .. 16 ``CalibratedMLP`` and / or ``Predictor`` objects with equal class lists in equal order and equal input
    widths (depths and hidden widths are free).  The device handle is made on first use; the members' own heads stay usable."""

    def __init__(self, members: Sequence[Any]):
        members = list(members)
        if not 1 <= len(members) <= _lib.MMC_ENSEMBLE_MAX:
            raise ValueError(f"an ensemble has 1 .. {_lib.MMC_ENSEMBLE_MAX} members; got {len(members)}")
        classes, dim = _member_parts(0, members[0])
        for i, m in enumerate(members[1:], 1):
            ci, di = _member_parts(i, m)
            if len(ci) != len(classes):
                raise ValueError(f"member {i} has {len(ci)} classes, member 0 has {len(classes)}")
            for pos, (a, b) in enumerate(zip(classes, ci)):
                if a != b:
                    raise ValueError(f"member {i}'s class {pos} is {b!r}, member 0's is {a!r}: class lists must be equal, in equal order")
            if di != dim:
                raise ValueError(f"member {i} takes {di} features, member 0 takes {dim}")
        if len(classes) > _lib.MMC_ENSEMBLE_MAX_CLASSES:
            raise ValueError(f"{len(classes)} classes: an ensemble takes at most {_lib.MMC_ENSEMBLE_MAX_CLASSES}")
        self.members = members
        self.classes = classes
        self.input_dim = int(dim)
        self.ranking: Optional[List[Dict[str, Any]]] = None
        self._h = None
        self._heads: List[Any] = []

    @classmethod
    def from_sweep(cls, results, val, top: int, image_sizes=None) -> "HeadEnsemble":
        """The ``top`` best configurations of ``results`` (what ``train_sweep`` returned) by ``rank_sweep``'s order on ``val``; the
        whole table is kept as ``.ranking``."""
        from .sweep import rank_sweep
        results = list(results)
        ranking = rank_sweep(results, val, image_sizes=image_sizes)
        ens = cls([results[i][0] for i in select_from_ranking(ranking, top)])
        ens.ranking = ranking
        return ens

    # sklearn-style aliases, as on Predictor / CalibratedMLP
    @property
    def classes_(self) -> List[Any]:
        return self.classes

    def __len__(self) -> int:
        return len(self.members)

    def _heads_of_members(self):
        return [m._device_head() if isinstance(m, CalibratedMLP) else m._head for m in self.members]

    def _handle(self):
        if self._h is None:
            self._heads = self._heads_of_members()      # kept alive: the library borrows them
            arr = (C.c_void_p * len(self._heads))(*[h._h.value for h in self._heads])
            h = C.c_void_p()
            _lib.check(_lib.lib().mmc_ensemble_create(arr, len(self._heads), C.byref(h)))
            self._h = h
            self.device_index = self._heads[0].device_index
        return self._h

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().mmc_ensemble_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _run(self, feats, k: int, views_per_point: int, want_proba: bool, want_stats: bool):
        h = self._handle()
        x, ptr, n, flags, alloc = self._heads[0]._input(feats)
        g = check_views_per_point(n, views_per_point)
        m, K = n // g, len(self.classes)
        (idx, ip), (scores, sp) = alloc((m, k), "int32"), alloc((m, k), "float32")
        proba, pp = alloc((m, K), "float32") if want_proba else (None, None)
        (stats, tp), (votes, vp) = (alloc((m, _lib.MMC_ENSEMBLE_STATS), "float32"), alloc((m,), "int32")) if want_stats else ((None, None),) * 2
        if m:
            _lib.check(_lib.lib().mmc_ensemble_topk(h, ptr, m, g, k, ip, sp, pp, tp, vp, flags, _current_stream_ptr(self.device_index)))
        return idx, scores, proba, stats, votes

    def topk(self, feats, k: int, views_per_point: int = 1, want_proba: bool = False):
        """The k best classes of the ensemble mean per point: ``feats`` (N, input_dim) float32, numpy (host) or a cuda tensor, as
        ``DeviceHead.topk`` takes them.  -> (idx (N/G, k) int32, scores (N/G, k) float32[, proba (N/G, K) float32])."""
        k = int(k)
        if not 1 <= k <= len(self.classes):
            raise ValueError(f"k = {k} is outside [1, {len(self.classes)}]")
        idx, scores, proba, _, _ = self._run(feats, k, views_per_point, want_proba, False)
        return (idx, scores, proba) if want_proba else (idx, scores)

    def uncertainty(self, feats, views_per_point: int = 1) -> Uncertainty:
        _, _, _, stats, votes = self._run(feats, 1, views_per_point, False, True)
        return _uncertainty(stats, votes)

    def _host_rows(self, X) -> np.ndarray:
        arr = np.asarray(X, dtype=np.float32)
        if arr.ndim != 2 or arr.shape[1] != self.input_dim:
            raise ValueError(f"features must be (N, {self.input_dim}); got {arr.shape}.")
        return arr

    def predict_proba(self, X) -> np.ndarray:
        """(N, K) float64: the ensemble mean, the values ``topk(..., want_proba=True)`` returns."""
        return self._run(self._host_rows(X), 1, 1, True, False)[2].astype(np.float64)

    def predict(self, X) -> List[Any]:
        idx = self._run(self._host_rows(X), 1, 1, False, False)[0]
        return [self.classes[i] for i in idx[:, 0].tolist()]


def risk_coverage(correct, uncertainty, levels) -> Dict[str, Any]:
    """Accuracy of the rows kept when the most uncertain are set aside.  Rows are ordered by ``uncertainty`` ascending with a stable
    sort (ties by row); coverage c keeps the first ceil(c n) of them (at least one).  -> ``{"coverage", "accuracy", "aurc"}``:
    the levels, the accuracy at each, and the area under accuracy against coverage (trapezoids over the given levels)."""
    correct = np.asarray(correct, dtype=np.float64)
    unc = np.asarray(uncertainty, dtype=np.float64)
    if correct.ndim != 1 or correct.shape != unc.shape or not len(correct):
        raise ValueError(f"correct {correct.shape} / uncertainty {unc.shape} must be equal, non-empty 1-D shapes")
    lv = np.asarray(levels, dtype=np.float64)
    if lv.ndim != 1 or not len(lv) or np.any(lv <= 0) or np.any(lv > 1) or np.any(np.diff(lv) <= 0):
        raise ValueError("levels must be increasing coverages in (0, 1]")
    order = np.argsort(unc, kind="stable")
    hits = np.concatenate([[0.0], np.cumsum(correct[order])])
    n = len(order)
    keep = np.maximum(1, np.ceil(lv * n - 1e-12).astype(np.int64))
    acc = hits[keep] / keep
    area = float(np.sum((acc[1:] + acc[:-1]) / 2 * np.diff(lv))) if len(lv) > 1 else float(acc[0])
    return {"coverage": lv, "accuracy": acc, "aurc": area}


class EnsembleValidation:
    """``validation``: a plain ``Validation`` of the ensemble mean; ``uncertainty``: per row (None without rows); ``members``: each
    member's ``validate(member, data, rows=False)``."""

    def __init__(self, validation: Validation, uncertainty: Optional[Uncertainty], members: List[Validation]):
        self.validation, self.uncertainty, self.members = validation, uncertainty, members

    def table(self) -> List[Dict[str, Any]]:
        """One row per member (``member`` = its position) plus the ensemble (``member`` = "ensemble"): accuracy, balanced accuracy,
        f1 macro, log-loss."""
        def row(name, v):
            cs = v.class_scores()
            return {"member": name, "accuracy": v.accuracy, "balanced_accuracy": cs.balanced_accuracy, "f1_macro": cs.f1_macro,
                    "log_loss": v.log_loss}
        return [row(j, v) for j, v in enumerate(self.members)] + [row("ensemble", self.validation)]

    def risk_coverage(self, by: str = "entropy", levels=None) -> Dict[str, Any]:
        """``risk_coverage`` over the scored rows (known class, finite probabilities), most certain first by ``by``: "entropy",
        "mutual_information", "votes" (fewer votes = less certain) or "score" (lower top score = less certain)."""
        v = self.validation
        if not v.has_rows or self.uncertainty is None:
            raise ValueError("risk_coverage needs the per-row values: ensemble_validate(..., rows=True)")
        u = self.uncertainty
        keys = {"entropy": lambda: u.entropy, "mutual_information": lambda: u.mutual_information,
                "votes": lambda: -u.votes.astype(np.float64), "score": lambda: -v.scores}
        if by not in keys:
            raise ValueError(f"by must be one of {sorted(keys)}; got {by!r}")
        key = np.asarray(keys[by](), dtype=np.float64)
        scored = (v.gt >= 0) & np.isfinite(v.scores) & np.isfinite(np.asarray(u.entropy, dtype=np.float64))
        lv = np.linspace(0.1, 1.0, 10) if levels is None else levels
        return risk_coverage((v.est == v.gt)[scored], key[scored], lv)


def ensemble_validate(ens: HeadEnsemble, data, *, rows: bool = True) -> EnsembleValidation:
    """``validate`` for an ensemble: ``data`` takes the forms ``validate`` takes, is checked the same way before the device is
    touched, and is scored with the ensemble mean (``mmc_ensemble_evaluate`` / ``_set``)."""
    if not isinstance(ens, HeadEnsemble):
        raise ValueError(f"ens must be a HeadEnsemble, got {type(ens).__name__}")
    if not isinstance(data, (FeatureSet, tuple, list)):
        data = list(data)   # an iterator of batches is walked once per model
    _, classes, sources = _prepare(ens.members[0], data, rows, True, "ensemble_validate")
    out = _Outputs(len(classes), rows)
    h = ens._handle()
    lib = _lib.lib()
    st = _current_stream_ptr(ens.device_index)
    stats_parts, votes_parts = [], []
    for src, yi, lmap in sources:
        map_args = (_ptr(lmap), 0 if lmap is None else len(lmap))
        for first in range(0, len(src), MAX_ROWS_PER_CALL):
            cur = min(MAX_ROWS_PER_CALL, len(src) - first)
            c = out.call(cur)
            stats = np.empty((cur, _lib.MMC_ENSEMBLE_STATS), np.float32) if rows else None
            votes = np.empty(cur, np.int32) if rows else None
            args = c.args[:4] + (_ptr(stats), _ptr(votes)) + c.args[4:]
            if yi is None:
                _lib.check(lib.mmc_ensemble_evaluate_set(h, src._handle(), first, cur, *map_args, *args, st))
                if rows:
                    c.gt = _set_labels(src, first, cur, lmap, st)
            else:
                ys = yi[first:first + cur]
                _lib.check(lib.mmc_ensemble_evaluate(h, src[first:first + cur].ctypes.data, ys.ctypes.data, cur, *map_args, *args,
                                                     _lib.MMC_IN_HOST, st))
                c.gt = ys if lmap is None else lmap[ys]
            if rows:
                stats_parts.append(stats)
                votes_parts.append(votes)
    unc = _uncertainty(np.concatenate(stats_parts), np.concatenate(votes_parts)) if rows else None
    return EnsembleValidation(out.result(classes), unc, [validate(m, data, rows=False) for m in ens.members])


def export_ensemble(ens: HeadEnsemble, output_dir, reference_features, **export_kwargs) -> Dict[str, Any]:
    """``member_00/``, ``member_01/``, ... through ``export_artifact`` (one standard model.pt + model.json each; ``export_kwargs``
    go to it) and ``ensemble.json``: format version, member directories in order, class list, input width.  Every member must be
    a ``CalibratedMLP``.  -> the manifest."""
    if not isinstance(ens, HeadEnsemble):
        raise ValueError(f"ens must be a HeadEnsemble, got {type(ens).__name__}")
    for i, m in enumerate(ens.members):
        if not isinstance(m, CalibratedMLP):
            raise ValueError(f"member {i} is a {type(m).__name__}: only CalibratedMLP members can be exported")
    out = Path(output_dir)
    names = [f"member_{i:02d}" for i in range(len(ens.members))]
    for name, m in zip(names, ens.members):
        export_artifact(m, out / name, reference_features, **export_kwargs)
    manifest = dict(format_version=ENSEMBLE_FORMAT_VERSION, members=names, classes=list(ens.classes), input_dim=ens.input_dim)
    (out / ENSEMBLE_MANIFEST).write_text(json.dumps(manifest, indent=2) + "\n")
    return manifest


def check_ensemble_dir(directory) -> Dict[str, Any]:
    """Reads and checks ``ensemble.json`` and the members' ``model.json`` files without touching the device -> the manifest.
    ``ManifestError`` for an unknown version, a member count outside 1 .. 16, a missing member, or a member whose class list or
    input width differs from the manifest's."""
    d = Path(directory)
    path = d / ENSEMBLE_MANIFEST
    if not path.is_file():
        raise ManifestError(f"{path} not found")
    manifest = json.loads(path.read_text())
    version = manifest.get("format_version")
    if version != ENSEMBLE_FORMAT_VERSION:
        raise ManifestError(f"ensemble.json format_version={version!r} is incompatible with this loader (expects {ENSEMBLE_FORMAT_VERSION}).")
    names, classes = manifest.get("members"), manifest.get("classes")
    if not isinstance(names, list) or not 1 <= len(names) <= _lib.MMC_ENSEMBLE_MAX:
        raise ManifestError(f"ensemble.json lists {len(names) if isinstance(names, list) else names!r} members: 1 .. {_lib.MMC_ENSEMBLE_MAX} expected")
    for name in names:
        for f in ("model.pt", "model.json"):
            if not (d / name / f).is_file():
                raise ManifestError(f"member {name!r}: {d / name / f} is missing")
        mj = json.loads((d / name / "model.json").read_text())
        if mj.get("classes") != classes:
            raise ManifestError(f"member {name!r}: its class list differs from ensemble.json's")
        if mj.get("input_dim") != manifest.get("input_dim"):
            raise ManifestError(f"member {name!r}: input_dim {mj.get('input_dim')!r} differs from ensemble.json's {manifest.get('input_dim')!r}")
    return manifest


def load_ensemble(directory, device="cuda") -> HeadEnsemble:
    """The directory ``export_ensemble`` wrote -> a ``HeadEnsemble`` of ``Predictor``s (``load_predictor`` per member, with its
    own checks).  The manifest is checked first (``check_ensemble_dir``), before the device is touched."""
    manifest = check_ensemble_dir(directory)
    d = Path(directory)
    return HeadEnsemble([load_predictor(d / name / "model.pt", d / name / "model.json", device=device) for name in manifest["members"]])
