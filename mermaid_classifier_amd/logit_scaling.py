"""Logit calibration of a trained ``TorchMLPClassifier`` on the MI355X: temperature, bias and vector scaling.

The reference's balancing study ends on "Platt-scaling parameters or temperature scaling on top of it should be investigated"
(``docs/research/balancing-experiments.md:142``).  ``logit_prior`` (``mmc_trainer_set_loss``) is the training-time half of that
line; this module is the test-time half.  All three maps are affine in the logits, ``z' = a * z + c``:

=================  ========================================  ==========
``kind``           parameters                                free
=================  ========================================  ==========
``"temperature"``  ``a = 1 / T`` for every class, ``c = 0``  1
``"bias"``         ``a = 1``, ``c`` free                     K
``"vector"``       both free                                 2 K
=================  ========================================  ==========

so a fitted ``LogitScaling`` folds exactly into the last ``Linear`` layer (``fold``), as ``FeatureTransform.fold`` goes into the
first: ``model.pt`` / ``model.json``, ``Predictor``, ``PointClassifier``, every ``validate`` entry and ``export_artifact`` work on
the result unchanged, and the Platt stage (``calibration.calibrate``) still runs on top.  The definition, the objective and the step
rule are include/mmc.h, section "logit calibration"; the device side is csrc/logit_scaling.hip (one fp64 pass over the stored
logits: loss, gradient, Hessian), the Newton iteration csrc/logit_newton.h.  The rows never leave the device.  No gain on reef
data has been measured.
"""

from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .backbone import _current_stream_ptr, _device_index
from .featureset import FeatureSet

__all__ = ["LogitScaling", "fit_logit_scaling", "KINDS"]

KINDS = {"temperature": _lib.MMC_LOGITCAL_TEMPERATURE, "bias": _lib.MMC_LOGITCAL_BIAS, "vector": _lib.MMC_LOGITCAL_VECTOR}


def _check_fit_args(kind, l2, tol, max_trials) -> None:
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {sorted(KINDS)}, got {kind!r}")
    if not (np.isfinite(l2) and l2 >= 0.0):
        raise ValueError(f"l2 must be finite and >= 0, got {l2!r}")
    if not (np.isfinite(tol) and tol > 0.0):
        raise ValueError(f"tol must be finite and > 0, got {tol!r}")
    if int(max_trials) != max_trials or not 1 <= int(max_trials) <= 1000:
        raise ValueError(f"max_trials must be an integer in [1, 1000], got {max_trials!r}")


class LogitScaling:
    """``z' = a * z + c``.  ``kind``, ``a`` / ``c`` (K,) float64, ``frozen`` (K,) bool -- classes without a row, left at the identity
    --, ``nll_before`` / ``nll_after`` (mean log-loss of the raw and of the scaled logits on the fitting rows), ``trials`` (trial
    points evaluated), ``converged``, ``n_rows``.  Make one with ``fit_logit_scaling`` or from known parameters."""

    def __init__(self, kind: str, a, c, *, frozen=None, nll_before: Optional[float] = None, nll_after: Optional[float] = None,
                 trials: int = 0, converged: bool = True, n_rows: int = 0):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {sorted(KINDS)}, got {kind!r}")
        self.kind = kind
        self.a = np.array(a, dtype=np.float64)
        self.c = np.array(c, dtype=np.float64)
        if self.a.ndim != 1 or self.a.shape != self.c.shape or len(self.a) < 2:
            raise ValueError(f"a and c must be two (K,) vectors with K >= 2; got {self.a.shape} and {self.c.shape}")
        if not (np.isfinite(self.a).all() and np.isfinite(self.c).all()):
            raise ValueError("a / c must be finite")
        self.frozen = np.zeros(len(self.a), bool) if frozen is None else np.array(frozen, dtype=bool)
        if self.frozen.shape != self.a.shape:
            raise ValueError(f"frozen must be ({len(self.a)},), got {self.frozen.shape}")
        self.nll_before, self.nll_after = nll_before, nll_after
        self.trials, self.converged, self.n_rows = int(trials), bool(converged), int(n_rows)

    @property
    def n_classes(self) -> int:
        return len(self.a)

    @property
    def temperature(self) -> float:
        """T = 1 / a[0]; kind "temperature" only."""
        if self.kind != "temperature":
            raise AttributeError(f"a {self.kind!r} scaling has no single temperature")
        return 1.0 / float(self.a[0])

    def apply(self, logits) -> np.ndarray:
        """(N, K) logits -> ``a * z + c`` in float64."""
        z = np.asarray(logits, np.float64)
        if z.ndim != 2 or z.shape[1] != self.n_classes:
            raise ValueError(f"logits must be (N, {self.n_classes}); got {z.shape}")
        return self.a[None, :] * z + self.c[None, :]

    def fold(self, weights: Sequence[np.ndarray], biases: Sequence[np.ndarray]) -> Tuple[List[np.ndarray], List[np.ndarray]]:
        """Parameters of a head -> parameters of the head whose logits are ``a * z + c``: the last layer becomes
        ``float32(a[:, None] * float64(W))`` and ``float32(a * float64(b) + c)``, each rounded once; the other layers are copied."""
        W = np.asarray(weights[-1], np.float64)
        b = np.asarray(biases[-1], np.float64)
        if W.ndim != 2 or W.shape[0] != self.n_classes or b.shape != (self.n_classes,):
            raise ValueError(f"the last layer writes {W.shape[0] if W.ndim == 2 else W.shape} logits, the scaling has {self.n_classes}")
        Wf = (self.a[:, None] * W).astype(np.float32)
        bf = (self.a * b + self.c).astype(np.float32)
        return ([np.array(w, dtype=np.float32) for w in weights[:-1]] + [Wf],
                [np.array(v, dtype=np.float32) for v in biases[:-1]] + [bf])

    def fold_classifier(self, clf):
        """-> a ``TorchMLPClassifier`` copy of the fitted ``clf`` with the scaling folded into its last layer (rebuilt through
        ``__setstate__``, as ``CalibratedMLP.to_sklearn`` rebuilds one; its Adam moments start from zero)."""
        from .torch_classifier import TorchMLPClassifier
        if not clf._fitted():
            raise RuntimeError("classifier not fitted: train it with partial_fit or fit first")
        if len(clf.classes_) != self.n_classes:
            raise ValueError(f"the classifier has {len(clf.classes_)} classes, the scaling {self.n_classes}")
        weights, biases = self.fold(*clf.parameters())
        state = {k: v for k, v in clf.__dict__.items() if k != "_h"}
        state["loss_curve_"] = list(clf.loss_curve_)
        out = TorchMLPClassifier.__new__(TorchMLPClassifier)
        out.__setstate__({**state, "_module_state": (weights, biases)})
        return out

    def __repr__(self) -> str:
        return (f"LogitScaling(kind={self.kind!r}, K={self.n_classes}, nll {self.nll_before} -> {self.nll_after}, "
                f"trials={self.trials}, converged={self.converged})")


class _LogitCalibrator:
    """mmc_logitcal_* handle wrapper: the device-resident logit store, one pass of sums, the fit."""

    def __init__(self, n_classes: int, device=0):
        self.device_index = _device_index(device)
        self.n_classes = int(n_classes)
        self._h = C.c_void_p()
        _lib.check(_lib.lib().mmc_logitcal_create(self.n_classes, self.device_index, C.byref(self._h)))

    def _stream(self):
        return _current_stream_ptr(self.device_index)

    def __len__(self) -> int:
        return int(_lib.lib().mmc_logitcal_rows(self._h))

    def add_features(self, clf, X: np.ndarray, y_idx: np.ndarray) -> None:
        _lib.check(_lib.lib().mmc_logitcal_add_features(self._h, clf._h, X.ctypes.data, y_idx.ctypes.data, X.shape[0], self._stream()))

    def add_set(self, clf, fs: FeatureSet, first: int = 0, n: Optional[int] = None) -> None:
        n = len(fs) - int(first) if n is None else int(n)
        _lib.check(_lib.lib().mmc_logitcal_add_set(self._h, clf._h, fs._handle(), int(first), n, self._stream()))

    def add_logits(self, logits, y_idx) -> None:
        Z = np.ascontiguousarray(np.asarray(logits, dtype=np.float32))
        yi = np.ascontiguousarray(np.asarray(y_idx, dtype=np.int32))
        if Z.ndim != 2 or Z.shape[1] != self.n_classes or yi.shape != (Z.shape[0],):
            raise ValueError(f"logits must be (N, {self.n_classes}) with N labels; got {Z.shape} and {yi.shape}")
        _lib.check(_lib.lib().mmc_logitcal_add_logits(self._h, Z.ctypes.data, yi.ctypes.data, Z.shape[0], self._stream()))

    def stats(self, a, c, hess: bool = True):
        """-> (nll_sum, grad (2K), hess (2K, 2K) or None, counts (K,)) at (a, c)."""
        K = self.n_classes
        a = np.ascontiguousarray(np.asarray(a, np.float64))
        c = np.ascontiguousarray(np.asarray(c, np.float64))
        if a.shape != (K,) or c.shape != (K,):
            raise ValueError(f"a and c must be ({K},); got {a.shape} and {c.shape}")
        nll = C.c_double(0.0)
        grad = np.zeros(2 * K, np.float64)
        H = np.zeros((2 * K, 2 * K), np.float64) if hess else None
        counts = np.zeros(K, np.int64)
        _lib.check(_lib.lib().mmc_logitcal_stats(self._h, a.ctypes.data, c.ctypes.data, C.byref(nll), grad.ctypes.data,
                                                 H.ctypes.data if hess else None, counts.ctypes.data, self._stream()))
        return float(nll.value), grad, H, counts

    def fit(self, kind: str = "temperature", l2: float = 0.0, tol: float = 1e-9, max_trials: int = 100) -> LogitScaling:
        _check_fit_args(kind, l2, tol, max_trials)
        K = self.n_classes
        a, c = np.zeros(K, np.float64), np.zeros(K, np.float64)
        frozen = np.zeros(K, np.uint8)
        before, after = C.c_double(0.0), C.c_double(0.0)
        trials, converged = C.c_int32(0), C.c_int32(0)
        _lib.check(_lib.lib().mmc_logitcal_fit(self._h, KINDS[kind], float(l2), float(tol), int(max_trials), a.ctypes.data, c.ctypes.data,
                                               frozen.ctypes.data, C.byref(before), C.byref(after), C.byref(trials), C.byref(converged),
                                               self._stream()))
        return LogitScaling(kind, a, c, frozen=frozen.astype(bool), nll_before=float(before.value), nll_after=float(after.value),
                            trials=int(trials.value), converged=bool(converged.value), n_rows=len(self))

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            _lib.lib().mmc_logitcal_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fit_logit_scaling(clf, data, kind: str = "temperature", l2: float = 0.0, tol: float = 1e-9, max_trials: int = 100) -> LogitScaling:
    """Fit ``kind`` scaling of ``clf``'s raw logits on ``data``: a ``FeatureSet`` (read where it lies on the device) or what
    ``calibration.calibrate`` takes -- ``(X, y)`` or an iterable of ``(x, y)`` batches.  Minimises the log-loss of
    ``softmax(a * z + c)`` plus ``l2 * N / 2 * (|a - 1|^2 + |c|^2)`` by damped Newton steps on the device sums; stops at
    ``max |gradient| / N <= tol`` or after ``max_trials`` trial points (``converged`` says which).  Classes without a row stay at the
    identity (``frozen``).  Argument errors are raised before a device is touched."""
    from .calibration import _batch_arrays, _batches, _require_fitted
    _check_fit_args(kind, l2, tol, max_trials)
    _require_fitted(clf)
    K = len(clf.classes_)
    if not 2 <= K <= _lib.MMC_LOGITCAL_MAX_CLASSES:
        raise ValueError(f"logit scaling takes 2 to {_lib.MMC_LOGITCAL_MAX_CLASSES} classes, the classifier has {K}")
    if isinstance(data, FeatureSet):
        data._check_against(clf)
    cal = _LogitCalibrator(K, clf.device)
    try:
        if isinstance(data, FeatureSet):
            cal.add_set(clf, data)
            data = ()   # nothing left to stream
        for x, y in _batches(data):
            X, yi = _batch_arrays(clf, x, y)
            cal.add_features(clf, X, yi)
        if len(cal) == 0:
            raise ValueError("fit_logit_scaling: no rows")
        return cal.fit(kind, l2, tol, max_trials)
    finally:
        cal.close()


def check_argument(logit_scaling) -> None:
    """Raise ``ValueError`` unless ``logit_scaling`` is a kind string or a ``LogitScaling`` (before any training is done)."""
    if isinstance(logit_scaling, LogitScaling) or (isinstance(logit_scaling, str) and logit_scaling in KINDS):
        return
    raise ValueError(f"logit_scaling must be None, one of {sorted(KINDS)} or a LogitScaling, got {logit_scaling!r}")


def resolve(logit_scaling, clf, data) -> Optional[LogitScaling]:
    """The ``logit_scaling`` argument of ``calibrate`` / ``train_classifier`` -> a fitted ``LogitScaling`` or None: itself, or a kind
    string fitted on ``data``."""
    if logit_scaling is None or isinstance(logit_scaling, LogitScaling):
        return logit_scaling
    check_argument(logit_scaling)
    return fit_logit_scaling(clf, data, kind=logit_scaling)
