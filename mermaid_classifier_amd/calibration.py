"""Evaluation, Platt calibration and export of a trained ``TorchMLPClassifier`` with the arithmetic on the MI355X.

Replaces the host steps the reference's ``MermaidTrainer`` takes after ``partial_fit`` (``mermaid_classifier/pyspacer/
trainer.py``), each fed there by ``predict_proba`` and sklearn on the host:

=====================================================  ===================================================================
reference                                              here
=====================================================  ===================================================================
``_calc_acc_batched`` (:295-307)                       ``evaluate(clf, data)[0]``
``_calc_acc_and_log_loss_batched`` (:309-342)          ``evaluate(clf, data)``
the same, plus the confusion-matrix scores of          ``evaluate_classes(clf, data)`` -> accuracy, log-loss and
``metrics/classification.py:171-302`` per epoch        ``ClassScores``
``_calibrate_in_batches`` (:344-396)                   ``calibrate(clf, data)`` -> ``CalibratedMLP`` (``.to_sklearn()`` gives
                                                       the ``CalibratedClassifierCV`` the reference returns)
``inference/export.py:24-94`` ``export_artifact``      ``export_artifact(calibrated, output_dir, reference_features)``
=====================================================  ===================================================================

``data`` is ``(X, y)`` or an iterable of ``(x, y)`` batches (what ``labels.load_data_in_batches`` yields); labels are mapped
through ``clf._labels_to_indices``.  Features never sit on the host beyond one batch.  ``data`` may also be a ``FeatureSet``
(featureset.py): the split is then read where it lies on the device (``mmc_trainer_evaluate_set_q32``, ``mmc_calibrator_add_set``),
with the same results as the host-fed route on the same rows.  The device side is csrc/calib.hip
(``mmc_trainer_evaluate``, ``mmc_calibrator_*``); the calibrated head is served by the existing ``mmc_head_*`` kernels
(``inference.DeviceHead``).  No sklearn in the path: ``to_sklearn`` imports it lazily for callers that store the sklearn object.

Note: ``from __future__ import annotations`` must not appear here: ``torch.jit.script`` reads the head module's
``forward`` annotations at scripting time.
"""

import ctypes as C
import json
from importlib.metadata import PackageNotFoundError, version as _pkg_version
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from . import _lib
from .backbone import _current_stream_ptr, _device_index
from .class_scores import ClassScores
from .featureset import FeatureSet
from .inference import SCHEMA_VERSION, TASK_NAME, DeviceHead, HeadParams, Predictor

__all__ = ["evaluate", "evaluate_classes", "calibrate", "CalibratedMLP", "export_artifact", "build_head_module", "ParityError"]


class ParityError(Exception):
    """The frozen graph of ``export_artifact`` diverges from ``CalibratedMLP.predict_proba`` beyond ``tol``."""


def _batches(data):
    """(X, y) -> one batch; anything else is iterated as (x, y) batches."""
    if isinstance(data, tuple) and len(data) == 2 and not isinstance(data[0], tuple):
        x0 = np.asarray(data[0])
        if x0.ndim == 2:
            yield data[0], data[1]
            return
    for x, y in data:
        yield x, y


def _batch_arrays(clf, x, y) -> Tuple[np.ndarray, np.ndarray]:
    X = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    if X.ndim != 2:
        raise ValueError(f"X must be 2D, got shape {X.shape}")
    if X.shape[1] != clf.n_features_in_:
        raise ValueError(f"X has {X.shape[1]} features, expected {clf.n_features_in_}")
    yi = np.ascontiguousarray(clf._labels_to_indices(np.asarray(y)).astype(np.int32))
    if yi.shape != (X.shape[0],):
        raise ValueError(f"y has shape {yi.shape}, expected ({X.shape[0]},)")
    return X, yi


def _require_fitted(clf) -> None:
    if not clf._fitted():
        raise RuntimeError("classifier not fitted: train it with partial_fit or fit first")


def evaluate(clf, data) -> Tuple[float, float]:
    """-> (accuracy, log_loss) of ``clf.predict_proba`` over every row of ``data``: ``accuracy_score`` and
    ``sklearn.metrics.log_loss(y, proba, labels=clf.classes_)`` as the reference computes them per epoch, on the device.
    The per-batch log-loss sums come back as 2^-32 fixed point and are added as integers, so the result does not depend on
    how the rows are split into batches."""
    _require_fitted(clf)
    lib = _lib.lib()
    st = _current_stream_ptr(_device_index(clf.device))
    n = correct = loss_q32 = 0
    if isinstance(data, FeatureSet):
        data._check_against(clf)
        n = len(data)
        if n:
            nc, q = C.c_int64(0), C.c_int64(0)
            _lib.check(lib.mmc_trainer_evaluate_set_q32(clf._h, data._handle(), 0, n, C.byref(nc), C.byref(q), st))
            correct, loss_q32 = int(nc.value), int(q.value)
        data = ()   # nothing left to stream
    for x, y in _batches(data):
        X, yi = _batch_arrays(clf, x, y)
        nc, q = C.c_int64(0), C.c_int64(0)
        _lib.check(lib.mmc_trainer_evaluate_q32(clf._h, X.ctypes.data, yi.ctypes.data, X.shape[0], C.byref(nc), C.byref(q), st))
        n += X.shape[0]
        correct += int(nc.value)
        loss_q32 += int(q.value)
    if n == 0:
        raise ValueError("evaluate: no rows")
    return correct / n, loss_q32 / (n << 32)   # int / int: one correctly rounded division


def evaluate_classes(clf, data) -> Tuple[float, float, ClassScores]:
    """-> (accuracy, log_loss, ``ClassScores``): ``evaluate(clf, data)`` -- the same two floats, from the same integers -- plus the
    K x K table of (true class, argmax) counts of the same pass (``mmc_trainer_evaluate_classes``, ``_set`` for a
    ``FeatureSet``), wrapped as ``ClassScores``: balanced accuracy, macro precision / recall / f1 and MCC of the uncalibrated
    classifier, which the reference computes once after training (metrics/classification.py:171-302) and a sweep wants per epoch.
    The tables of the batches are added as integers."""
    _require_fitted(clf)
    lib = _lib.lib()
    st = _current_stream_ptr(_device_index(clf.device))
    K = len(clf.classes_)
    n = correct = loss_q32 = 0
    table = np.zeros((K, K), np.int64)
    part = np.zeros((K, K), np.int64)
    if isinstance(data, FeatureSet):
        data._check_against(clf)
        n = len(data)
        if n:
            nc, q = C.c_int64(0), C.c_int64(0)
            _lib.check(lib.mmc_trainer_evaluate_classes_set(clf._h, data._handle(), 0, n, C.byref(nc), C.byref(q), table.ctypes.data, st))
            correct, loss_q32 = int(nc.value), int(q.value)
        data = ()   # nothing left to stream
    for x, y in _batches(data):
        X, yi = _batch_arrays(clf, x, y)
        nc, q = C.c_int64(0), C.c_int64(0)
        _lib.check(lib.mmc_trainer_evaluate_classes(clf._h, X.ctypes.data, yi.ctypes.data, X.shape[0], C.byref(nc), C.byref(q),
                                                    part.ctypes.data, st))
        n += X.shape[0]
        correct += int(nc.value)
        loss_q32 += int(q.value)
        table += part
    if n == 0:
        raise ValueError("evaluate_classes: no rows")
    return correct / n, loss_q32 / (n << 32), ClassScores(table, clf.classes_)


class _Calibrator:
    """mmc_calibrator_* handle wrapper (device-resident probability store + per-class Platt fit)."""

    def __init__(self, n_classes: int, device=0):
        self.device_index = _device_index(device)
        self.n_classes = int(n_classes)
        self._h = C.c_void_p()
        _lib.check(_lib.lib().mmc_calibrator_create(self.n_classes, self.device_index, C.byref(self._h)))

    def add_features(self, clf, X: np.ndarray, y_idx: np.ndarray) -> None:
        _lib.check(_lib.lib().mmc_calibrator_add_features(self._h, clf._h, X.ctypes.data, y_idx.ctypes.data, X.shape[0],
                                                          _current_stream_ptr(self.device_index)))

    def add_set(self, clf, fs: FeatureSet) -> None:
        _lib.check(_lib.lib().mmc_calibrator_add_set(self._h, clf._h, fs._handle(), 0, len(fs), _current_stream_ptr(self.device_index)))

    def add_scores(self, scores, y_idx) -> None:
        S = np.ascontiguousarray(np.asarray(scores, dtype=np.float64))
        yi = np.ascontiguousarray(np.asarray(y_idx, dtype=np.int32))
        if S.ndim != 2 or S.shape[1] != self.n_classes or yi.shape != (S.shape[0],):
            raise ValueError(f"scores must be (N, {self.n_classes}) with N labels; got {S.shape} and {yi.shape}")
        _lib.check(_lib.lib().mmc_calibrator_add_scores(self._h, S.ctypes.data, yi.ctypes.data, S.shape[0],
                                                        _current_stream_ptr(self.device_index)))

    def fit(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        a = np.empty(self.n_classes, np.float64)
        b = np.empty(self.n_classes, np.float64)
        it = np.empty(self.n_classes, np.int32)
        _lib.check(_lib.lib().mmc_calibrator_fit(self._h, a.ctypes.data, b.ctypes.data, it.ctypes.data,
                                                 _current_stream_ptr(self.device_index)))
        return a, b, it

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            _lib.lib().mmc_calibrator_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CalibratedMLP:
    """A ``TorchMLPClassifier`` plus one Platt sigmoid per class: ``CalibratedClassifierCV(clf, cv="prefit",
    method="sigmoid")`` of the reference, served by the device head.

    Holds a snapshot of the classifier's parameters taken at calibration time: later ``partial_fit`` calls on the classifier
    do not change it.  ``a_`` / ``b_`` are float64 (calibrated p_k = 1 / (1 + exp(a_k p_k + b_k)), row-normalised);
    ``iterations_`` counts the Newton trial points of each class's fit."""

    def __init__(self, weights: List[np.ndarray], biases: List[np.ndarray], classes, a, b, iterations=None, device=0,
                 clf_state: Optional[Dict[str, Any]] = None):
        self.weights = [np.array(w, dtype=np.float32) for w in weights]
        self.biases = [np.array(v, dtype=np.float32) for v in biases]
        self.classes_ = np.asarray(classes)
        self.a_ = np.asarray(a, dtype=np.float64)
        self.b_ = np.asarray(b, dtype=np.float64)
        self.iterations_ = None if iterations is None else np.asarray(iterations, dtype=np.int32)
        self.device = device
        self._clf_state = clf_state
        if len(self.classes_) < 3 or self.a_.shape != (len(self.classes_),) or self.b_.shape != self.a_.shape:
            raise ValueError(f"need K >= 3 classes and K calibrators; got {len(self.classes_)} classes, a {self.a_.shape}, b {self.b_.shape}")
        self._head = None
        self.logit_scaling_ = None   # the LogitScaling folded into the last layer, when calibrate() was given one

    @property
    def n_features_in_(self) -> int:
        return int(self.weights[0].shape[1])

    def head_params(self) -> HeadParams:
        return HeadParams(self.weights, self.biases, self.a_, self.b_)

    def _device_head(self) -> DeviceHead:
        if self._head is None:
            self._head = DeviceHead(self.head_params(), device=self.device)
        return self._head

    def predict_proba(self, X) -> np.ndarray:
        arr = np.asarray(X, dtype=np.float32)
        if arr.ndim != 2 or arr.shape[1] != self.n_features_in_:
            raise ValueError(f"X must be (N, {self.n_features_in_}); got {arr.shape}.")
        proba, _ = self._device_head().predict(arr, want_argmax=False)
        return proba.astype(np.float64)

    def predict(self, X) -> np.ndarray:
        arr = np.asarray(X, dtype=np.float32)
        if arr.ndim != 2 or arr.shape[1] != self.n_features_in_:
            raise ValueError(f"X must be (N, {self.n_features_in_}); got {arr.shape}.")
        _, arg = self._device_head().predict(arr, want_argmax=True)
        return self.classes_[arg]

    def predictor(self) -> Predictor:
        """The served form (``inference.Predictor``) without a round trip through files."""
        return Predictor(self._device_head(), self.classes_.tolist(), self.n_features_in_)

    def folded(self, transform) -> "CalibratedMLP":
        """This model, trained on ``transform``'s output, as a model of RAW features: ``transform.fold`` of the first Linear
        layer (``feature_transform.FeatureTransform.fold``), the same ``a_`` / ``b_`` / ``classes_``, ``n_features_in_ ==
        transform.dim``.  The classifier state is dropped -- its sklearn twin would take transformed features -- so ``to_sklearn``
        raises on the result.  The transform is kept as ``transform_``."""
        if transform.n_components != self.n_features_in_:
            raise ValueError(f"the transform writes {transform.n_components} features, this model takes {self.n_features_in_}")
        weights, biases = transform.fold(self.weights, self.biases)
        out = CalibratedMLP(weights, biases, self.classes_, self.a_, self.b_, self.iterations_, device=self.device, clf_state=None)
        out.transform_ = transform
        out.logit_scaling_ = self.logit_scaling_
        return out

    def to_sklearn(self):
        """-> ``CalibratedClassifierCV(clf, cv="prefit")`` carrying ``_SigmoidCalibration`` objects with ``a_`` / ``b_``: the
        object the reference's ``_calibrate_in_batches`` returns (trainer.py:385-396).  ``clf`` is a ``TorchMLPClassifier``
        rebuilt from this snapshot (its Adam state starts from zero).  Imports sklearn."""
        import warnings
        from sklearn.calibration import CalibratedClassifierCV, _CalibratedClassifier, _SigmoidCalibration
        from .torch_classifier import TorchMLPClassifier
        if self._clf_state is None:
            raise RuntimeError("to_sklearn needs the classifier this model was calibrated from (use calibrate())")
        clf = TorchMLPClassifier.__new__(TorchMLPClassifier)
        clf.__setstate__({**self._clf_state, "_module_state": ([w.copy() for w in self.weights], [v.copy() for v in self.biases])})
        calibrators = []
        for a, b in zip(self.a_, self.b_):
            cal = _SigmoidCalibration()
            cal.a_, cal.b_ = float(a), float(b)
            calibrators.append(cal)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", FutureWarning)   # cv="prefit" is deprecated in newer sklearn; the reference uses it
            wrapper = CalibratedClassifierCV(clf, cv="prefit")
        wrapper.calibrated_classifiers_ = [_CalibratedClassifier(clf, calibrators, method="sigmoid", classes=clf.classes_)]
        wrapper.classes_ = clf.classes_
        return wrapper


def calibrate(clf, data, logit_scaling=None) -> CalibratedMLP:
    """Platt calibration of ``clf`` on the ref split ``data`` (the reference's ``_calibrate_in_batches``): every batch goes
    through the classifier's current parameters into the device-resident probability store, then all K sigmoids are fitted
    at once.  Raises ``RuntimeError`` for an unfitted classifier and ``ValueError`` for fewer than 3 classes.

    ``logit_scaling``: a fitted ``logit_scaling.LogitScaling``, or a kind string (``"temperature"`` / ``"bias"`` / ``"vector"``) that is
    fitted on ``data`` first (``data`` is then read twice: not a one-shot generator).  It is folded into the last layer before the
    Platt fit, which runs on the folded classifier's probabilities; the returned model holds the folded snapshot and the scaling as
    ``logit_scaling_``.  ``None`` is the path above, call for call."""
    _require_fitted(clf)
    K = len(clf.classes_)
    if K < 3:
        raise ValueError(f"calibrate: {K} classes; one Platt sigmoid per class is defined here for K >= 3 only")
    if isinstance(data, FeatureSet):
        data._check_against(clf)
    if logit_scaling is not None:
        from . import logit_scaling as _ls
        scaling = _ls.resolve(logit_scaling, clf, data)
        out = calibrate(scaling.fold_classifier(clf), data)
        out.logit_scaling_ = scaling
        return out
    weights, biases = clf.parameters()   # the snapshot (read before the forward passes: the same parameters)
    cal = _Calibrator(K, clf.device)
    try:
        if isinstance(data, FeatureSet):
            cal.add_set(clf, data)
            data = ()   # nothing left to stream
        for x, y in _batches(data):
            X, yi = _batch_arrays(clf, x, y)
            cal.add_features(clf, X, yi)
        a, b, it = cal.fit()
    finally:
        cal.close()
    state = {k: v for k, v in clf.__dict__.items() if k != "_h"}
    state["loss_curve_"] = list(clf.loss_curve_)
    return CalibratedMLP(weights, biases, clf.classes_, a, b, it, device=clf.device, clf_state=state)


# ---- TorchScript artifact -------------------------------------------------------------------------------------------------
# manifest "config" when the caller passes none: the patch edge the features were extracted at (include/mmc.h MMC_PATCH)
DEFAULT_CONFIG = {"patch_size": 224}


def build_head_module(weights, biases, a, b):
    """-> the frozen TorchScript graph that ``model.pt`` holds, written from the formula of the calibrated head:

        p = softmax(MLP(x))                    MLP = Linear, then (ReLU, Linear) per further layer
        q_k = sigmoid(-(a_k p_k + b_k))        one Platt sigmoid per class
        q = q / sum_k q_k                      a row whose q sums to 0 becomes uniform, 1 / K
        q = 1 where 1 < q <= 1 + 1e-5          the overshoot clip

    fp32 throughout (a / b rounded to float32).  Freezing turns every parameter into a graph constant, which is what
    ``inference.params_from_torchscript`` reads back."""
    import torch
    from torch import nn

    def f32(v):
        return torch.tensor(np.asarray(v, dtype=np.float32))

    stages = []
    for i, (w, v) in enumerate(zip(weights, biases)):
        if i:
            stages.append(nn.ReLU())
        lin = nn.Linear(w.shape[1], w.shape[0])
        lin.weight = nn.Parameter(f32(w), requires_grad=False)
        lin.bias = nn.Parameter(f32(v), requires_grad=False)
        stages.append(lin)

    class PlattHead(nn.Module):
        def __init__(self):
            super().__init__()
            self.mlp = nn.Sequential(*stages)
            self.register_buffer("slope", f32(a))
            self.register_buffer("intercept", f32(b))

        def forward(self, x: torch.Tensor) -> torch.Tensor:
            p = torch.softmax(self.mlp(x), dim=1)
            q = torch.sigmoid(torch.neg(self.slope * p + self.intercept))
            total = torch.sum(q, dim=1, keepdim=True)
            q = torch.where(total > 0.0, q / total, torch.full_like(q, 1.0 / q.size(1)))
            return q.masked_fill((q > 1.0) & (q <= 1.0 + 1e-5), 1.0)

    return torch.jit.freeze(torch.jit.script(PlattHead().eval()))


def _installed(dist: str) -> Optional[str]:
    try:
        return _pkg_version(dist)
    except PackageNotFoundError:
        return None


def _graph_gap(graph, calibrated: "CalibratedMLP", features) -> float:
    """max |graph(features) - calibrated.predict_proba(features)| over every element."""
    import torch
    feats = np.ascontiguousarray(features, dtype=np.float32)
    served = calibrated.predict_proba(feats)
    with torch.no_grad():
        scripted = graph(torch.as_tensor(feats)).double().numpy()
    return float(np.abs(scripted - served).max())


def export_artifact(calibrated: CalibratedMLP, output_dir, reference_features, *, config: Optional[Dict[str, Any]] = None,
                    task: str = TASK_NAME, tol: float = 1e-6) -> Tuple[Path, Dict[str, Any], float]:
    """Write ``output_dir/model.pt`` (``build_head_module``'s graph) and ``output_dir/model.json`` (the keys
    ``load_predictor`` and the reference's loader read) for ``calibrated``.  The graph must reproduce
    ``calibrated.predict_proba`` on ``reference_features`` within ``tol``, or ``ParityError`` is raised and nothing is
    written.  -> (path of model.pt, manifest, the measured gap).  ``trained_with`` records the installed torch / sklearn /
    pyspacer versions (``None`` for an absent package): no sklearn version is required, since sklearn fits nothing here."""
    import torch
    graph = build_head_module(calibrated.weights, calibrated.biases, calibrated.a_, calibrated.b_)
    gap = _graph_gap(graph, calibrated, reference_features)
    if not gap <= tol:
        raise ParityError(f"export_artifact: the TorchScript head is {gap:.3e} away from the device head on the reference "
                          f"features (allowed {tol:.1e}); no files written")
    manifest = dict(schema_version=SCHEMA_VERSION, task=task, classes=calibrated.classes_.tolist(),
                    input_dim=calibrated.n_features_in_, config=dict(DEFAULT_CONFIG) if config is None else config,
                    trained_with={"torch": torch.__version__, "sklearn": _installed("scikit-learn"),
                                  "pyspacer": _installed("pyspacer")})
    out = Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    pt_path, json_path = out / "model.pt", out / "model.json"
    graph.save(str(pt_path))
    json_path.write_text(json.dumps(manifest, indent=2) + "\n")
    return pt_path, manifest, gap
