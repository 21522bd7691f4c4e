"""Distillation: a head ensemble (or any calibrated head) trained into one exportable head (include/mmc.h, "distillation").

The reference has no counterpart: its trainer knows hard labels only, and every artifact it reads or writes carries one
``Linear -> ReLU -> ... -> Linear`` stack, so a ``HeadEnsemble`` can be scored here but not shipped.  Distillation (Hinton et al.
2015) trains one head of that shape on the teacher's probabilities beside the labels.

``TargetSet``        an N x K float32 matrix of per-row class distributions resident on the device, row i belonging to row i of a
                     ``FeatureSet`` (``mmc_targetset_*``, csrc/targets.hip).  It never holds a row that is not a distribution.
``teacher_targets``  the teacher's calibrated probabilities of every row of a set, made on the device by
                     ``mmc_ensemble_predict_set``: the matrix never visits the host.
``distill``          ``train_classifier`` with the targets made for ``train``.

A student's loss per row is ``s_i [(1 - alpha) b_i + alpha tau^2 w_t k_i]``: ``b_i`` its own hard-label term, ``k_i`` the
cross-entropy between the teacher's row (softened by ``tau``) and the student's softmax at temperature ``tau``.
"""

from __future__ import annotations

import ctypes as C
from typing import Any, Optional

import numpy as np

from . import _lib
from .backbone import _current_stream_ptr, _device_index

__all__ = ["TargetSet", "teacher_targets", "distill"]


class TargetSet:
    """``TargetSet(classes, device=0, reserve_rows=0)``: rows of ``len(classes)`` float32 probabilities (``classes`` stored sorted
    and unique, as a ``FeatureSet``'s).  A row is valid when every entry is finite and >= 0 and the row sums to 1 within 1e-3; an
    ``append`` that holds an invalid row raises ``ValueError`` naming the first one and adds nothing."""

    def __init__(self, classes, device=0, reserve_rows: int = 0):
        self.classes = np.unique(np.asarray(classes))
        if self.classes.size < 1:
            raise ValueError("classes is empty")
        if isinstance(reserve_rows, bool) or int(reserve_rows) != reserve_rows or int(reserve_rows) < 0:
            raise ValueError(f"reserve_rows must be an integer >= 0, got {reserve_rows!r}")
        if int(reserve_rows) * len(self.classes) > _lib.MMC_TARGETSET_MAX_CELLS:
            raise ValueError(f"{reserve_rows} rows x {len(self.classes)} classes: a target set holds at most "
                             f"{_lib.MMC_TARGETSET_MAX_CELLS} cells")
        self.device = device
        self.device_index = _device_index(device)
        self._reserve = int(reserve_rows)
        self._h = None

    def _handle(self) -> C.c_void_p:
        if self._h is None:
            h = C.c_void_p()
            _lib.check(_lib.lib().mmc_targetset_create(len(self.classes), self.device_index, self._reserve, C.byref(h)))
            self._h = h
        return self._h

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().mmc_targetset_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        return 0 if self._h is None else int(_lib.lib().mmc_targetset_rows(self._h))

    def append(self, P) -> "TargetSet":
        """Rows ``P`` (n, K): a host array, or a contiguous float32 cuda tensor on the set's device (the rows stay there)."""
        K = len(self.classes)
        if not isinstance(P, np.ndarray) and type(P).__module__.startswith("torch") and getattr(P, "is_cuda", False):
            import torch
            if P.device.index != self.device_index:
                raise ValueError(f"P lives on {P.device}, the set on device {self.device_index}")
            if P.dtype != torch.float32 or P.dim() != 2 or P.shape[1] != K or not P.is_contiguous():
                raise ValueError(f"P must be a contiguous float32 tensor (n, {K}); got {P.dtype} {tuple(P.shape)}")
            ptr, n, flags = P.data_ptr(), int(P.shape[0]), _lib.MMC_IN_DEVICE
        else:
            arr = np.ascontiguousarray(np.asarray(P, dtype=np.float32))
            if arr.ndim != 2 or arr.shape[1] != K:
                raise ValueError(f"P must be (n, {K}); got shape {arr.shape}")
            ptr, n, flags = arr.ctypes.data, int(arr.shape[0]), _lib.MMC_IN_HOST
        _lib.check(_lib.lib().mmc_targetset_append(self._handle(), ptr, n, flags, _current_stream_ptr(self.device_index)))
        return self

    def read(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """-> rows [first, first + n) on the host, (n, K) float32 (``n=None``: to the end)."""
        total = len(self)
        first = int(first)
        n = total - first if n is None else int(n)
        if first < 0 or n < 0 or first + n > total:
            raise ValueError(f"rows [{first}, {first + n}) outside the set's {total} rows")
        P = np.empty((n, len(self.classes)), np.float32)
        if n:
            _lib.check(_lib.lib().mmc_targetset_read(self._h, first, n, P.ctypes.data, _current_stream_ptr(self.device_index)))
        return P


def as_teacher(teacher):
    """``teacher`` as a ``HeadEnsemble``: one is taken as it is, a ``CalibratedMLP`` / ``Predictor`` is wrapped in an ensemble of one."""
    from .ensemble import HeadEnsemble
    if isinstance(teacher, HeadEnsemble):
        return teacher
    return HeadEnsemble([teacher])   # (refuses anything that is neither a CalibratedMLP nor a Predictor)


def check_teacher(teacher, fs) -> None:
    """The teacher's class list and input width against the set's; ``ValueError`` before the device is touched."""
    from .featureset import FeatureSet
    if not isinstance(fs, FeatureSet):
        raise ValueError(f"fs must be a FeatureSet, got {type(fs).__name__}")
    if not np.array_equal(np.asarray(teacher.classes), fs.classes):
        raise ValueError(f"the teacher's classes {list(teacher.classes)} differ from the feature set's {fs.classes.tolist()}")
    if int(teacher.input_dim) != fs.dim:
        raise ValueError(f"the teacher takes {teacher.input_dim} features, the feature set has {fs.dim}")


def teacher_targets(teacher, fs) -> TargetSet:
    """The teacher's calibrated probabilities of every row of ``fs``, as a ``TargetSet`` aligned with it.  ``teacher``: a
    ``HeadEnsemble`` (its mean, the values ``topk(..., want_proba=True)`` returns), or a ``CalibratedMLP`` / ``Predictor``.  Made on
    the device in the ensemble's chunks (``mmc_ensemble_predict_set``).  A feature row with NaN refuses the fill (``ValueError``)."""
    ens = as_teacher(teacher)
    ts = None
    try:
        check_teacher(ens, fs)
        h = ens._handle()
        if ens.device_index != fs.device_index:
            raise ValueError(f"the teacher is on device {ens.device_index}, the feature set on device {fs.device_index}")
        ts = TargetSet(fs.classes, device=fs.device, reserve_rows=len(fs))
        if len(fs):
            _lib.check(_lib.lib().mmc_ensemble_predict_set(h, fs._handle(), 0, len(fs), ts._handle(), _current_stream_ptr(fs.device_index)))
    except Exception:
        if ts is not None:
            ts.close()
        raise
    finally:
        if ens is not teacher:      # the ensemble of one made here: its device handle is not needed once the rows are there
            ens.close()
    return ts


def distill(teacher, train, ref, val, nbr_epochs: int, *, batch_size: int, alpha: float, temperature: float = 1.0, **kwargs: Any):
    """``train_classifier(train, ref, val, nbr_epochs, batch_size=batch_size, teacher=teacher, **kwargs)`` on a student with
    ``distill_alpha=alpha`` and ``distill_temperature=temperature``: the production head unless ``clf=`` is given, which must then
    carry those two values itself.  -> what ``train_classifier`` returns: a ``CalibratedMLP`` that ``export_artifact`` writes and
    ``load_predictor`` reads like any other."""
    from .torch_classifier import TorchMLPClassifier, check_distillation
    from .training import train_classifier
    check_distillation(alpha, temperature)
    if float(alpha) == 0.0:
        raise ValueError("distill needs alpha > 0 (alpha = 0 is train_classifier)")
    clf = kwargs.pop("clf", None)
    if clf is None:
        clf = TorchMLPClassifier(hidden_layer_sizes=(500, 300, 100), learning_rate_init=1e-4, class_weight=kwargs.pop("class_weight", None),
                                 random_state=0, device=ref.device, distill_alpha=alpha, distill_temperature=temperature)
    elif float(clf.distill_alpha) != float(alpha) or float(clf.distill_temperature) != float(temperature):
        raise ValueError(f"clf has distill_alpha={clf.distill_alpha!r}, distill_temperature={clf.distill_temperature!r}; "
                         f"distill was given alpha={alpha!r}, temperature={temperature!r}")
    return train_classifier(train, ref, val, nbr_epochs, batch_size=batch_size, clf=clf, teacher=teacher, **kwargs)
